"""-m gpu: group-wise grids above the kernel -- the packed layer, the hand-over from GPTQ, the checkpoint and the decode engine.

  1. QuantLinear(groupsize=G).forward against the dense layer built from the same codes and tables in fp64, with and without Kronecker
     U / V (64 x 32) and a rescale vector, at 1 and 40 rows: 2e-3, what tests/test_gpu_dqgemm_v2.py asks of QuantLinear.forward against its
     dense fake-quant twin;
  2. GPTQ.fasterquant(groupsize=64 / 128) on a 256 x 512 Linear at 4 and 3 bits under decode.collect_packed: one packed group-wise layer
     whose weight, read back through forward on the identity, is layer.weight to fp16 rounding; layer.weight and the quantiser left
     behind are bit-equal to a run outside collect_packed; groups of 16 and a 40-row layer stay dense without raising;
  3. quant.save_model -> load_model reproduces the forward bit for bit;
  4. a 2-block OPT-shaped decoder (h 512, ffn 2048, 8 heads, fp16) with all twelve Linears packed group-wise (w4, g128) under DecodeEngine
     at 1 and 4 sequences, with and without the graph, against the same decoder holding the dense fake-quant nn.Linears in mode plain:
     logits of 6 steps behind a 5-token prefill within the 1e-2 of tests/test_gpu_decode_e2e.py, greedy tokens identical; mode "v3_head"
     raises; score() agrees with the log-softmax of prefill(all_logits=True) to 2e-3;
  5. a small Hugging Face OPT through the driver with GPTQ w4 --groupsize 128 under collect_packed -> save_model -> load_model into a
     fresh skeleton -> DecodeEngine.from_hf, against Hugging Face on the dense fake-quant model the driver left."""
import copy
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import groupwise_ref as R  # noqa: E402

F16 = torch.float16


def _rtn_groups(W, bits, G):
    """nearest rounding on a min / max grid per (row, group): codes uint8 [m, d], scale and zero fp32 [m, d / G], and the fp32 weight
    scale * (code - zero) the packed layer stands for"""
    m, d = W.shape
    maxq = 2 ** bits - 1
    w = W.float().reshape(m, d // G, G)
    lo, hi = w.min(-1).values.clamp(max=0), w.max(-1).values.clamp(min=0)
    scale = ((hi - lo) / maxq).clamp(min=1e-8)
    zero = torch.round(-lo / scale)
    codes = torch.clamp(torch.round(w / scale[..., None]) + zero[..., None], 0, maxq)
    What = (scale[..., None] * (codes - zero[..., None])).reshape(m, d)
    return codes.reshape(m, d).to(torch.uint8).contiguous(), scale.contiguous(), zero.contiguous(), What


# ---- 1. the packed layer ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 40])
@pytest.mark.parametrize("operators", [False, True], ids=["plain", "kron"])
def test_groupwise_quantlinear_forward_is_its_dense_twin(operators, rows):
    from quip_amd import ops, method, quant
    m = d = 2048
    bits, G = 4, 128
    g = torch.Generator().manual_seed(3 + rows)
    np.random.seed(0)
    torch.manual_seed(0)
    W = (0.02 * torch.randn(m, d, generator=g)).to(DEV)
    codes, scale, zero, What = _rtn_groups(W, bits, G)
    bias = torch.randn(m, generator=g).to(DEV)
    ql = quant.QuantLinear(d, m, bits=bits, qfn='a', groupsize=G).to(DEV)
    if operators:
        U = ops.OrthoOp(method.gen_rand_ortho_butterfly_noblock(m), DEV)
        V = ops.OrthoOp(method.gen_rand_ortho_butterfly_noblock(d), DEV)
        assert (U.p, U.q) == (V.p, V.q) == (64, 32)
        sWH = (0.5 + torch.rand(d, generator=g)).to(DEV)
        ql.pack(codes, scale, zero, bias=bias, scaleWH=sWH, U=U, V=V)
        dense = U.apply_cols(V.apply_rows(What, transpose=True), transpose=True) / sWH[None, :]        # U^T What V diag(1 / s)
    else:
        ql.pack(codes, scale, zero, bias=bias)
        dense = What
    assert ql.groupwise and ql.gscales.shape == (d // G, m) and ql.gscales.dtype == torch.float32
    holder = nn.Sequential(ql).half()                                             # model.half() must not narrow the tables
    assert ql.gscales.dtype == ql.gzeros.dtype == torch.float32
    x = torch.randn(rows, d, generator=g).to(DEV).half()
    got = holder(x)
    assert got.dtype == F16 and tuple(got.shape) == (rows, m)
    want = x.double() @ dense.double().T + bias.double()
    err = float((got.double() - want).norm() / want.norm())
    print(f"groupwise QuantLinear {'kron' if operators else 'plain'} rows {rows}: rel {err:.3e}")
    assert err <= 2e-3
    got3 = ql(x.reshape(rows, 1, d))                                              # any batch shape
    assert tuple(got3.shape) == (rows, 1, m) and torch.equal(got3.reshape(rows, m), got)
    for call in (ql.to_native3, ql.decode_only, ql.decode_qweight):
        with pytest.raises(ValueError, match="group-wise grid"):
            call()
    assert not quant.fused_ok([ql], 1) and not quant.fused_head_ok(ql, 1, nn.LayerNorm(m))


# ---- 2. GPTQ hand-over -------------------------------------------------------------------------------------------------------------------------
def _gptq_run(W0, H, bits, gs, collect):
    from quip_amd import gptq as GQ, quant as Q, decode
    m, d = W0.shape
    lin = nn.Linear(d, m, bias=False).to(DEV)
    lin.weight.data = W0.clone()
    meth = GQ.GPTQ(lin)
    meth.quantizer = Q.Quantizer()
    meth.quantizer.configure(bits, perchannel=True, sym=False, qfn='a', mse=False)
    meth.H = H.clone()
    meth.preproc(preproc_gptqH=True, percdamp=.01)
    if collect:
        with decode.collect_packed() as packed:
            meth.fasterquant(groupsize=gs)
            meth.free()
        return lin, meth, packed
    meth.fasterquant(groupsize=gs)
    return lin, meth, None


def _problem(m, d, seed):
    g = torch.Generator().manual_seed(seed)
    W0 = (0.05 * torch.randn(m, d, generator=g)).to(DEV)
    X = torch.randn(4 * d, d, generator=g) * (torch.arange(1, d + 1) ** -0.25)
    return W0, (X.T @ X / X.shape[0]).to(DEV)


@pytest.mark.parametrize("bits,gs", [(4, 64), (4, 128), (3, 64), (3, 128)])
def test_gptq_with_groups_hands_over_a_packed_layer(bits, gs):
    from quip_amd import quant
    m, d = 256, 512
    W0, H = _problem(m, d, bits * 10 + gs)
    lin0, meth0, _ = _gptq_run(W0, H, bits, gs, collect=False)
    assert meth0.codes.shape == (m, d) and meth0.codes.dtype == torch.uint8 and meth0.group_scale.shape == (m, d // gs)
    lin, meth, packed = _gptq_run(W0, H, bits, gs, collect=True)
    # collecting changes nothing the driver sees
    assert torch.equal(lin.weight.data, lin0.weight.data)
    assert torch.equal(meth.quantizer.scale, meth0.quantizer.scale) and torch.equal(meth.quantizer.zero, meth0.quantizer.zero)
    assert tuple(meth.quantizer.scale.shape) == (m, 1)
    assert len(packed.layers) == 1 and packed.layers[0][0] is lin
    ql = packed.layers[0][1]
    assert isinstance(ql, quant.QuantLinear) and ql.groupwise and ql.groupsize == gs and ql.bits == bits and ql.qfn == 'a'
    assert ql.U is None and ql.V is None and ql.bias is None
    # the codes and tables ARE the fake-quant weight
    Wq = lin.weight.data.float()
    back = R.dense_weight(meth0.codes.cpu().numpy(), meth0.group_scale.cpu().numpy(), meth0.group_zero.cpu().numpy(), gs)
    assert np.abs(back - Wq.double().cpu().numpy()).max() <= 1e-6 * float(Wq.abs().max())
    # ... and so is the packed layer, read back through forward on the identity, to fp16 rounding (2^-11 relative, doubled for the
    # one-ulp fp32 difference between scale * (q - zero) here and in the quantiser)
    got = ql(torch.eye(d, dtype=F16, device=DEV)).float().t()
    assert bool(((got - Wq).abs() <= 2.0 ** -10 * Wq.abs() + 1e-7).all()), float((got - Wq).abs().max())


@pytest.mark.parametrize("m,gs", [(256, 16), (40, 64)])
def test_what_the_kernel_cannot_hold_stays_dense(capsys, m, gs):
    d = 512
    W0, H = _problem(m, d, m + gs)
    lin0, meth0, _ = _gptq_run(W0, H, 4, gs, collect=False)
    lin, meth, packed = _gptq_run(W0, H, 4, gs, collect=True)                      # does not raise
    assert packed.layers == [] and torch.equal(lin.weight.data, lin0.weight.data)
    out = capsys.readouterr().out
    assert out.count("stays dense") == 1 and f"{m} x {d}" in out


# ---- 3. checkpoint -----------------------------------------------------------------------------------------------------------------------------
def test_save_model_load_model_round_trip(tmp_path):
    from quip_amd import quant
    m, d, bits, G = 256, 512, 4, 64
    g = torch.Generator().manual_seed(9)
    mk = lambda: nn.Sequential(nn.LayerNorm(d), nn.Linear(d, m), nn.ReLU(), nn.Linear(m, 48)).to(DEV).half()
    model = mk()
    codes, scale, zero, _ = _rtn_groups(model[1].weight.data, bits, G)
    ql = quant.QuantLinear(d, m, bits=bits, qfn='a', groupsize=G).to(DEV).pack(codes, scale, zero, bias=model[1].bias.data)
    x = torch.randn(7, d, generator=g).to(DEV).half()
    layers = {"1": ql}
    path = str(tmp_path / "gw_model.pt")
    quant.save_model(model, layers, path)                                         # (before the layer is installed)
    quant.make_quant(model, layers)
    assert model[1] is ql
    want = model(x)
    fresh = mk()
    loaded = quant.load_model(fresh, path, DEV)
    q2 = loaded["1"]
    assert fresh[1] is q2 and q2 is not ql and q2.groupwise and q2.groupsize == G
    for name in ("qweight", "gscales", "gzeros", "bias"):
        assert torch.equal(getattr(q2, name), getattr(ql, name)), name
    assert torch.equal(fresh(x), want)
    p2 = str(tmp_path / "gw_layers.pt")
    quant.save_packed(layers, p2)
    q3 = quant.load_packed(p2, DEV)["1"]
    assert q3.groupsize == G and torch.equal(q3(x), ql(x))


# ---- 4. engine ---------------------------------------------------------------------------------------------------------------------------------
H_, FFN, HEADS, VOCAB, MAXPOS, NAMES = 512, 2048, 8, 512, 64, ("q_proj", "k_proj", "v_proj", "out_proj", "fc1", "fc2")
_BUILT = {}


def _decoders():
    """(dense fake-quant decoder, the same decoder with the twelve Linears packed group-wise), built once"""
    if _BUILT:
        return _BUILT["dense"], _BUILT["packed"]
    from quip_amd import decode, quant
    torch.manual_seed(21)
    blocks = [decode.OPTBlock.random(H_, FFN, HEADS, F16) for _ in range(2)]
    dense = decode.OPTDecoder(nn.Embedding(VOCAB, H_, dtype=F16), nn.Embedding(MAXPOS + 2, H_, dtype=F16), blocks, nn.LayerNorm(H_, dtype=F16), HEADS)
    for p in dense.parameters():
        if p.dim() > 1:
            p.data.normal_(0, 0.05)
        else:
            p.data.add_(0.05 * torch.randn_like(p))
    dense.tok.weight.data.normal_(0, 0.5)
    dense = dense.to(DEV).eval()
    # an untied head with small entries: |logit| stays near 1, so the fp16 rounding of the logits that the score test's REFERENCE carries
    # (2^-10 max|logit| on a log-probability, tests/test_gpu_score_engine.py) stays under that test's 2e-3
    dense._head_w = (0.01 * torch.randn(VOCAB, H_)).to(F16).to(DEV)
    packed = copy.deepcopy(dense)
    for bd, bp in zip(dense.blocks, packed.blocks):
        for n in NAMES:
            lin = getattr(bd, n)
            codes, scale, zero, What = _rtn_groups(lin.weight.data, 4, 128)
            lin.weight.data = What.to(F16)                                         # the dense fake-quant twin
            m, d = What.shape
            setattr(bp, n, quant.QuantLinear(d, m, bits=4, qfn='a', groupsize=128).to(DEV).pack(codes, scale, zero, bias=lin.bias.data))
    _BUILT.update(dense=dense, packed=packed)
    return dense, packed


def _prefill_then_steps(eng, prompt, toks=None, steps=6):
    """logits after the prompt and after each of `steps` tokens: its own greedy ones, or `toks` teacher-forced"""
    eng.reset()
    out = [eng.prefill(prompt).float().clone()]
    fed = []
    for i in range(steps):
        t = out[-1].argmax(-1) if toks is None else toks[i]
        fed.append(t.clone())
        out.append(eng.forward(t).float().clone())
    return torch.stack(out), torch.stack(fed)


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("bs", [1, 4])
def test_engine_on_groupwise_layers_matches_the_dense_fake_quant_decoder(bs, graph):
    from quip_amd import decode
    dense, packed = _decoders()
    assert len(decode.groupwise_layers(packed)) == 12 and decode.groupwise_layers(dense) == []
    prompt = torch.randint(0, VOCAB, (bs, 5), generator=torch.Generator().manual_seed(50 + bs)).to(DEV)
    ref_eng = decode.DecodeEngine(dense, bs=bs, max_len=MAXPOS, mode="plain", graph=graph)
    ref, toks = _prefill_then_steps(ref_eng, prompt)
    eng = decode.DecodeEngine(packed, bs=bs, max_len=MAXPOS, graph=graph)
    assert eng.mode == "fused", eng.mode                                           # never a fused decode launch
    got, _ = _prefill_then_steps(eng, prompt, toks)
    worst = max(float((got[i, b] - ref[i, b]).norm() / ref[i, b].norm()) for i in range(got.shape[0]) for b in range(bs))
    print(f"groupwise engine bs {bs} graph {graph}: worst relative logits error {worst:.3e}")
    assert worst <= 1e-2
    assert torch.equal(got.argmax(-1), ref.argmax(-1))                            # the greedy tokens
    free, own = _prefill_then_steps(eng, prompt)                                   # ... also free-running
    assert torch.equal(own, toks)
    e2 = decode.DecodeEngine(packed, bs=bs, max_len=MAXPOS, mode="plain", graph=graph)
    got2, _ = _prefill_then_steps(e2, prompt, toks)
    assert max(float((got2[i, b] - ref[i, b]).norm() / ref[i, b].norm()) for i in range(got2.shape[0]) for b in range(bs)) <= 1e-2


def test_engine_refuses_the_fused_launches_and_scores():
    from quip_amd import decode
    _, packed = _decoders()
    for mode in ("v3", "v3_head"):
        with pytest.raises(ValueError, match=r"blocks\.0\.q_proj"):
            decode.DecodeEngine(packed, bs=1, max_len=MAXPOS, mode=mode)
    assert decode.best_mode(packed, 1, F16, MAXPOS) == "fused"
    bs = 2
    ids = torch.randint(0, VOCAB, (bs, 5), generator=torch.Generator().manual_seed(8)).to(DEV)
    eng = decode.DecodeEngine(packed, bs=bs, max_len=MAXPOS)
    lg = eng.prefill(ids, all_logits=True).double()
    eng.reset()
    logprob, greedy = eng.score(ids)
    want = torch.log_softmax(lg, dim=-1)[:, :-1].gather(2, ids[:, 1:, None])[..., 0]
    err = float((logprob[:, :-1].double() - want).abs().max())
    assert 2.0 ** -10 * float(lg.abs().max()) <= 1e-3, "the reference's own rounding is too coarse for the gate below"
    print(f"groupwise engine score: max |delta logprob| {err:.3e}")
    assert err <= 2e-3


# ---- 5. the whole path: driver --groupsize 128 -> collect_packed -> save -> load -> DecodeEngine.from_hf ---------------------------------------
def test_driver_with_groupsize_packs_saves_reloads_and_generates(tmp_path):
    """a small Hugging Face OPT through the driver's call sequence (tests/test_gpu_decode_e2e.py's, GPTQ w4 with --groupsize 128): all
    twelve Linears come back group-wise, the packed checkpoint reloads into a fresh skeleton, and the engine over it agrees with
    Hugging Face on the SAME model object as the driver left it (dense fake-quant weights) within that file's 1e-2"""
    import types
    from transformers import OPTConfig, OPTForCausalLM
    from quip_amd import decode, quant
    import test_gpu_decode_e2e as E
    from test_gpu_decode_hf import hf_generate, _gate
    import run_reference_driver as RD
    ntok = 8
    cfg = OPTConfig(hidden_size=H_, ffn_dim=FFN, num_hidden_layers=2, num_attention_heads=HEADS, word_embed_proj_dim=H_, vocab_size=VOCAB,
                    max_position_embeddings=MAXPOS, dropout=0.0, attention_dropout=0.0, activation_dropout=0.0, layerdrop=0.0)
    mk = lambda: OPTForCausalLM(cfg).half().to(DEV).eval()
    model = mk()
    E._init(model, 31)
    model.seqlen = MAXPOS
    drv, _ = RD.load_driver()
    rs = np.random.RandomState(5)
    batches = [(torch.from_numpy(rs.randint(0, VOCAB, size=(1, MAXPOS))).long(), None) for _ in range(8)]
    args = types.SimpleNamespace(nsamples=8, quant="gptq", wbits=4, qbits=4, qfn="a", npasses=0, unbiased=False, lazy_batch=False, percdamp=0.01,
                                 pre_gptqH=True, pre_rescale=False, pre_proj=False, pre_proj_extra=0, groupsize=128)
    np.random.seed(0)
    torch.manual_seed(0)
    with decode.collect_packed() as packed:
        drv(model, batches, torch.device(DEV), args)
    model.to(DEV)
    assert len(packed.layers) == 12 and all(q.groupwise and q.groupsize == 128 and q.bits == 4 for _, q in packed.layers)
    toks, ref = hf_generate(copy.deepcopy(model), 7, ntok)                       # the dense fake-quant model under Hugging Face
    path = str(tmp_path / "opt_g128.pt")
    quant.save_model(model, packed.named(model), path)
    fresh = mk()
    layers = quant.load_model(fresh, path, DEV)
    assert len(layers) == 12 and all(q.groupwise for q in layers.values())
    eng = decode.DecodeEngine.from_hf(fresh, max_len=MAXPOS)
    assert eng.mode == "fused", eng.mode
    got = torch.stack([eng.forward(t)[0].float().clone() for t in toks])
    rel, decisive, _ = _gate("opt-gptq-g128", got, ref, toks)
    print(f"driver --groupsize 128 -> packed -> reloaded -> engine: worst relative logits error {rel:.3e}, {decisive} of {ntok} steps decisive")
    eng.reset()
    gen = eng.generate(toks[0], ntok - 1)[:, 0].tolist()
    if decisive == ntok:
        assert gen == toks[1:], (gen, toks[1:])
