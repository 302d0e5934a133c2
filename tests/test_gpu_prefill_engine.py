"""-m gpu: DecodeEngine.prefill / generate(prompt) / perplexity against the Hugging Face model, with the helpers, builders and the gate
(max relative logits error 1e-2, greedy tokens equal on decisive steps) of tests/test_gpu_decode_hf.py.

  1. dense twins (mode plain) of OPT and Llama (multi-head and grouped-query): prefill(all_logits=True) against HF's full-sequence logits
     at every position, the caches against HF's past_key_values within the attention gate;
  2. packed w2 models with incoherence operators in modes fused / v3 / v3_head, and a native 3-bit one: prefill, then 16 teacher-forced
     steps by graph replay, against HF holding the dense twins (prompt in one call, then past_key_values);
  3. the engine against itself: prefill vs the token-by-token path, chunked vs one pass, prefill(a) + prefill(b) vs prefill(a | b),
     reset and repeat (bit for bit);
  4. Llama-2-7B width at max_len 4096: prefill 4080, then 16 steps to the end of the context;
  5. perplexity == exp(mean CE) from the all_logits the same engine returned; the refusals leave caches and position untouched."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import prefill_ref as R  # noqa: E402
from test_gpu_decode_hf import _load, _gate, hf_opt_from_decoder, _llama7b  # noqa: E402
from test_gpu_decode_gqa import hf_llama_gqa  # noqa: E402

NTOK = 16
MAXPOS = 768
VOCAB = 512
DT = torch.float16


def _randomise(dec, seed=0):
    torch.manual_seed(seed)
    for p_ in dec.parameters():
        if p_.dim() > 1:
            p_.data.normal_(0, 0.02)
        else:
            p_.data.add_(0.05 * torch.randn_like(p_))


def _fp32_rotary(hf, hd):
    """.to(float16) rounded HF's rotary frequencies (harmless over 64 positions, not over 700): give it the decoder's fp32 ones, as
    test_gpu_decode_hf._llama7b does"""
    inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd))
    rot = hf.model.rotary_emb
    rot.inv_freq = inv.to(DEV)
    rot.original_inv_freq = inv.to(DEV)


_BUILT = {}


def _pack_llama(dec, bits, native3):
    """decode_llama.pack_model with the layout as a parameter: nearest-rounded qfn-b codes, Kronecker U / V, random scaleWH, dense twins"""
    from quip_amd import ops, method
    from quip_amd.quant import QuantLinear
    np.random.seed(0)
    torch.manual_seed(0)
    dense = {}
    for li, blk in enumerate(dec.blocks):
        for name in dec.NAMES:
            lin = getattr(blk, name)
            m, d = lin.weight.shape
            W = lin.weight.data
            s = ops.qfnb_scale(W)
            What, codes = ops.quantize(W, 'b', s, None, 2 ** bits - 1, want_codes=True)
            U = ops.OrthoOp(method.gen_rand_ortho_butterfly_noblock(m), DEV)
            V = ops.OrthoOp(method.gen_rand_ortho_butterfly_noblock(d), DEV)
            sWH = (0.5 + torch.rand(d)).to(DEV)
            ql = QuantLinear(d, m, bits=bits, qfn='b', native3=native3).to(DEV)
            ql.pack(codes, s, None, bias=None, scaleWH=sWH, U=U, V=V)
            setattr(blk, name, ql)
            dense[(li, name)] = (U.apply_cols(V.apply_rows(What.float(), transpose=True), transpose=True) / sWH[None, :]).to(W.dtype)
    return dense


def _model(kind):
    """(decoder, HF model holding the same / the twin weights), built once: opt_dense, llama_dense, gqa_dense, opt_w2, llama_w2, llama_w3n"""
    if kind in _BUILT:
        return _BUILT[kind]
    arch, what = kind.split("_")
    if arch == "opt":
        D = _load("decode_opt")
        dec = D.Decoder(layers=2, h=2048, ffn=8192, heads=32, vocab=VOCAB, maxpos=MAXPOS, dtype=DT).to(DEV).eval()
        _randomise(dec)
        if what == "dense":
            for b in dec.blocks:
                b.fused_attn = True
            twin = {(li, n): (getattr(b, n).weight.data, getattr(b, n).bias.data) for li, b in enumerate(dec.blocks)
                    for n in ("q_proj", "k_proj", "v_proj", "out_proj", "fc1", "fc2")}
        else:
            twin, _ = D.pack_model(dec, 2, DEV)
        hf = hf_opt_from_decoder(dec, twin, 32, MAXPOS, DT, DEV)
    else:
        L = _load("decode_llama")
        kv = 4 if arch == "gqa" else None
        dec = L.Decoder(layers=2, h=2048, ffn=11008, heads=16, kv_heads=kv, vocab=VOCAB, maxpos=MAXPOS, eps=1e-5, dtype=DT).to(DEV).eval()
        _randomise(dec)
        if what == "dense":
            twin = {(li, n): getattr(b, n).weight.data for li, b in enumerate(dec.blocks) for n in L.Decoder.NAMES}
        elif what == "w3n":
            twin = _pack_llama(dec, 3, True)
            assert dec.blocks[0].q_proj.native3
        else:
            twin, _ = L.pack_model(dec, 2, DEV)
        hf = hf_llama_gqa(dec, twin, 16, kv or 16, MAXPOS, 1e-5, DT)
        _fp32_rotary(hf, 128)
    _BUILT[kind] = (dec, hf)
    return dec, hf


def _prompts(bs, n, seed):
    return torch.randint(0, VOCAB, (bs, n), generator=torch.Generator().manual_seed(seed)).to(DEV)


@torch.no_grad()
def _hf_prompt_then_steps(hf, prompts, ntok=NTOK):
    """HF: the prompt in one call, then ntok greedy steps on past_key_values.  Returns (logits of the last prompt position [bs, vocab],
    tokens fed at the steps [ntok, bs], their logits [ntok, bs, vocab], full-sequence prompt logits [bs, n, vocab], past_key_values of
    the prompt as [(K, V)] per layer)"""
    out = hf(input_ids=prompts, use_cache=True)
    pkv = out.past_key_values
    kvs = [(l.keys.clone(), l.values.clone()) for l in pkv.layers]
    full = out.logits.float().clone()
    ids = full[:, -1].argmax(-1, keepdim=True)
    toks, logits = [], []
    for _ in range(ntok):
        o = hf(input_ids=ids, past_key_values=pkv, use_cache=True)
        pkv = o.past_key_values
        lg = o.logits[:, -1].float()
        toks.append(ids[:, 0].clone())
        logits.append(lg.clone())
        ids = lg.argmax(-1, keepdim=True)
    if not ntok:
        return full[:, -1], None, None, full, kvs
    return full[:, -1], torch.stack(toks), torch.stack(logits), full, kvs


def _gate_steps(name, eng, first, toks, ref0, ref, tol=1e-2):
    """first: the engine's logits after the prompt; then teacher-force HF's tokens through the engine, every step a graph replay"""
    got = [first.float().clone()]
    for t in toks:
        got.append(eng.forward(t).float().clone())
    got = torch.stack(got)                                                   # [1 + ntok, bs, vocab]
    want = torch.cat([ref0[None], ref])
    worst = 0.0
    for b in range(got.shape[1]):
        worst = max(worst, _gate(f"{name}-seq{b}", got[:, b], want[:, b], None, tol)[0])
    return worst


# ---------------------------------------------------------------------------------------------------------------- 1. dense twins
@pytest.mark.parametrize("kind", ["opt_dense", "llama_dense", "gqa_dense"])
def test_dense_prefill_matches_hf_at_every_position_and_in_the_caches(kind):
    from quip_amd import decode
    dec, hf = _model(kind)
    bs, n = 2, 130
    prompts = _prompts(bs, n, 1)
    _, _, _, full, kvs = _hf_prompt_then_steps(hf, prompts, ntok=0)
    eng = decode.DecodeEngine(dec, bs=bs, max_len=MAXPOS, mode="plain")
    got = eng.prefill(prompts, all_logits=True).float()
    assert got.shape == (bs, n, VOCAB) and eng._steps == n and int(eng.pos) == n
    assert torch.equal(eng.logits.float(), got[:, -1])
    assert torch.equal(got[:, -1].gather(1, eng.ids[:, None])[:, 0], got[:, -1].max(-1).values)     # `ids` holds the argmax of the last position
    worst = max(_gate(f"{kind}-seq{b}", got[b], full[b], None)[0] for b in range(bs))
    for (kc, vc), (K, V) in zip(eng.caches, kvs):
        assert kc.shape[1] == K.shape[1] == dec.kv_heads
        for mine, want in ((kc[:, :, :n], K), (vc[:, :, :n], V)):
            ok, frac = R.within_gate(mine, want, DT)
            assert ok, (kind, frac)
        assert not bool(kc[:, :, n:].any()) and not bool(vc[:, :, n:].any())              # nothing behind the prompt
    print(f"{kind}: prefill of {n} vs HF at every position, worst max-rel logits err {worst:.2e}")


# ---------------------------------------------------------------------------------------------------------------- 2. packed models
SHAPES = [(1, 1), (1, 5), (1, 130), (1, 700), (3, 5), (3, 700), (16, 1), (16, 130)]       # (sequences, prompt length)


@pytest.mark.parametrize("kind", ["opt_w2", "llama_w2"])
def test_packed_prefill_then_greedy_steps_match_hf(kind):
    from quip_amd import decode
    dec, hf = _model(kind)
    report = {}
    for bs, n in SHAPES:
        prompts = _prompts(bs, n, 100 * bs + n)
        ref0, toks, ref, _, _ = _hf_prompt_then_steps(hf, prompts)
        for mode in (("fused", "v3", "v3_head") if bs <= 4 else ("fused", "v3")):
            eng = decode.DecodeEngine(dec, bs=bs, max_len=MAXPOS, mode=mode)
            assert eng.mode == mode
            first = eng.prefill(prompts)
            assert first is eng.logits and eng._steps == n and int(eng.pos) == n
            report[(bs, n, mode)] = round(_gate_steps(f"{kind}-{mode}-bs{bs}-n{n}", eng, first, toks, ref0, ref), 5)
            assert eng._graph is not None and eng._steps == n + NTOK and int(eng.pos) == n + NTOK       # the steps ran by graph replay
            del eng
    print(f"{kind}: prefill + {NTOK} steps vs HF, worst max-rel logits err per (bs, prompt, mode):", report)


def test_native_3bit_prefill_then_greedy_steps_match_hf():
    from quip_amd import decode
    dec, hf = _model("llama_w3n")
    for bs, n in ((1, 130), (3, 5)):
        prompts = _prompts(bs, n, 7 + n)
        ref0, toks, ref, _, _ = _hf_prompt_then_steps(hf, prompts)
        eng = decode.DecodeEngine(dec, bs=bs, max_len=MAXPOS)
        rel = _gate_steps(f"w3n-bs{bs}-n{n}", eng, eng.prefill(prompts), toks, ref0, ref)
        assert eng._graph is not None and eng._steps == n + NTOK
        print(f"native 3-bit llama, mode {eng.mode}, bs {bs}, prompt {n}: worst max-rel logits err {rel:.2e}")


@pytest.mark.parametrize("kind", ["opt_w2", "llama_w2"])
def test_generate_from_a_prompt_is_hf_greedy_while_hf_is_decisive(kind):
    from quip_amd import decode
    dec, hf = _model(kind)
    bs, n = 2, 40
    prompts = _prompts(bs, n, 3)
    ref0, toks, ref, _, _ = _hf_prompt_then_steps(hf, prompts)
    for mode in ("v3_head", "fused"):
        eng = decode.DecodeEngine(dec, bs=bs, max_len=MAXPOS, mode=mode)
        out = eng.generate(prompts, NTOK)                                    # [NTOK, bs]: the tokens following the prompt
        assert out.shape == (NTOK, bs) and eng._steps == n + NTOK - 1
        # logits within the gate (1e-2 relative l2, asserted by the tests above) differ by at most 1e-2 |ref| in any entry: a top-1 margin above
        # twice that is decisive, as _gate defines it.  Compare up to HF's first step without such a margin, per sequence.
        allref = torch.cat([ref0[None], ref])[:NTOK]
        top2 = allref.topk(2, dim=-1).values
        sure = ((top2[..., 0] - top2[..., 1]) > 2e-2 * allref.norm(dim=-1)).cumprod(0).bool()
        assert bool((out[sure] == toks[sure]).all())
        print(f"{kind} {mode}: generate from a prompt, {int(sure.sum())} of {sure.numel()} tokens compared with HF's greedy ones")
        one = eng.generate(int(toks[0, 0]), 2)                               # int / 1-D inputs behave as before
        assert one.shape == (2, bs)


# ---------------------------------------------------------------------------------------------------------------- 3. the engine against itself
@pytest.mark.parametrize("kind", ["opt_w2", "llama_w2"])
def test_prefill_and_the_token_by_token_path_both_match_hf(kind):
    from quip_amd import decode
    dec, hf = _model(kind)
    bs, n = 3, 130
    prompts = _prompts(bs, n, 11)
    ref0 = _hf_prompt_then_steps(hf, prompts, ntok=0)[0]
    eng = decode.DecodeEngine(dec, bs=bs, max_len=MAXPOS)
    a = eng.prefill(prompts).float().clone()
    eng.reset()
    for i in range(n):
        b = eng.forward(prompts[:, i])
    b = b.float().clone()
    for name, got in (("prefill", a), ("token by token", b)):
        rel = ((got - ref0).norm(dim=1) / ref0.norm(dim=1)).max().item()
        assert rel <= 1e-2, (kind, name, rel)
    mutual = ((a - b).norm(dim=1) / b.norm(dim=1)).max().item()
    print(f"{kind} mode {eng.mode}: prefill vs token by token, mutual max-rel logits difference {mutual:.2e} (not gated)")


def test_chunked_prefill_against_one_pass():
    from quip_amd import decode
    bs, n = 2, 300
    prompts = _prompts(bs, n, 21)
    for kind in ("llama_w2", "opt_w2", "llama_dense", "opt_dense"):
        dec, hf = _model(kind)
        ref0 = _hf_prompt_then_steps(hf, prompts, ntok=0)[0]
        mode = "plain" if kind.endswith("dense") else "auto"
        e1 = decode.DecodeEngine(dec, bs=bs, max_len=MAXPOS, mode=mode)
        e2 = decode.DecodeEngine(dec, bs=bs, max_len=MAXPOS, mode=mode)
        a = e1.prefill(prompts).float().clone()
        b = e2.prefill(prompts, chunk=128).float().clone()
        assert e2._steps == n and int(e2.pos) == n
        for name, got in (("one pass", a), ("chunk=128", b)):
            rel = ((got - ref0).norm(dim=1) / ref0.norm(dim=1)).max().item()
            assert rel <= 1e-2, (kind, name, rel)
        if kind.endswith("dense"):                                           # dense fp16 layers: block 0's K rows are the same bits
            assert torch.equal(e1.caches[0][0][:, :, :n], e2.caches[0][0][:, :, :n]), kind
        del e1, e2
    dec, _ = _model("llama_dense")
    e3 = decode.DecodeEngine(dec, bs=bs, max_len=MAXPOS, mode="plain")
    one = e3.prefill(prompts[:, :200], all_logits=True).float().clone()
    e3.reset()
    cut = e3.prefill(prompts[:, :200], chunk=64, all_logits=True).float()
    assert cut.shape == one.shape == (bs, 200, VOCAB)
    assert ((cut - one).norm(dim=-1) / one.norm(dim=-1)).max().item() <= 1e-2


@pytest.mark.parametrize("kind", ["opt_w2", "llama_w2", "gqa_dense"])
def test_prefill_continues_a_sequence_and_repeats_after_reset(kind):
    from quip_amd import decode
    dec, hf = _model(kind)
    bs, na, nb = 2, 70, 45
    prompts = _prompts(bs, na + nb, 31)
    ref0 = _hf_prompt_then_steps(hf, prompts, ntok=0)[0]
    eng = decode.DecodeEngine(dec, bs=bs, max_len=MAXPOS, mode="plain" if kind.endswith("dense") else "auto")
    whole = eng.prefill(prompts).float().clone()
    kc_whole = eng.caches[-1][0].clone()
    eng.reset()
    eng.prefill(prompts[:, :na])
    assert eng._steps == na
    parts = eng.prefill(prompts[:, na:]).float().clone()
    assert eng._steps == na + nb and int(eng.pos) == na + nb
    for name, got in (("cat", whole), ("a then b", parts)):
        rel = ((got - ref0).norm(dim=1) / ref0.norm(dim=1)).max().item()
        assert rel <= 1e-2, (kind, name, rel)
    eng.reset()
    again = eng.prefill(prompts).float()
    assert torch.equal(again, whole) and torch.equal(eng.caches[-1][0], kc_whole)        # reset, then the same bits
    eng.step()
    eng.step()
    assert eng._graph is not None and eng._steps == na + nb + 2


# ---------------------------------------------------------------------------------------------------------------- 4. Llama-2-7B width
@torch.no_grad()
def test_llama_7b_width_prefill_4080_then_steps_to_the_end_of_the_context():
    """test_llama_7b_width_engine_near_the_end_of_its_context_matches_hf with HF's prefill replaced by the engine's own"""
    from quip_amd import decode
    dec, hf = _llama7b(4096)
    bs, start, maxlen = 9, 4080, 4096
    g = torch.Generator().manual_seed(4080)
    prompts = torch.randint(0, dec.tok.weight.shape[0], (bs, start), generator=g).to(DEV)
    ref0, toks, ref = [], [], []
    for s in range(bs):                                                      # HF one sequence at a time (its eager attention at 4080 rows)
        r0, t, r, _, _ = _hf_prompt_then_steps(hf, prompts[s:s + 1], ntok=maxlen - start)
        ref0.append(r0), toks.append(t), ref.append(r)
    ref0, toks, ref = torch.cat(ref0), torch.cat(toks, dim=1), torch.cat(ref, dim=1)
    eng = decode.DecodeEngine(dec, bs=bs, max_len=maxlen)
    assert eng.mode in ("v3", "v3_head"), eng.mode
    first = eng.prefill(prompts)
    assert eng._steps == start
    worst = _gate_steps("llama7b-prefill", eng, first, toks, ref0, ref)
    assert eng._steps == maxlen and eng._graph is not None
    with pytest.raises(RuntimeError, match="KV cache"):
        eng.prefill(prompts[:, :1])                                          # the cache is full
    print(f"llama 7b width, {bs} sequences, prefill {start} + {maxlen - start} steps, mode {eng.mode} vs HF: worst max-rel logits err {worst:.2e}")


# ---------------------------------------------------------------------------------------------------------------- 5. perplexity, refusals
@pytest.mark.parametrize("kind", ["opt_w2", "llama_dense"])
def test_perplexity_is_exp_mean_cross_entropy_of_the_engines_own_logits(kind):
    from quip_amd import decode
    dec, _ = _model(kind)
    nsamples, seqlen, bs = 5, 96, 2                                          # the last pass is short of a full batch
    ids = _prompts(nsamples, seqlen, 41)
    eng = decode.DecodeEngine(dec, bs=bs, max_len=MAXPOS, mode="plain" if kind.endswith("dense") else "auto")
    got = eng.perplexity(ids)
    assert eng._steps == 0 and int(eng.pos) == 0
    nlls = []
    for lo in range(0, nsamples, bs):                                        # opt.py:287-296 on the all_logits of the same engine
        batch = ids[lo:lo + bs]
        real = batch.shape[0]
        if real < bs:
            batch = torch.cat([batch, batch[:1].expand(bs - real, seqlen)])
        eng.reset()
        lg = eng.prefill(batch, all_logits=True)
        for r in range(real):
            shift_logits = lg[r:r + 1, :-1, :].float().contiguous()
            shift_labels = batch[r:r + 1, 1:]
            loss = nn.CrossEntropyLoss()(shift_logits.view(-1, shift_logits.size(-1)), shift_labels.reshape(-1))
            nlls.append(loss.float() * seqlen)
    want = torch.exp(torch.stack(nlls).sum() / (nsamples * seqlen))
    assert torch.allclose(torch.tensor(got), want.cpu().float()), (got, float(want))
    assert np.isfinite(got) and got > 1.0
    print(f"{kind}: perplexity {got:.3f} over {nsamples} x {seqlen}")


def test_module_level_perplexity_on_an_hf_model():
    from quip_amd import decode
    _, hf = _model("llama_dense")
    hf.seqlen = 64
    testenc = _prompts(1, 64 * 3 + 10, 51)
    ppl = decode.perplexity(hf, testenc)
    eng = hf.__dict__["_quip_decode_engine"]
    assert eng.max_len == 64 and abs(ppl - eng.perplexity(testenc[0, :192].view(3, 64))) <= 1e-5 * ppl
    del hf.__dict__["_quip_decode_engine"]


def test_refusals_leave_caches_and_position_untouched():
    from quip_amd import decode
    from quip_amd.quant import QuantLinear
    dec, _ = _model("opt_w2")
    eng = decode.DecodeEngine(dec, bs=2, max_len=64)
    eng.prefill(_prompts(2, 10, 61))
    snap = [(kc.clone(), vc.clone()) for kc, vc in eng.caches]

    def untouched():
        return (int(eng.pos) == 10 and eng._steps == 10 and all(torch.equal(kc, a) and torch.equal(vc, b) for (kc, vc), (a, b) in zip(eng.caches, snap)))
    with pytest.raises(RuntimeError, match="does not fit the KV cache"):
        eng.prefill(_prompts(2, 55, 62))                                     # 10 + 55 > 64
    assert untouched()
    with pytest.raises(ValueError, match="bs = 2"):
        eng.prefill(_prompts(3, 4, 63))
    with pytest.raises(ValueError, match="n >= 1"):
        eng.prefill(_prompts(2, 4, 63)[:, :0])
    assert untouched()
    # a layer that kept only its decode-order codes: forward cannot run, and prefill says so before it writes
    lay = dec.blocks[1].fc1
    keep = lay.qweight
    try:
        lay.decode_qweight()
        lay.qweight = torch.empty(0, dtype=torch.int32, device=DEV)          # what QuantLinear.decode_only() leaves
        with pytest.raises(RuntimeError, match=r"decode_only\(\).*token by token"):
            eng.prefill(_prompts(2, 4, 64))
        assert untouched()
    finally:
        lay.qweight = keep
    eng.prefill(_prompts(2, 4, 64))
    assert eng._steps == 14
