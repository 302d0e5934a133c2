"""-m gpu: grouped-query decode attention (quipamd_decode_attention_grouped, csrc/decode_gqa.hip) and the Llama decode engine on
grouped-query models.

  1. the op against fp64 attention over HF's repeat_kv layout, with the cache append checked exactly (rotary: bit-identical to
     rope_inplace + append), out-of-range positions, run-to-run identity and hipGraph replay with the device position;
  2. the engine (plain and fused, 1 and 16 sequences) against LlamaForCausalLM with num_key_value_heads < num_attention_heads fed
     with past_key_values, on the dense twin weights of the packed layers (test_gpu_decode_hf.py's gates);
  3. LDLQ w2 with incoherence through the restated llama_sequential -> collect_packed -> DecodeEngine.from_hf vs the fake-quant model;
  4. Llama-2-70B-width blocks (8192 / 28672, 64 heads over 8 key / value heads)."""
import copy
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "scripts"))
NTOK = 16


# ---------------------------------------------------------------------------------------------------------------- 1. the op
def _ref(q, k, v, kc, vc, pos, g):
    bs, kv, maxlen, hd = kc.shape
    kc, vc = kc.clone(), vc.clone()
    kc[:, :, pos] = k.view(bs, kv, hd)
    vc[:, :, pos] = v.view(bs, kv, hd)
    K = kc[:, :, :pos + 1].double().repeat_interleave(g, dim=1)            # HF repeat_kv: query head j reads kv head j // g
    V = vc[:, :, :pos + 1].double().repeat_interleave(g, dim=1)
    s = torch.einsum("bhd,bhtd->bht", q.view(bs, kv * g, hd).double(), K) / math.sqrt(hd)
    o = torch.einsum("bht,bhtd->bhd", torch.softmax(s, -1), V)
    return o.reshape(bs, kv * g * hd), kc, vc


def _tables(hd, rows):
    from quip_amd import decode
    inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd))
    return decode.rotary_tables(inv, rows)


CASES = ([(dt, hd, g, bs, 512, pos) for dt in (torch.float16, torch.bfloat16) for hd in (64, 128) for g in (2, 4, 8, 16)
          for bs in (1, 3) for pos in (0, 1, 300, 511)]
         + [(torch.float16, 128, 8, 16, 4096, 4095), (torch.bfloat16, 128, 8, 16, 4096, 2050), (torch.float16, 64, 16, 16, 700, 257),
            (torch.float16, 128, 3, 2, 256, 255), (torch.bfloat16, 64, 5, 1, 1000, 999)])


@pytest.mark.parametrize("dtype,hd,g,bs,maxlen,pos", CASES)
def test_matches_fp64_repeat_kv_attention(dtype, hd, g, bs, maxlen, pos):
    from quip_amd import ops
    kv = 2 if g > 4 else 3
    heads = kv * g
    gen = torch.Generator().manual_seed(pos + 7 * g + hd + bs)
    mk = lambda *s: torch.randn(*s, generator=gen).to(dtype).to(DEV)
    q, k, v = mk(bs, heads * hd), mk(bs, kv * hd), mk(bs, kv * hd)
    kc, vc = mk(bs, kv, maxlen, hd), mk(bs, kv, maxlen, hd)
    want, kc_w, vc_w = _ref(q, k, v, kc, vc, pos, g)
    p = torch.tensor([pos], dtype=torch.int64, device=DEV)
    got = ops.decode_attention_grouped(q, k, v, kc, vc, p)
    assert torch.equal(kc, kc_w) and torch.equal(vc, vc_w)                 # append exact, no other row or head touched
    tol = 2e-3 if dtype == torch.float16 else 1.6e-2                       # test_gpu_decode_attn.py's: the output rounding
    assert (got.double() - want).abs().max().item() <= tol * max(1.0, want.abs().max().item())
    # a caller-owned workspace, reused: the same bits again (fixed-order merge, re-armed counters)
    ws = ops.decode_attention_grouped_workspace(bs, heads, kv, hd, maxlen, DEV)
    kc2, vc2 = kc.clone(), vc.clone()
    r1 = ops.decode_attention_grouped(q, k, v, kc2, vc2, p, workspace=ws)
    r2 = ops.decode_attention_grouped(q, k, v, kc2, vc2, p, workspace=ws)
    assert torch.equal(r1, got) and torch.equal(r2, got)


@pytest.mark.parametrize("dtype,hd,g,pos", [(torch.float16, 128, 8, 0), (torch.float16, 128, 8, 777), (torch.bfloat16, 64, 4, 1500),
                                            (torch.float16, 64, 16, 2047)])
def test_rotary_matches_rope_inplace_then_append(dtype, hd, g, pos):
    from quip_amd import ops
    bs, kv, maxlen = 3, 2, 2048
    heads = g * kv
    cos, sin = _tables(hd, maxlen)
    cos, sin = cos.to(DEV), sin.to(DEV)
    gen = torch.Generator().manual_seed(pos + g)
    mk = lambda *s: torch.randn(*s, generator=gen).to(dtype).to(DEV)
    q, k, v = mk(bs, heads * hd), mk(bs, kv * hd), mk(bs, kv * hd)
    kc, vc = mk(bs, kv, maxlen, hd), mk(bs, kv, maxlen, hd)
    p = torch.tensor([pos], dtype=torch.int64, device=DEV)
    qr, kr = q.clone(), k.clone()
    ops.rope_inplace(qr, kr, cos, sin, p, heads, kv)
    want, kc_w, vc_w = _ref(qr, kr, v, kc, vc, pos, g)
    got = ops.decode_attention_grouped(q, k, v, kc, vc, p, cos, sin)
    assert torch.equal(kc, kc_w) and torch.equal(vc, vc_w)                 # the appended K row is rope_inplace's, bit for bit
    tol = 2e-3 if dtype == torch.float16 else 1.6e-2
    assert (got.double() - want).abs().max().item() <= tol * max(1.0, want.abs().max().item())


def test_out_of_range_position_is_a_no_op():
    from quip_amd import ops
    for pos in (-1, 8, 300):
        for maxlen in (8, 300):
            if pos < maxlen and pos >= 0:
                continue
            kc = torch.ones(2, 2, maxlen, 64, dtype=torch.float16, device=DEV)
            vc = kc.clone()
            q = torch.ones(2, 8 * 64, dtype=torch.float16, device=DEV)
            kv = torch.full((2, 2 * 64), 2.0, dtype=torch.float16, device=DEV)
            out = torch.zeros(2, 8 * 64, dtype=torch.float16, device=DEV)
            out.copy_(ops.decode_attention_grouped(q, kv, kv, kc, vc, torch.tensor([pos], dtype=torch.int64, device=DEV)) * 0)
            assert bool((kc == 1).all()) and bool((vc == 1).all())
    with pytest.raises(RuntimeError):
        x = torch.ones(1, 256)
        ops.decode_attention_grouped(x, x[:, :128], x[:, :128], torch.ones(1, 2, 8, 64), torch.ones(1, 2, 8, 64), torch.tensor([0]))


@pytest.mark.parametrize("maxlen", [64, 1024])
def test_graph_replay_advances_with_the_device_position(maxlen):
    from quip_amd import ops
    bs, g, kv, hd = 2, 4, 2, 128
    heads = g * kv
    cos, sin = _tables(hd, maxlen)
    cos, sin = cos.to(DEV), sin.to(DEV)
    gen = torch.Generator().manual_seed(maxlen)
    mk = lambda *s: torch.randn(*s, generator=gen).half().to(DEV)
    xs = [(mk(bs, heads * hd), mk(bs, kv * hd), mk(bs, kv * hd)) for _ in range(5)]
    kc, vc = torch.zeros(bs, kv, maxlen, hd, dtype=torch.float16, device=DEV), torch.zeros(bs, kv, maxlen, hd, dtype=torch.float16, device=DEV)
    kr, vr = kc.clone(), vc.clone()
    q, k, v = (t.clone() for t in xs[0])
    pos = torch.zeros(1, dtype=torch.int64, device=DEV)
    out = torch.zeros(bs, heads * hd, dtype=torch.float16, device=DEV)
    ws = ops.decode_attention_grouped_workspace(bs, heads, kv, hd, maxlen, DEV)
    start = 0 if maxlen == 64 else 510                                     # 1024: steps 510..514 cross a chunk boundary (merge in the launch)

    def step():
        out.copy_(ops.decode_attention_grouped(q, k, v, kc, vc, pos, cos, sin, workspace=ws))
        pos.add_(1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    fill = mk(bs, kv, maxlen, hd)
    kc.copy_(fill)
    vc.copy_(fill)
    kr.copy_(fill)
    vr.copy_(fill)
    pos.fill_(start)
    for i, (qi, ki, vi) in enumerate(xs):
        q.copy_(qi), k.copy_(ki), v.copy_(vi)
        graph.replay()
        p = torch.tensor([start + i], dtype=torch.int64, device=DEV)
        qr, kr_ = qi.clone(), ki.clone()
        ops.rope_inplace(qr, kr_, cos, sin, p, heads, kv)
        want, kr, vr = _ref(qr, kr_, vi, kr, vr, start + i, g)
        assert (out.double() - want).abs().max().item() < 2e-3 * max(1.0, want.abs().max().item())
    assert int(pos.item()) == start + 5 and torch.equal(kc, kr) and torch.equal(vc, vr)


# ---------------------------------------------------------------------------------------------------------------- 2. engine vs HF
def hf_llama_gqa(dec, twin, heads, kv_heads, maxpos, eps, dtype):
    from transformers import LlamaConfig, LlamaForCausalLM
    ffn = next(W.shape[0] for (li, n), W in twin.items() if n == "gate_proj")
    cfg = LlamaConfig(hidden_size=dec.h, intermediate_size=ffn, num_hidden_layers=len(dec.blocks), num_attention_heads=heads,
                      num_key_value_heads=kv_heads, vocab_size=dec.tok.weight.shape[0], max_position_embeddings=maxpos, rms_norm_eps=eps,
                      rope_theta=10000.0, attention_dropout=0.0, tie_word_embeddings=False, attention_bias=False, mlp_bias=False)
    with torch.device(DEV):
        hf = LlamaForCausalLM(cfg).to(dtype).eval()
    with torch.no_grad():
        hf.model.embed_tokens.weight.copy_(dec.tok.weight)
        hf.model.norm.weight.copy_(dec.norm.weight)
        hf.lm_head.weight.copy_(dec.lm_head.weight)
        for li, (blk, lay) in enumerate(zip(dec.blocks, hf.model.layers)):
            lay.input_layernorm.weight.copy_(blk.n1.weight)
            lay.post_attention_layernorm.weight.copy_(blk.n2.weight)
            for name, tgt in (("q_proj", lay.self_attn.q_proj), ("k_proj", lay.self_attn.k_proj), ("v_proj", lay.self_attn.v_proj),
                              ("o_proj", lay.self_attn.o_proj), ("gate_proj", lay.mlp.gate_proj), ("up_proj", lay.mlp.up_proj),
                              ("down_proj", lay.mlp.down_proj)):
                tgt.weight.copy_(twin[(li, name)])
    return hf


@torch.no_grad()
def hf_batch_logits(hf, toks):
    """teacher-forced: toks int64 [bs, n], one position per call with past_key_values; returns logits [n, bs, vocab] fp32"""
    pkv, out = None, []
    for i in range(toks.shape[1]):
        o = hf(input_ids=toks[:, i:i + 1], past_key_values=pkv, use_cache=True)
        pkv = o.past_key_values
        out.append(o.logits[:, -1].float().clone())
    return torch.stack(out)


def _gqa_decoder(h, ffn, heads, kv_heads, layers, vocab, maxpos, seed=0):
    from test_gpu_decode_hf import _load
    L = _load("decode_llama")
    torch.manual_seed(seed)
    dec = L.Decoder(layers=layers, h=h, ffn=ffn, heads=heads, kv_heads=kv_heads, vocab=vocab, maxpos=maxpos, eps=1e-5,
                    dtype=torch.float16).to(DEV).eval()
    for p_ in dec.parameters():
        if p_.dim() > 1:
            p_.data.normal_(0, 0.02)
    return L, dec


def _engine_vs_hf(dec, hf, bs, mode, maxlen, seed):
    from quip_amd import decode
    from test_gpu_decode_hf import _gate
    vocab = dec.tok.weight.shape[0]
    gen = torch.Generator().manual_seed(seed)
    toks = torch.randint(0, vocab, (bs, NTOK), generator=gen).to(DEV)
    ref = hf_batch_logits(hf, toks)
    eng = decode.DecodeEngine(dec, bs=bs, max_len=maxlen, mode=mode)
    assert eng.mode == mode
    got = torch.stack([eng.forward(toks[:, i]).float().clone() for i in range(NTOK)])
    hd = dec.h // dec.heads
    assert sum(c.numel() * c.element_size() for kc_vc in eng.caches for c in kc_vc) == dec.layers_n * 2 * bs * dec.kv_heads * eng.max_len * hd * 2
    worst = 0.0
    for b in range(bs):
        worst = max(worst, _gate(f"{mode}-bs{bs}-seq{b}", got[:, b], ref[:, b], toks[b].tolist())[0])
    return eng, worst


@pytest.mark.parametrize("h,heads,kv_heads", [(2048, 16, 4), (2048, 16, 8), (2048, 32, 8)])
def test_engine_matches_hf_grouped_query_llama(h, heads, kv_heads):
    from quip_amd import decode
    maxpos = 64
    L, dec = _gqa_decoder(h, 11008, heads, kv_heads, 2, 512, maxpos)
    assert dec.kv_heads == kv_heads and dec.blocks[0].k_proj.out_features == kv_heads * (h // heads)
    twin, _ = L.pack_model(dec, 2, DEV)
    hf = hf_llama_gqa(dec, twin, heads, kv_heads, maxpos, 1e-5, torch.float16)
    assert decode.best_mode(dec, 1, torch.float16) == "fused" and not dec.v3_ok(1)     # v3 / v3_head stay multi-head only
    report = {}
    for bs in (1, 16):
        for mode in ("plain", "fused"):
            _, report[(bs, mode)] = _engine_vs_hf(dec, hf, bs, mode, maxpos, seed=bs + kv_heads)
    eng = decode.DecodeEngine(dec, bs=1, max_len=maxpos)
    assert eng.mode == "fused"
    print(f"gqa engine h={h} heads={heads} kv={kv_heads}:", report)


# ---------------------------------------------------------------------------------------------------------------- 3. end to end
def test_ldlq_pack_decode_grouped_query_matches_the_fake_quant_model():
    import run_reference_driver as R
    from quip_amd import decode, quant
    from test_gpu_decode_e2e import _init
    from test_gpu_decode_hf import hf_generate, _gate
    from transformers import LlamaConfig, LlamaForCausalLM
    VOCAB, SEQLEN, NSAMPLES = 512, 64, 8
    for extra in (1, 0):
        cfg = LlamaConfig(hidden_size=2048, intermediate_size=11008, num_hidden_layers=2, num_attention_heads=16, num_key_value_heads=4,
                          vocab_size=VOCAB, max_position_embeddings=SEQLEN, rms_norm_eps=1e-5, attention_dropout=0.0, tie_word_embeddings=False)
        model = LlamaForCausalLM(cfg).half().to(DEV).eval()
        _init(model, 13)
        model.seqlen = SEQLEN
        drv, is_ref = R.load_llama_driver(restatement=True)
        assert not is_ref
        rs = np.random.RandomState(5)
        batches = [(torch.from_numpy(rs.randint(0, VOCAB, size=(1, SEQLEN))).long(), None) for _ in range(NSAMPLES)]
        args = types.SimpleNamespace(nsamples=NSAMPLES, quant="ldlq", wbits=2, qbits=2, qfn="b", npasses=0, unbiased=False, lazy_batch=False,
                                     percdamp=0.01, pre_gptqH=True, pre_rescale=True, pre_proj=True, pre_proj_extra=extra, groupsize=-1)
        np.random.seed(0)
        torch.manual_seed(0)
        with decode.collect_packed() as packed:
            drv(model, batches, torch.device(DEV), args)
        model.to(DEV)
        assert len(packed.layers) == 14
        hf = copy.deepcopy(model)                                        # the dense fake-quant model
        toks, ref = hf_generate(hf, 7, NTOK)
        named = packed.install(model)
        assert named["model.layers.0.self_attn.k_proj"].outfeatures == 4 * 128
        eng = decode.DecodeEngine.from_hf(model, max_len=SEQLEN)
        assert eng.mode == "fused" and eng.dec.kv_heads == 4
        got = torch.stack([eng.forward(t)[0].float().clone() for t in toks])
        rel, decisive, agree = _gate(f"gqa-e2e-extra{extra}", got, ref, toks)
        e2 = decode.DecodeEngine(eng.dec, max_len=SEQLEN, mode="plain")
        rel2 = _gate(f"gqa-e2e-extra{extra}-plain", torch.stack([e2.forward(t)[0].float().clone() for t in toks]), ref, toks)[0]
        print(f"gqa e2e pre_proj_extra={extra}:", {"rel": rel, "decisive": decisive, "agree": agree, "plain": rel2})
        del model, hf, eng, e2
        torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------- 4. real width
def test_llama2_70b_width_blocks_match_hf():
    """one Llama-2-70B-geometry block (hidden 8192, ffn 28672, 64 heads of 128 over 8 key / value heads), dense fp16 weights, small vocab"""
    from test_gpu_decode_hf import _load
    maxpos = 64
    L = _load("decode_llama")
    torch.manual_seed(0)
    dec = L.Decoder(layers=1, h=8192, ffn=28672, heads=64, kv_heads=8, vocab=512, maxpos=maxpos, eps=1e-5, dtype=torch.float16).to(DEV).eval()
    for p_ in dec.parameters():
        if p_.dim() > 1:
            p_.data.normal_(0, 0.01)
    twin = {(li, n): getattr(b, n).weight.data for li, b in enumerate(dec.blocks) for n in L.Decoder.NAMES}
    hf = hf_llama_gqa(dec, twin, 64, 8, maxpos, 1e-5, torch.float16)
    for bs in (1, 16):
        eng, rel = _engine_vs_hf(dec, hf, bs, "plain", maxpos, seed=70 + bs)
        assert eng.caches[0][0].shape == (bs, 8, maxpos, 128)
        print(f"70B-width block bs={bs}: max rel logits err {rel:.2e}")
