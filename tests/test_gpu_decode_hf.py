"""-m gpu: the decode harnesses against what the reference's benchmark() actually drives -- the Hugging Face model with
past_key_values (opt.py:431-482, llama.py:418-471: `model(input_ids[:, i:i+1], past_key_values=..., use_cache=True)` token by
token).  scripts/decode_opt.py / decode_llama.py are hand-rolled blocks; their other test compares them with their own dense
twins, which cannot catch an architecture mistake shared by both sides.  Here:

  1. an HF OPTForCausalLM / LlamaForCausalLM (random init, fp16, hidden 2048 so that the fused launch paths are the ones that
     run) receives EXACTLY the weights the harness computes with: embeddings, norms, and for every decoder Linear the dense
     equivalent  U^T What V diag(1/s)  (+ bias) of the packed layer;
  2. HF generates 16 tokens greedily with use_cache=True, one token per call, like benchmark();
  3. the harness is fed the same tokens, one hipGraph replay per token (device-resident position, static KV cache): dense
     (fp16 Linears holding the same twin weights), packed (QuantLinear.forward per layer) and the fused decode variants.

Gates: logits within 1e-2 of HF's (relative l2, every token); HF's greedy token is the harness's greedy token wherever HF's
top-1 margin exceeds the logits difference (a random-init model has near-ties no two fp16 implementations agree on), and the
free-running greedy continuations are identical as long as every step had such a margin."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NTOK = 16


def _load(name):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def hf_opt_from_decoder(dec, twin, heads, maxpos, dtype, dev):
    """an HF OPTForCausalLM holding the harness's tensors: tok / pos embeddings, LayerNorms, final norm, and per Linear either
    the twin's dense equivalent (packed harness) or the harness's own weight"""
    from transformers import OPTConfig, OPTForCausalLM
    h, ffn, vocab = dec.h, dec.blocks[0].fc1.out_features if hasattr(dec.blocks[0].fc1, "out_features") else dec.blocks[0].fc1.outfeatures, dec.tok.weight.shape[0]
    cfg = OPTConfig(hidden_size=h, ffn_dim=ffn, num_hidden_layers=len(dec.blocks), num_attention_heads=heads, word_embed_proj_dim=h,
                    vocab_size=vocab, max_position_embeddings=maxpos, dropout=0.0, attention_dropout=0.0, activation_dropout=0.0,
                    layerdrop=0.0, do_layer_norm_before=True)
    hf = OPTForCausalLM(cfg).to(dtype).to(dev).eval()
    d = hf.model.decoder
    with torch.no_grad():
        d.embed_tokens.weight.copy_(dec.tok.weight)
        d.embed_positions.weight.copy_(dec.posemb.weight)                      # OPTLearnedPositionalEmbedding: maxpos + 2 rows, offset 2
        d.final_layer_norm.weight.copy_(dec.lnf.weight)
        d.final_layer_norm.bias.copy_(dec.lnf.bias)
        for li, (blk, lay) in enumerate(zip(dec.blocks, d.layers)):
            lay.self_attn_layer_norm.load_state_dict(blk.ln1.state_dict())
            lay.final_layer_norm.load_state_dict(blk.ln2.state_dict())
            for name, tgt in (("q_proj", lay.self_attn.q_proj), ("k_proj", lay.self_attn.k_proj), ("v_proj", lay.self_attn.v_proj),
                              ("out_proj", lay.self_attn.out_proj), ("fc1", lay.fc1), ("fc2", lay.fc2)):
                W, b = twin[(li, name)]
                tgt.weight.copy_(W)
                tgt.bias.copy_(b)
    assert hf.lm_head.weight.data_ptr() == d.embed_tokens.weight.data_ptr()    # tied, like the harness's F.linear(.., tok.weight)
    return hf


def hf_llama_from_decoder(dec, twin, heads, maxpos, eps, dtype, dev):
    from transformers import LlamaConfig, LlamaForCausalLM
    ffn = next(W.shape[0] for (li, n), W in twin.items() if n == "gate_proj")
    cfg = LlamaConfig(hidden_size=dec.h, intermediate_size=ffn, num_hidden_layers=len(dec.blocks), num_attention_heads=heads,
                      num_key_value_heads=heads, vocab_size=dec.tok.weight.shape[0], max_position_embeddings=maxpos, rms_norm_eps=eps,
                      rope_theta=10000.0, attention_dropout=0.0, tie_word_embeddings=False, attention_bias=False, mlp_bias=False)
    hf = LlamaForCausalLM(cfg).to(dtype).to(dev).eval()
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
def hf_generate(hf, first, ntok):
    """benchmark()'s loop (opt.py:463-480): one token per call with the cache handed back; returns (tokens fed [ntok], logits [ntok, vocab])"""
    ids = torch.tensor([[first]], device=DEV)
    pkv, toks, logits = None, [], []
    for _ in range(ntok):
        out = hf(input_ids=ids, past_key_values=pkv, use_cache=True)
        pkv = out.past_key_values
        lg = out.logits[0, -1].float()
        toks.append(int(ids[0, 0]))
        logits.append(lg.clone())
        ids = lg.argmax().reshape(1, 1)
    return toks, torch.stack(logits)


@torch.no_grad()
def harness_logits(dec, toks, maxlen, dtype, graph=True):
    """feed `toks` one per step through Decoder.step under ONE captured hipGraph replayed per token (eager when graph=False)"""
    heads, hd = dec.heads, dec.h // dec.heads
    caches = [(torch.zeros(1, heads, maxlen, hd, dtype=dtype, device=DEV), torch.zeros(1, heads, maxlen, hd, dtype=dtype, device=DEV))
              for _ in range(dec.layers_n)]
    arange = torch.arange(maxlen, device=DEV)
    ids = torch.zeros(1, dtype=torch.int64, device=DEV)
    pos = torch.zeros(1, dtype=torch.int64, device=DEV)
    vocab = dec.tok.weight.shape[0]
    out = torch.zeros(1, vocab, dtype=torch.float32, device=DEV)

    fh = bool(getattr(dec, 'fused_head', False) and dec.v3)    # csrc/decode_head.hip at both ends of the step (teacher-forced: no argmax partials)
    out16 = torch.zeros(1, vocab, dtype=torch.float16, device=DEV)

    def one():
        if fh:
            dec.step_fused_head(ids, pos, caches, out16, None, None)      # increments pos itself
            out.copy_(out16)
            return
        out.copy_(dec.step(ids, pos, caches, arange))
        pos.add_(1)
    ids.fill_(toks[0])
    one()                                                    # warm-up; the caches are rewritten from position 0 below
    pos.zero_()
    run = one
    if graph:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            one()
            pos.zero_()
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            one()
        pos.zero_()
        run = g.replay
    logits = []
    for t in toks:
        ids.fill_(t)
        run()
        logits.append(out[0].clone())
    if graph:
        torch.cuda.synchronize()
    return torch.stack(logits)


def _gate(name, got, ref, toks, tol=1e-2):
    rel = ((got - ref).norm(dim=1) / ref.norm(dim=1)).max().item()
    assert rel <= tol, (name, rel)
    top2 = ref.topk(2, dim=1).values
    margin = top2[:, 0] - top2[:, 1]
    diff = (got - ref).abs().max(dim=1).values
    decisive = margin > 2 * diff
    assert bool((got.argmax(1)[decisive] == ref.argmax(1)[decisive]).all()), name
    # free-running greedy: toks[i + 1] is HF's argmax at step i; the harness picks the same token at every decisive step
    agree = int((got.argmax(1) == ref.argmax(1)).sum())
    return rel, int(decisive.sum()), agree


def test_opt_decode_harness_matches_hf_with_past_key_values():
    D = _load("decode_opt")
    dtype, maxpos = torch.float16, 64
    torch.manual_seed(0)
    dec = D.Decoder(layers=2, h=2048, ffn=8192, heads=32, vocab=512, maxpos=maxpos, dtype=dtype).to(DEV).eval()
    for p_ in dec.parameters():
        if p_.dim() > 1:
            p_.data.normal_(0, 0.02)
        else:
            p_.data.add_(0.05 * torch.randn_like(p_))       # non-trivial LayerNorm gains / biases, Linear biases
    twin, _ = D.pack_model(dec, 2, DEV)                      # the 12 Linears are packed w2 QuantLinear layers now
    hf = hf_opt_from_decoder(dec, twin, 32, maxpos, dtype, DEV)
    toks, ref = hf_generate(hf, 7, NTOK)
    report = {}
    # packed, layer by layer (QuantLinear.forward, eager torch attention): the plain path
    report["packed"] = _gate("packed", harness_logits(dec, toks, maxpos, dtype), ref, toks)
    for blk in dec.blocks:
        blk.fused, blk.fused_attn = True, True
    report["fused"] = _gate("fused", harness_logits(dec, toks, maxpos, dtype), ref, toks)
    dec.chained = True
    report["chained"] = _gate("chained", harness_logits(dec, toks, maxpos, dtype), ref, toks)
    if D.vgemm_fusable([dec.blocks[0].q_proj, dec.blocks[0].k_proj, dec.blocks[0].v_proj], 1):
        dec.vfused, dec.split_handover = True, True
        report["vfused_split_handover"] = _gate("vfused", harness_logits(dec, toks, maxpos, dtype), ref, toks)
    assert dec.v3_ok(1)
    dec.v3 = True                                            # csrc/decode_fused.hip: 5 launches per block
    report["v3"] = _gate("v3", harness_logits(dec, toks, maxpos, dtype), ref, toks)
    dec.fused_head = True                                    # + embedding and [U^T + residual -> final norm -> lm_head] as one launch each
    report["v3_head"] = _gate("v3_head", harness_logits(dec, toks, maxpos, dtype), ref, toks)
    dec.fused_head = False
    dec.v3 = False
    # and the dense harness (fp16 Linears with the twin weights): the architecture alone, no packed kernels
    dec.chained = dec.vfused = dec.split_handover = dec.tiled = False
    for li, blk in enumerate(dec.blocks):
        blk.fused = blk.fused_attn = False
        for name in ["q_proj", "k_proj", "v_proj", "out_proj", "fc1", "fc2"]:
            W, b = twin[(li, name)]
            lin = nn.Linear(W.shape[1], W.shape[0], bias=True, dtype=dtype, device=DEV)
            lin.weight.data, lin.bias.data = W, b
            setattr(blk, name, lin)
    report["dense"] = _gate("dense", harness_logits(dec, toks, maxpos, dtype), ref, toks)
    print("opt decode vs HF (max rel logits err, decisive steps, greedy agreement of %d):" % NTOK, report)


def test_llama_decode_harness_matches_hf_with_past_key_values():
    L = _load("decode_llama")
    dtype, maxpos, eps = torch.float16, 64, 1e-5
    torch.manual_seed(0)
    dec = L.Decoder(layers=2, h=2048, ffn=11008, heads=16, vocab=512, maxpos=maxpos, eps=eps, dtype=dtype).to(DEV).eval()
    for p_ in dec.parameters():
        if p_.dim() > 1:
            p_.data.normal_(0, 0.02)
        else:
            p_.data.add_(0.05 * torch.randn_like(p_))
    twin, _ = L.pack_model(dec, 2, DEV)
    hf = hf_llama_from_decoder(dec, twin, 16, maxpos, eps, dtype, DEV)
    toks, ref = hf_generate(hf, 7, NTOK)
    report = {}
    report["packed"] = _gate("packed", harness_logits(dec, toks, maxpos, dtype), ref, toks)
    for blk in dec.blocks:
        blk.fused = True
    report["fused"] = _gate("fused", harness_logits(dec, toks, maxpos, dtype), ref, toks)
    assert dec.v3_ok(1)
    dec.v3 = True                                            # fused launches (64 x 32 operators at hidden 2048) + rotary in the attention prologue
    report["v3"] = _gate("v3", harness_logits(dec, toks, maxpos, dtype), ref, toks)
    dec.fused_head = True                                    # + embedding and [U^T + residual -> final norm -> lm_head] as one launch each
    report["v3_head"] = _gate("v3_head", harness_logits(dec, toks, maxpos, dtype), ref, toks)
    dec.fused_head = False
    dec.v3 = False
    for li, blk in enumerate(dec.blocks):
        blk.fused = False
        for name in L.Decoder.NAMES:
            W = twin[(li, name)]
            lin = nn.Linear(W.shape[1], W.shape[0], bias=False, dtype=dtype, device=DEV)
            lin.weight.data = W
            setattr(blk, name, lin)
    report["dense"] = _gate("dense", harness_logits(dec, toks, maxpos, dtype), ref, toks)
    print("llama decode vs HF (max rel logits err, decisive steps, greedy agreement of %d):" % NTOK, report)


@pytest.mark.parametrize("bs", [3, 4, 8, 16])
def test_opt_engine_many_sequences_matches_hf(bs):
    """round 5: 8 and 16 sequences per step stay on the fused launch family -- engine mode v3, every layer group as
    [prologue-only launch, one workgroup per row] + [dequant-GEMM on the decode-order codes] -- and every sequence's logits are HF's
    (past_key_values, one token per call) within 1e-2, greedy tokens equal wherever HF's margin is decisive.
    3 and 4 sequences: the same two-launch groups (quant.two_launch_from: hidden 2048 takes them from 3 rows on) under the fused
    embedding / head launches of mode v3_head."""
    from quip_amd import decode
    D = _load("decode_opt")
    dtype, maxpos = torch.float16, 64
    torch.manual_seed(0)
    dec = D.Decoder(layers=2, h=2048, ffn=8192, heads=32, vocab=512, maxpos=maxpos, dtype=dtype).to(DEV).eval()
    for p_ in dec.parameters():
        if p_.dim() > 1:
            p_.data.normal_(0, 0.02)
        else:
            p_.data.add_(0.05 * torch.randn_like(p_))
    twin, _ = D.pack_model(dec, 2, DEV)
    hf = hf_opt_from_decoder(dec, twin, 32, maxpos, dtype, DEV)
    seqs = [hf_generate(hf, 7 + 31 * s, NTOK) for s in range(bs)]           # (tokens fed, HF logits) per sequence
    eng = decode.DecodeEngine(dec, bs=bs, max_len=maxpos)
    assert eng.mode == ("v3" if bs > 4 else "v3_head"), eng.mode
    got = []
    for i in range(NTOK):
        ids = torch.tensor([seqs[s][0][i] for s in range(bs)], device=DEV)
        got.append(eng.forward(ids).float().clone())
    got = torch.stack(got)                                                   # [NTOK, bs, vocab]
    worst = 0.0
    for s in range(bs):
        rel, decisive, agree = _gate(f"opt-bs{bs}-seq{s}", got[:, s], seqs[s][1], seqs[s][0])
        worst = max(worst, rel)
    # the same engine one sequence at a time (mode v3_head, the single fused launches) sees the same logits up to fp16 hand-over rounding
    e1 = decode.DecodeEngine(dec, bs=1, max_len=maxpos)
    one = torch.stack([e1.forward(t)[0].float().clone() for t in seqs[0][0]])
    assert float((one - got[:, 0]).norm() / one.norm()) <= 5e-3
    print(f"opt engine, {bs} sequences per step vs HF: worst max-rel logits err {worst:.2e}")


@pytest.mark.parametrize("bs", [6, 16])
def test_llama_engine_many_sequences_matches_hf(bs):
    """the Llama block at 6 and 16 sequences per step: mode v3 -- fused-stage pairs for q / k / v, o, gate / up, and the 11008-wide MLP tail
    on csrc/decode_bigp.hip's multi-row launches (bigp_u: row groups of 4; bigp_v_gemm: ONE weight pass for all rows) -- against HF with
    past_key_values, every sequence within 1e-2."""
    from quip_amd import decode
    L = _load("decode_llama")
    dtype, maxpos, eps = torch.float16, 64, 1e-5
    torch.manual_seed(0)
    dec = L.Decoder(layers=2, h=2048, ffn=11008, heads=16, vocab=512, maxpos=maxpos, eps=eps, dtype=dtype).to(DEV).eval()
    for p_ in dec.parameters():
        if p_.dim() > 1:
            p_.data.normal_(0, 0.02)
        else:
            p_.data.add_(0.05 * torch.randn_like(p_))
    twin, _ = L.pack_model(dec, 2, DEV)
    hf = hf_llama_from_decoder(dec, twin, 16, maxpos, eps, dtype, DEV)
    seqs = [hf_generate(hf, 7 + 31 * s, NTOK) for s in range(bs)]
    eng = decode.DecodeEngine(dec, bs=bs, max_len=maxpos)
    assert eng.mode == "v3", eng.mode
    got = []
    for i in range(NTOK):
        ids = torch.tensor([seqs[s][0][i] for s in range(bs)], device=DEV)
        got.append(eng.forward(ids).float().clone())
    got = torch.stack(got)
    worst = max(_gate(f"llama-bs{bs}-seq{s}", got[:, s], seqs[s][1], seqs[s][0])[0] for s in range(bs))
    print(f"llama engine, {bs} sequences per step vs HF: worst max-rel logits err {worst:.2e}")


# ---------------------------------------------------------------------------------- Llama-2-7B width at its context length
_L7 = {}
# Mode `fused` at this width is further from HF than the suite's 1e-2 at the last of 16 steps (measured 1.1e-2, max_len 4096 and 16384
# alike; v3 5.3e-3, QuantLinear.forward per layer 4.0e-3): its K3 launches hand x~ over in bf16, 1.7-1.9e-3 per layer against the dense
# twin where QuantLinear.forward is 4-9e-4, and 14 such layers compound.  A property of that mode's launches, not of the cache length.
FUSED_7B_GATE = 1.5e-2


def _llama7b(maxpos):
    """2 layers of Llama-2-7B's width (hidden 4096: 64 x 64 operators, 32 heads of 128, intermediate 11008) with `maxpos` positions:
    the packed decoder and the HF model holding its dense twins, built once per maxpos"""
    from quip_amd import decode
    if maxpos not in _L7:
        L = _load("decode_llama")
        dtype, eps = torch.float16, 1e-5
        torch.manual_seed(0)
        dec = L.Decoder(layers=2, h=4096, ffn=11008, heads=32, vocab=512, maxpos=maxpos, eps=eps, dtype=dtype).to(DEV).eval()
        for p_ in dec.parameters():
            if p_.dim() > 1:
                p_.data.normal_(0, 0.02)
            else:
                p_.data.add_(0.05 * torch.randn_like(p_))
        twin, _ = L.pack_model(dec, 2, DEV)
        hf = hf_llama_from_decoder(dec, twin, 32, maxpos, eps, dtype, DEV)
        # .to(float16) rounded HF's rotary frequencies to fp16 (up to 4e-4 off): harmless over 64 positions, ~1 rad at position 4080.
        # Give HF the decoder's fp32 frequencies (decode_llama.Decoder's formula, checked against its tables).
        inv = 1.0 / (10000.0 ** (torch.arange(0, 128, 2, dtype=torch.float32) / 128))
        assert torch.equal(decode.rotary_tables(inv, maxpos)[0], dec.cos.cpu())
        rot = hf.model.rotary_emb
        rot.inv_freq = inv.to(DEV)
        rot.original_inv_freq = inv.to(DEV)
        _L7[maxpos] = (dec, hf)
    return _L7[maxpos]


def _engine_logits(eng, seqs):
    """teacher-force every sequence's tokens through the engine: logits [steps, bs, vocab]"""
    got = []
    for i in range(len(seqs[0][0])):
        ids = torch.tensor([s[0][i] for s in seqs], device=DEV)
        got.append(eng.forward(ids).float().clone())
    return torch.stack(got)


def _engine_vs_hf(eng, seqs, name, tol=1e-2):
    """gate each sequence's engine logits against HF's"""
    got = _engine_logits(eng, seqs)
    return max(_gate(f"{name}-seq{s}", got[:, s], seqs[s][1], seqs[s][0], tol)[0] for s in range(len(seqs)))


@pytest.mark.parametrize("bs", [1, 9, 16])
def test_llama_7b_width_engine_at_its_4096_context_matches_hf(bs):
    """max_len 4096 in whatever mode best_mode picks (v3 / v3_head): from 9 sequences on, 288+ (sequence, head) pairs ask the fused attention
    launch for its three-heads form, whose LDS does not fit a 4096-position cache -- it used to refuse the step"""
    from quip_amd import decode
    dec, hf = _llama7b(4096)
    seqs = [hf_generate(hf, 7 + 31 * s, NTOK) for s in range(bs)]
    eng = decode.DecodeEngine(dec, bs=bs, max_len=4096)
    assert eng.mode in ("v3", "v3_head"), eng.mode
    worst = _engine_vs_hf(eng, seqs, f"llama7b-bs{bs}")
    print(f"llama 7b width, {bs} sequences, max_len 4096, mode {eng.mode} vs HF: worst max-rel logits err {worst:.2e} (gate 1e-2)")


def _continue_at(eng, kvs, start):
    """let the engine go on at position `start` over a prefix another implementation computed: kvs[layer] = (K, V) [bs, kv_heads, start, hd]
    (post-rotary, like the engine's caches).  _prepare() -- warm-up and graph capture -- writes cache position 0 and resets the position,
    so it runs first; then the prefix goes into the caches, and the device position and the step count step() checks against max_len
    move to `start`."""
    eng._prepare()
    for (kc, vc), (K, V) in zip(eng.caches, kvs):
        kc[:, :, :start].copy_(K)
        vc[:, :, :start].copy_(V)
    eng.pos.fill_(start)
    eng._steps = start


@torch.no_grad()
def test_llama_7b_width_engine_near_the_end_of_its_context_matches_hf():
    """9 sequences: HF prefills 4080 tokens of each (one call per sequence), its keys and values become the engine's caches, then 16 steps
    up to position 4095 against HF fed past_key_values"""
    from quip_amd import decode
    dec, hf = _llama7b(4096)
    bs, start, maxlen = 9, 4080, 4096
    g = torch.Generator().manual_seed(4080)
    prompts = torch.randint(0, dec.tok.weight.shape[0], (bs, start + 1), generator=g).to(DEV)
    eng = decode.DecodeEngine(dec, bs=bs, max_len=maxlen)
    assert eng.mode in ("v3", "v3_head"), eng.mode
    kvs = [(torch.empty(bs, 32, start, 128, dtype=torch.float16, device=DEV), torch.empty(bs, 32, start, 128, dtype=torch.float16, device=DEV))
           for _ in dec.blocks]
    seqs = []
    for s in range(bs):
        pkv = hf(input_ids=prompts[s:s + 1, :start], use_cache=True).past_key_values
        for li, (K, V) in enumerate(kvs):
            K[s].copy_(pkv.layers[li].keys[0])
            V[s].copy_(pkv.layers[li].values[0])
        ids, toks, logits = prompts[s:s + 1, start:], [], []
        for _ in range(maxlen - start):                                  # hf_generate's loop, from the prefilled cache
            out = hf(input_ids=ids, past_key_values=pkv, use_cache=True)
            pkv = out.past_key_values
            lg = out.logits[0, -1].float()
            toks.append(int(ids[0, 0]))
            logits.append(lg.clone())
            ids = lg.argmax().reshape(1, 1)
        seqs.append((toks, torch.stack(logits)))
        del pkv
    _continue_at(eng, kvs, start)
    worst = _engine_vs_hf(eng, seqs, "llama7b-end")
    assert eng._steps == maxlen
    print(f"llama 7b width, {bs} sequences, positions {start}..{maxlen - 1}, mode {eng.mode} vs HF: worst max-rel logits err {worst:.2e}")


def test_llama_7b_width_engine_past_the_fused_attention_limit_matches_hf():
    """max_len 16384 is more than any form of the fused attention launch holds (13360 positions at 64 x 64): the engine takes mode `fused`
    (it used to take v3 and fail on its first step).  Its logits are those of the same decoder at max_len 4096 bit for bit -- the long
    cache changes nothing -- and HF's within FUSED_7B_GATE."""
    from quip_amd import decode, ops
    dec, hf = _llama7b(16384)
    assert 4096 < ops.decode_attention_fused_max_len(128, 64, 64) < 16384
    toks, ref = hf_generate(hf, 7, NTOK)
    eng = decode.DecodeEngine(dec, bs=1, max_len=16384)
    assert eng.mode == "fused", eng.mode
    got = _engine_logits(eng, [(toks, ref)])
    short = decode.DecodeEngine(dec, bs=1, max_len=4096, mode="fused")
    assert torch.equal(got, _engine_logits(short, [(toks, ref)]))
    rel = _gate("llama7b-16k", got[:, 0], ref, toks, FUSED_7B_GATE)[0]
    print(f"llama 7b width, max_len 16384, mode {eng.mode} vs HF: max-rel logits err {rel:.2e} (gate {FUSED_7B_GATE}); = max_len 4096 bit for bit")
