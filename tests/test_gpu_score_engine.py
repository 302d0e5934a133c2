"""-m gpu: DecodeEngine.score / loglikelihood / perplexity(fused=True) against the same engine's prefill(all_logits=True), on the
models of tests/test_gpu_prefill_engine.py (packed 2-bit OPT, dense Llama, dense grouped-query Llama; vocabulary 512).

The bound.  The reference side is log_softmax(logits.double()) of logits the head ROUNDED to fp16: each carries a relative error of up
to 2^-11, and both the target's logit and the lse inherit it, so the reference's own log-probability is off by up to 2^-10 max|logit|.
A factor 2 covers the different accumulation order of the two GEMMs: |delta logprob| <= 2^-9 max|logit| of the batch.  greedy is compared
wherever the reference's top-2 gap exceeds the same bound; at most 5 % of the positions may fall under it (the share is printed).

  1. score() in one pass and with chunk=64 (the reference prefilled with the same chunk): logprob, greedy, caches, position; `logits`
     and `ids` untouched;
  2. loglikelihood on 7 ragged requests with bs = 2 against the harness arithmetic on each request ALONE (bs = 1, no padding): right
     padding and batch filling do not leak into a request;
  3. perplexity(fused=True) against perplexity(); perplexity() itself against its code as it stood before the flag, exactly;
  4. the memory claim: the peak of a score() of bs * n positions stays below the bs * n * vocab * 2 bytes of the logits it never builds;
  5. the module-level decode.loglikelihood builds and keeps the engine; the refusals write nothing."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from test_gpu_prefill_engine import _model, _prompts, MAXPOS, VOCAB  # noqa: E402

KINDS = ["opt_w2", "llama_dense", "gqa_dense"]


def _engine(kind, bs, max_len=MAXPOS):
    from quip_amd import decode
    dec, _ = _model(kind)
    return decode.DecodeEngine(dec, bs=bs, max_len=max_len, mode="plain" if kind.endswith("dense") else "auto")


def _bound(logits):
    return 2.0 ** -9 * logits.abs().max().item()


def _decisive(lg, bound):
    top2 = lg.topk(2, dim=-1).values
    return (top2[..., 0] - top2[..., 1]) > bound


# ---------------------------------------------------------------------------------------------------------------- 1. score
@pytest.mark.parametrize("chunk", [None, 64])
@pytest.mark.parametrize("kind", KINDS)
def test_score_against_log_softmax_of_the_engines_own_logits(kind, chunk):
    bs, n = 2, 96
    ids = _prompts(bs, n, 71)
    eng = _engine(kind, bs)
    lg = eng.prefill(ids, chunk=chunk, all_logits=True).double()
    caches = [(kc.clone(), vc.clone()) for kc, vc in eng.caches]
    eng.reset()
    eng.forward(ids[:, 0])                                                   # something to find untouched in `logits` and `ids`
    keep_logits, keep_ids = eng.logits.clone(), eng.ids.clone()
    eng.reset()
    logprob, greedy = eng.score(ids, chunk=chunk)
    assert logprob.shape == greedy.shape == (bs, n) and logprob.dtype == torch.float32 and greedy.dtype == torch.int64
    assert eng._steps == n and int(eng.pos) == n
    assert torch.equal(eng.logits, keep_logits) and torch.equal(eng.ids, keep_ids)
    for (kc, vc), (a, b) in zip(eng.caches, caches):                         # the caches are written as by prefill
        assert torch.equal(kc, a) and torch.equal(vc, b)
    bound = _bound(lg)
    want = torch.log_softmax(lg, dim=-1)[:, :-1].gather(2, ids[:, 1:, None])[..., 0]
    err = (logprob[:, :-1].double() - want).abs().max().item()
    assert bool((logprob[:, -1] == 0).all())                                 # the last position has no next token: ignored
    sure = _decisive(lg, bound)
    share = 1.0 - sure.double().mean().item()
    print(f"{kind} chunk {chunk}: max |delta logprob| {err:.3e} (bound {bound:.3e}), {100 * share:.1f} % of the positions under the greedy gap")
    assert err <= bound, (err, bound)
    assert share <= 0.05, share
    assert torch.equal(greedy[sure], lg.argmax(-1)[sure])
    # explicit targets: the same numbers where they agree with the default, 0 where ignored
    eng.reset()
    tg = torch.cat([ids[:, 1:], ids[:, :1]], dim=1)
    tg[:, ::5] = -1
    lp2, gr2 = eng.score(ids, tg, chunk=chunk)
    on = tg[:, :-1] >= 0
    assert torch.equal(lp2[:, :-1][on], logprob[:, :-1][on]) and bool((lp2[tg < 0] == 0).all()) and torch.equal(gr2, greedy)


# ---------------------------------------------------------------------------------------------------------------- 2. loglikelihood
def _requests():
    g = torch.Generator().manual_seed(81)
    lens = [(3, 1), (60, 5), (17, 9), (30, 2), (8, 4), (45, 3), (17, 9)]     # (context, continuation) tokens; 60 + 5 is cut at max_len 48
    return [(torch.randint(1, VOCAB, (c,), generator=g).tolist(), torch.randint(1, VOCAB, (k,), generator=g).tolist()) for c, k in lens]


@pytest.mark.parametrize("kind", KINDS)
def test_loglikelihood_of_ragged_requests_is_each_request_alone(kind):
    max_len = 48
    reqs = _requests()
    assert any(len(c) + len(k) > max_len + 1 for c, k in reqs)
    eng = _engine(kind, 2, max_len)
    got = eng.loglikelihood(reqs)
    assert eng._steps == 0 and int(eng.pos) == 0
    assert len(got) == len(reqs) and all(isinstance(s, float) and isinstance(f, bool) for s, f in got)
    one = _engine(kind, 1, max_len)
    compared = 0
    for i, ((ctx, cont), (s, flag)) in enumerate(zip(reqs, got)):
        inp = torch.tensor((ctx + cont)[-(max_len + 1):][:-1], device=DEV)[None]
        one.reset()
        lg = one.prefill(inp, all_logits=True).double()[0, -len(cont):]       # the continuation's positions
        ct = torch.tensor(cont, device=DEV)
        want = torch.log_softmax(lg, dim=-1).gather(1, ct[:, None]).sum().item()
        bound = _bound(lg)
        print(f"{kind} request {i} ({len(ctx)} + {len(cont)} tokens): sum {s:.5f} alone {want:.5f} (bound {len(cont) * bound:.3e})")
        assert abs(s - want) <= len(cont) * bound, (i, s, want)
        if bool(_decisive(lg, bound).all()):
            compared += 1
            assert flag == bool((lg.argmax(-1) == ct).all()), i
    assert compared >= 4                                                     # (random continuations: the flags are False; see the test below)


def test_loglikelihood_flags_a_greedy_continuation():
    """a continuation made of the model's own arg-max tokens is flagged, one with a changed token is not"""
    kind, max_len = "llama_dense", 64
    eng = _engine(kind, 2, max_len)
    ctx = _prompts(1, 12, 91)[0].tolist()
    one = _engine(kind, 1, max_len)
    toks = one.generate(torch.tensor([ctx], device=DEV), 4)[:, 0].tolist()   # the 4 greedy tokens behind the context
    other = [(t + 1) % VOCAB for t in toks]
    (s1, f1), (s2, f2), (s3, f3) = eng.loglikelihood([(ctx, toks), (ctx, toks[:3] + other[3:]), (ctx, other[:1])])
    assert f1 and not f2 and not f3 and s1 > s2


# ---------------------------------------------------------------------------------------------------------------- 3. perplexity
@pytest.mark.parametrize("kind", ["opt_w2", "llama_dense"])
def test_fused_perplexity_and_the_default_path(kind):
    nsamples, seqlen, bs = 5, 96, 2                                          # the last pass is short of a full batch
    ids = _prompts(nsamples, seqlen, 41)
    eng = _engine(kind, bs)
    plain = eng.perplexity(ids)
    assert eng._steps == 0
    nlls, peak = [], 0.0
    for lo in range(0, nsamples, bs):                                        # perplexity() as it stood before the flag
        batch = ids[lo:lo + bs]
        real = batch.shape[0]
        if real < bs:
            batch = torch.cat([batch, batch[:1].expand(bs - real, seqlen)])
        eng.reset()
        lg = eng.prefill(batch, all_logits=True)
        peak = max(peak, lg.abs().max().item())
        for r in range(real):
            nlls.append(F.cross_entropy(lg[r, :-1].float(), batch[r, 1:]).float() * seqlen)
    eng.reset()
    assert plain == float(torch.exp(torch.stack(nlls).sum() / (nsamples * seqlen)))          # bit for bit
    fused = eng.perplexity(ids, fused=True)
    assert eng._steps == 0 and int(eng.pos) == 0
    bound = 2.0 ** -9 * peak                                                 # on the mean NLL, hence (to first order) relative on its exponential
    print(f"{kind}: perplexity {plain:.5f}, fused {fused:.5f}, relative difference {abs(fused - plain) / plain:.3e} (bound {bound:.3e})")
    assert abs(fused - plain) / plain <= bound


# ---------------------------------------------------------------------------------------------------------------- 4. memory
def test_score_never_builds_the_logits():
    """bs = 2, n = 512 against a head widened to 8192 rows, in passes of 64 positions: the logits would be bs * n * vocab * 2 bytes
    (16 MiB; prefill(all_logits=True) with the same passes allocates them, and is shown to).  The passes are 64 positions because the
    feed-forward activation of a pass, [bs * chunk, 8192] fp16, is itself as large as the logits at chunk = n."""
    dec, _ = _model("opt_w2")
    bs, n, vocab, chunk = 2, 512, 8192, 64
    ids = _prompts(bs, n, 101)
    keep = dec._head_w
    try:
        dec._head_w = (0.02 * torch.randn(vocab, dec.h, generator=torch.Generator().manual_seed(5))).to(torch.float16).to(DEV)
        eng = _engine("opt_w2", bs)
        assert eng.logits.shape == (bs, vocab)
        eng.score(ids, chunk=chunk)                                          # warm-up: graph capture, the engine's workspace, table builds
        eng.reset()
        limit = bs * n * vocab * 2

        def peak_of(call):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            out = call()
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base
            del out
            eng.reset()
            return peak
        fused = peak_of(lambda: eng.score(ids, chunk=chunk))
        chain = peak_of(lambda: eng.prefill(ids, chunk=chunk, all_logits=True))
        print(f"peak above the baseline: score {fused / 2 ** 20:.2f} MiB, prefill(all_logits=True) {chain / 2 ** 20:.2f} MiB, "
              f"the logits {limit / 2 ** 20:.2f} MiB")
        assert fused < limit, (fused, limit)
        assert chain >= limit                                                # the measurement sees the tensor when it is built
    finally:
        dec._head_w = keep


# ---------------------------------------------------------------------------------------------------------------- 5. module level, refusals
def test_module_level_loglikelihood_on_an_hf_model():
    from quip_amd import decode
    _, hf = _model("llama_dense")
    hf.seqlen = 64
    reqs = _requests()[:3]
    try:
        got = decode.loglikelihood(hf, reqs, bs=2)
        eng = hf.__dict__["_quip_decode_engine"]
        assert eng.max_len == 64 and eng.bs == 2
        assert decode.loglikelihood(hf, reqs, bs=2) == got and hf.__dict__["_quip_decode_engine"] is eng        # kept, and repeatable
        assert got == eng.loglikelihood(reqs)
    finally:
        hf.__dict__.pop("_quip_decode_engine", None)
        del hf.seqlen


def test_score_refusals_leave_caches_and_position_untouched():
    eng = _engine("opt_w2", 2, 64)
    eng.prefill(_prompts(2, 10, 61))
    snap = [(kc.clone(), vc.clone()) for kc, vc in eng.caches]

    def untouched():
        return (int(eng.pos) == 10 and eng._steps == 10 and all(torch.equal(kc, a) and torch.equal(vc, b) for (kc, vc), (a, b) in zip(eng.caches, snap)))
    with pytest.raises(RuntimeError, match="DecodeEngine.score: a prompt of 55 positions does not fit the KV cache"):
        eng.score(_prompts(2, 55, 62))
    with pytest.raises(ValueError, match="bs = 2"):
        eng.score(_prompts(3, 4, 63))
    with pytest.raises(ValueError, match="targets must be int64"):
        eng.score(_prompts(2, 4, 63), _prompts(2, 5, 63))
    with pytest.raises(ValueError, match="vocab 513"):
        eng.score(_prompts(2, 4, 63), vocab=VOCAB + 1)
    with pytest.raises(ValueError, match="more than max_len 64"):
        eng.loglikelihood([([1], list(range(1, 66)))])
    assert untouched()
    lp, gr = eng.score(_prompts(2, 4, 64), vocab=100)                        # continues the sequence; a shorter vocabulary
    assert eng._steps == 14 and bool((gr < 100).all())
