"""-m gpu: DecodeEngine with a decode.Sampling in force, on the two-block h = 2048 OPT and Llama decoders with packed w2 layers that
tests/test_gpu_prefill_engine.py builds (vocab 512, max_len 64), in every mode the model allows.

  1. step by step: the oracle (tests/sample_ref.py) applied to `engine.logits` of each of 16 sampled steps accepts the token in `engine.ids`
     with counter = the position the token is fed at and row = the sequence; the next step's logits are those of forward(that token) on a
     twin engine that never sampled;
  2. the same seed: graph replay against eager launches, prefill against the token-by-token prompt, reset and repeat; another seed differs;
  3. Sampling(top_k=1) reproduces greedy generate token for token;
  4. the parameters change without a recapture; set_sampling(None) is the greedy engine again; generate(sampling=) restores the setting.

"The same tokens" between two runs is asserted for as long as the two runs' logits are the same bits -- a token is a function of its step's
logits, the seed, the position and the sequence.  OPT's launches are deterministic, so there it is asserted for all 16 tokens.  Llama's v3
down-projection meets its K-slices through fp32 atomics and the prompt pass is other kernels than the step: runs differ in the last fp16
bit of a few logits, and from the first such step on each run is held to the oracle on its own logits instead."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import sample_ref as R  # noqa: E402
from test_gpu_decode_hf import _load  # noqa: E402

NTOK, VOCAB, MAXLEN, MAXPOS, DT = 16, 512, 64, 768, torch.float16
_BUILT = {}


def _decoder(arch):
    """the packed w2 decoder of tests/test_gpu_prefill_engine.py (_model('opt_w2') / _model('llama_w2')) without its Hugging Face twin"""
    if arch not in _BUILT:
        if arch == "opt":
            D = _load("decode_opt")
            dec = D.Decoder(layers=2, h=2048, ffn=8192, heads=32, vocab=VOCAB, maxpos=MAXPOS, dtype=DT).to(DEV).eval()
        else:
            D = _load("decode_llama")
            dec = D.Decoder(layers=2, h=2048, ffn=11008, heads=16, kv_heads=None, vocab=VOCAB, maxpos=MAXPOS, eps=1e-5, dtype=DT).to(DEV).eval()
        torch.manual_seed(0)
        for p_ in dec.parameters():
            if p_.dim() > 1:
                p_.data.normal_(0, 0.02)
            else:
                p_.data.add_(0.05 * torch.randn_like(p_))
        D.pack_model(dec, 2, DEV)
        _BUILT[arch] = dec
    return _BUILT[arch]


CASES = [(a, m, bs) for a in ("opt", "llama") for m in ("v3_head", "v3", "fused", "plain") for bs in (1, 4)] + [("opt", "v3", 8), ("llama", "v3", 8)]
IDS = [f"{a}-{m}-bs{bs}" for a, m, bs in CASES]
S1 = dict(temperature=0.9, top_k=40, top_p=0.95, seed=0xABCDEF0123456789)


def _engine(arch, mode, bs, graph=True):
    from quip_amd import decode
    eng = decode.DecodeEngine(_decoder(arch), bs=bs, max_len=MAXLEN, mode=mode, graph=graph)
    assert eng.mode == mode
    return eng


def _first(bs, seed=1):
    return torch.randint(0, VOCAB, (bs,), generator=torch.Generator().manual_seed(seed)).to(DEV)


def _record(eng):
    return int(eng.pos), eng.logits.clone(), eng.ids.clone(), eng.logprob.clone()


def _sampled_trace(eng, start, ntok=NTOK):
    """start(eng) feeds the beginning (forward / prefill); then ntok - 1 steps.  One record per sampled token: (the position it is fed at,
    the logits it was drawn from, the token, its logprob)"""
    start(eng)
    trace = [_record(eng)]
    for _ in range(ntok - 1):
        eng.step()
        trace.append(_record(eng))
    return trace


def _held_to_the_oracle(trace, s, what):
    for pos, lg, ids, lp in trace:
        vals, ids, lp = R.values(lg), ids.cpu().numpy(), lp.cpu().numpy()
        for b in range(vals.shape[0]):
            o = R.Oracle(vals[b], s.temperature, s.top_k, s.top_p)
            u = R.uniform(s.seed, pos, b)
            assert o.accepts(u, ids[b]), (what, pos, b, int(ids[b]), int(o.draw(u)))
            assert abs(lp[b] - o.logprob(ids[b])) <= 1e-3, (what, pos, b)


def _same_tokens_while_same_logits(a, b, all_of_them, what):
    n = 0
    for (pa, la, ta, _), (pb, lb, tb, _) in zip(a, b):
        assert pa == pb
        if not torch.equal(la, lb):
            assert not all_of_them, f"{what}: the logits at position {pa} differ between the two runs"
            break
        assert torch.equal(ta, tb), (what, pa, ta.tolist(), tb.tolist())
        n += 1
    print(f"{what}: {n} of {len(a)} steps had the same logits, and then the same tokens")
    return n


# ---------------------------------------------------------------------------------------------------------------- 1. step by step
@pytest.mark.parametrize("arch,mode,bs", CASES, ids=IDS)
def test_every_sampled_step_is_the_oracles_draw_on_that_steps_logits(arch, mode, bs):
    from quip_amd import decode
    s = decode.Sampling(**S1)
    eng, twin = _engine(arch, mode, bs), _engine(arch, mode, bs)
    eng.set_sampling(s)
    first = _first(bs)
    trace = _sampled_trace(eng, lambda e: e.forward(first))
    assert [t[0] for t in trace] == list(range(1, NTOK + 1)) and eng._graph_sampled is not None and eng._graph is None
    _held_to_the_oracle(trace, s, f"{arch}-{mode}-bs{bs}")
    fed, worst, same = first, 0.0, 0
    for pos, lg, ids, _ in trace:                                            # the twin is teacher-forced with the sampled tokens
        want = twin.forward(fed).float()
        rel = ((lg.float() - want).norm(dim=1) / want.norm(dim=1)).max().item()
        worst, same = max(worst, rel), same + int(torch.equal(lg.float(), want))
        assert rel <= 2e-3, (pos, rel)                                       # the same launches: at most the last fp16 bit (Llama's fp32 atomics)
        assert arch != "opt" or torch.equal(lg.float(), want), pos
        fed = ids
    assert len({tuple(t[2].tolist()) for t in trace}) > 1
    print(f"{arch} {mode} bs {bs}: {NTOK} sampled steps accepted; logits vs the teacher-forced greedy twin: {same} of {NTOK} bit-equal, worst rel {worst:.1e}")


# ---------------------------------------------------------------------------------------------------------------- 2. the same seed
@pytest.mark.parametrize("arch,mode,bs", CASES, ids=IDS)
def test_the_same_seed_gives_the_same_tokens(arch, mode, bs):
    from quip_amd import decode
    s = decode.Sampling(**S1)
    first = _first(bs, 2)
    det = arch == "opt"
    name = f"{arch}-{mode}-bs{bs}"
    eng = _engine(arch, mode, bs)
    eng.set_sampling(s)
    a = _sampled_trace(eng, lambda e: e.forward(first))
    eng.reset()
    again = _sampled_trace(eng, lambda e: e.forward(first))
    _same_tokens_while_same_logits(a, again, det, name + " reset and repeat")
    eager = _engine(arch, mode, bs, graph=False)
    eager.set_sampling(s)
    b = _sampled_trace(eager, lambda e: e.forward(first))
    assert eager._graph_sampled is None and eng._graph_sampled is not None
    _same_tokens_while_same_logits(a, b, det, name + " graph against eager")
    _held_to_the_oracle(b, s, name + " eager")
    eng.reset()
    eng.set_sampling(decode.Sampling(**{**S1, "seed": 5}))
    c = _sampled_trace(eng, lambda e: e.forward(first))
    assert any(not torch.equal(x[2], y[2]) for x, y in zip(a, c)), "another seed gave the same 16 tokens"


@pytest.mark.parametrize("arch,mode,bs", [c for c in CASES if c[2] == 4], ids=[i for i, c in zip(IDS, CASES) if c[2] == 4])
def test_prefill_and_the_token_by_token_prompt_draw_alike(arch, mode, bs):
    """the prompt pass runs other kernels than the step, so the two logits differ in their last bits: both runs are held to the oracle with
    the same (seed, position, sequence) -- the position is where the drawn token is fed, whichever way the prompt went in -- and their tokens
    are equal wherever the draw is decisive for both (one acceptable token, the same one)"""
    from quip_amd import decode
    s = decode.Sampling(**S1)
    prompt = torch.randint(0, VOCAB, (bs, 9), generator=torch.Generator().manual_seed(3)).to(DEV)
    e1, e2 = _engine(arch, mode, bs), _engine(arch, mode, bs)
    e1.set_sampling(s)
    e2.set_sampling(s)

    def by_token(e):
        for i in range(prompt.shape[1]):
            e.forward(prompt[:, i])
    a = _sampled_trace(e1, lambda e: e.prefill(prompt))
    b = _sampled_trace(e2, by_token)
    assert [t[0] for t in a] == [t[0] for t in b] == list(range(9, 9 + NTOK))
    _held_to_the_oracle(a, s, "prefill")
    _held_to_the_oracle(b, s, "token by token")
    compared = 0
    for (pos, la, ta, _), (_, lb, tb, _) in zip(a, b):
        va, vb = R.values(la), R.values(lb)
        decisive = True
        for r in range(bs):
            u = R.uniform(s.seed, pos, r)
            oa, ob = R.Oracle(va[r], s.temperature, s.top_k, s.top_p), R.Oracle(vb[r], s.temperature, s.top_k, s.top_p)
            (la_, ha_), (lb_, hb_) = oa.bounds(u), ob.bounds(u)
            decisive = decisive and la_ == ha_ and lb_ == hb_ and oa.draw(u) == ob.draw(u)
        if not decisive:
            break
        assert torch.equal(ta, tb), (pos, ta.tolist(), tb.tolist())
        compared += 1
    assert compared >= 1
    print(f"{arch} {mode}: prefill vs token-by-token prompt, the same tokens on the first {compared} decisive steps of {NTOK}")


# ---------------------------------------------------------------------------------------------------------------- 3. greedy equivalence
@pytest.mark.parametrize("arch,mode,bs", CASES, ids=IDS)
def test_top_k_1_reproduces_greedy_generate_and_nothing_sticks(arch, mode, bs):
    from quip_amd import decode
    first = _first(bs, 4)
    eng, never = _engine(arch, mode, bs), _engine(arch, mode, bs)
    want = never.generate(first, NTOK)
    want_logits = never.logits.clone()
    s = decode.Sampling(**S1)
    eng.set_sampling(s)
    sampled = eng.generate(first, NTOK)                                       # a sampled call first
    g = eng._graph_sampled
    assert g is not None and eng.sampling == s and sampled.shape == (NTOK, bs)
    assert bool((sampled >= 0).all()) and bool((sampled < VOCAB).all())
    eng.reset()
    got = eng.generate(first, NTOK, sampling=decode.Sampling(temperature=0.7, top_k=1, top_p=0.5, seed=9))
    assert torch.equal(got, want), "Sampling(top_k=1) is not greedy"
    assert eng.sampling == s and eng._graph_sampled is g                      # the setting is back, the graph is the one captured before
    assert not eng.logprob.any() and bool((eng.kept_n == 1).all())
    eng.reset()
    assert torch.equal(eng.generate(first, NTOK, sampling=decode.Sampling(temperature=0.0)), want)
    # parameters without recapture: other temperature / k / p / seed take effect through the same graph
    eng.reset()
    again = eng.generate(first, NTOK)
    eng.reset()
    other = eng.generate(first, NTOK, sampling=decode.Sampling(temperature=1.5, top_k=0, top_p=0.99, seed=S1["seed"] + 1))
    assert not torch.equal(other, again) and eng._graph_sampled is g
    assert arch != "opt" or torch.equal(again, sampled)
    # generate(sampling=) restores the setting when the call raises, too
    eng.reset()
    with pytest.raises(RuntimeError, match="KV cache full"):
        eng.generate(first, MAXLEN + 8, sampling=decode.Sampling(seed=3))
    assert eng.sampling == s
    with pytest.raises(TypeError):
        eng.set_sampling("greedy")
    # greedy regression: set_sampling(None) is the engine that never sampled
    eng.set_sampling(None)
    eng.reset()
    back = eng.generate(first, NTOK)
    assert eng.sampling is None and torch.equal(back, want)
    rel = ((eng.logits.float() - want_logits.float()).norm(dim=1) / want_logits.float().norm(dim=1)).max().item()
    assert rel <= 2e-3 and (arch != "opt" or torch.equal(eng.logits, want_logits)), rel
    assert eng._graph is not None and eng._graph_sampled is g


# ---------------------------------------------------------------------------------------------------------------- 4. switching in mid-sequence
@pytest.mark.parametrize("arch,mode,bs", [("opt", "v3_head", 1), ("opt", "fused", 4), ("opt", "plain", 1), ("llama", "v3_head", 4), ("llama", "v3", 1)])
def test_switching_between_greedy_and_sampled_in_mid_sequence_keeps_the_sequence(arch, mode, bs):
    """the graph of the other kind is captured at the engine's current position: position, token, logits and caches survive the capture"""
    from quip_amd import decode
    s = decode.Sampling(**S1)
    first = _first(bs, 6)

    def close(a, b):
        rel = ((a.float() - b.float()).norm(dim=1) / b.float().norm(dim=1)).max().item()
        return rel <= 2e-3 and (arch != "opt" or torch.equal(a, b))
    # sampled, sampled, then greedy
    eng, twin = _engine(arch, mode, bs), _engine(arch, mode, bs)
    eng.set_sampling(s)
    eng.forward(first)
    t1 = eng.ids.clone()
    eng.step()
    t2 = eng.ids.clone()
    eng.set_sampling(None)
    eng.step()                                                                # the greedy graph is captured here, at position 2
    assert int(eng.pos) == 3 and eng._steps == 3 and eng._graph is not None
    twin.forward(first), twin.forward(t1)
    assert close(eng.logits, twin.forward(t2))
    # greedy, greedy, then sampled
    eng, twin = _engine(arch, mode, bs), _engine(arch, mode, bs)
    l0 = eng.forward(first).clone()
    eng.step()
    l1 = eng.logits.clone()
    eng.set_sampling(s)
    eng.step()                                                                # the sampled graph is captured here
    assert int(eng.pos) == 3 and eng._graph_sampled is not None
    _held_to_the_oracle([_record(eng)], s, "greedy then sampled")
    assert close(twin.forward(first), l0) and close(twin.forward(l0.float().argmax(-1)), l1)
    assert close(twin.forward(l1.float().argmax(-1)), eng.logits)
