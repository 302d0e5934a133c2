"""-m gpu: DecodeEngine with a decode.Generation in force, on the tiny packed decoders and the (arch, mode, bs) cases of
tests/test_gpu_sample_engine.py (imported, not copied: vocab 512, max_len 64).

  1. Generation(sampling=S) is generate(sampling=S) and Generation() is greedy generate, in every mode;
  2. with a penalty, every step's token is ops.sample_rows on generate_ref.penalise(engine.logits, engine.history[:, :pos], p) -- bit for
     bit -- with the graph and without, after prefill() and after a token-by-token prompt;
  3. stop ids taken from a plain run: every sequence is the plain run up to and including its first stop token, pad_id behind it; lengths,
     finished, stop_pos; n' is the latest stop's step + 1 for poll 0, 1 and 8;
  4. per-sequence Sampling and penalties at bs 4; 5. reset() and re-run; 6. generation= for one call, set_generation(None), switching in
     mid-sequence; 7. new parameters through the same graph.

"The same tokens" between two RUNS is asserted as tests/test_gpu_sample_engine.py does: OPT's launches are deterministic, so there every
token; Llama's v3 down-projection sums through fp32 atomics, so two runs may differ in the last bit of a logit -- greedy runs are still
compared whole (as that file does), drawn ones are held step by step to ops.sample_rows on the run's OWN logits, which is exact."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import generate_ref as GR  # noqa: E402
import test_gpu_sample_engine as SE  # noqa: E402
from test_gpu_sample_engine import CASES, IDS, MAXLEN, NTOK, S1, VOCAB, _engine, _first, _same_tokens_while_same_logits, _sampled_trace  # noqa: E402

BS4 = [c for c in CASES if c[2] == 4]
BS4_IDS = [i for i, c in zip(IDS, CASES) if c[2] == 4]
PAD = 1


@pytest.fixture(scope="module", autouse=True)
def _decoders_of_this_file_alone():
    """test_gpu_sample_engine._decoder keeps what it built, and OPT's Linear biases are drawn from torch's global generator as it stands at
    that moment (the decoder is constructed before it seeds).  That file's own tests are to meet the decoders they would have met had this
    file never run: the ones built here are dropped at the end, and the generators are put back as they were found.  In between they start
    from a seed of this file's, so the models here are the same ones in whatever order the suite runs."""
    cpu, gpu = torch.get_rng_state(), torch.cuda.get_rng_state(DEV)
    SE._BUILT.clear()
    torch.manual_seed(20)
    yield
    SE._BUILT.clear()
    torch.set_rng_state(cpu)
    torch.cuda.set_rng_state(gpu, DEV)


def _held_to_sample_rows(trace, history, rows, what):
    """every record (position, logits, token, logprob) of the trace: row b's token and logprob are row b of ops.sample_rows on the logits
    penalised over history[b, :position] with row b's parameters (rows: Generation.rows(bs)) -- the same bits"""
    from quip_amd import ops
    hist = history.cpu().numpy()
    bs = hist.shape[0]
    sets = sorted(set(rows))
    for pos, lg, ids, lp in trace:
        vals = lg.float().cpu().numpy()
        ctr = torch.tensor([pos], dtype=torch.int64, device=DEV)
        for T, k, p, seed, pen in sets:
            ref = torch.from_numpy(GR.penalise_rows(vals, hist, [pos] * bs, [pen] * bs)).to(DEV)
            out, rlp, _, _ = ops.sample_rows(ref, ops.sample_params(T, top_k=k, top_p=p, seed=seed, device=DEV), ctr)
            for b in range(bs):
                if rows[b] == (T, k, p, seed, pen):
                    assert int(out[b]) == int(ids[b]), (what, pos, b, int(ids[b]), int(out[b]))
                    assert rlp[b].item() == lp[b].item(), (what, pos, b)


def _trace(eng, start):
    tr = _sampled_trace(eng, start)
    return tr, torch.stack([t[2] for t in tr])


# ---------------------------------------------------------------------------------------------------------------- 1. the default Generation
@pytest.mark.parametrize("arch,mode,bs", CASES, ids=IDS)
def test_a_default_generation_is_the_engine_without_one(arch, mode, bs):
    from quip_amd import decode
    s = decode.Sampling(**S1)
    first = _first(bs, 11)
    plain, eng = _engine(arch, mode, bs), _engine(arch, mode, bs)
    want_greedy = plain.generate(first, NTOK)
    plain.reset()
    want_sampled = plain.generate(first, NTOK, sampling=s)
    got = eng.generate(first, NTOK, generation=decode.Generation())
    assert torch.equal(got, want_greedy) and eng.generation is None and eng.lengths.tolist() == [NTOK] * bs
    assert eng._graph is None and eng._graph_sampled is None and len(eng._graphs_generation) == 1
    assert not eng.finished.any() and bool((eng.stop_pos == -1).all())
    eng.reset()
    gen = decode.Generation(sampling=s)
    eng.set_generation(gen)
    tr, toks = _trace(eng, lambda e: e.forward(first))
    _held_to_sample_rows(tr, eng.history, gen.rows(bs), f"{arch}-{mode}-bs{bs}")
    assert arch != "opt" or torch.equal(toks, want_sampled)
    assert torch.equal(eng.history[:, 0], first.to(torch.int32)) and torch.equal(eng.history[:, 1:NTOK + 1].T, toks.to(torch.int32))
    assert bool((eng.history[:, NTOK + 1:] == -1).all()) and len(eng._graphs_generation) == 1


# ---------------------------------------------------------------------------------------------------------------- 2. the penalty, step by step
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("arch,mode,bs", BS4 + [("opt", "v3_head", 1), ("llama", "v3", 1)], ids=BS4_IDS + ["opt-v3_head-bs1", "llama-v3-bs1"])
def test_every_penalised_step_is_sample_rows_on_the_penalised_logits(arch, mode, bs, graph):
    from quip_amd import decode
    gen = decode.Generation(sampling=decode.Sampling(**S1), repetition_penalty=1.3)
    prompt = torch.randint(0, VOCAB, (bs, 9), generator=torch.Generator().manual_seed(3)).to(DEV)
    e1, e2 = _engine(arch, mode, bs, graph=graph), _engine(arch, mode, bs, graph=graph)
    e1.set_generation(gen)
    e2.set_generation(gen)

    def by_token(e):
        for i in range(prompt.shape[1]):
            e.forward(prompt[:, i])
    a, ta = _trace(e1, lambda e: e.prefill(prompt))
    b, tb = _trace(e2, by_token)
    assert [t[0] for t in a] == [t[0] for t in b] == list(range(9, 9 + NTOK))
    assert (len(e1._graphs_generation) == 1) == graph and e1._graph is None and e1._graph_sampled is None
    for e, tr, toks, what in ((e1, a, ta, "prefill"), (e2, b, tb, "token by token")):
        assert torch.equal(e.history[:, :9], prompt.to(torch.int32)), what               # the prompt is history, whichever way it went in
        assert torch.equal(e.history[:, 9:9 + NTOK].T, toks.to(torch.int32)), what
        _held_to_sample_rows(tr, e.history, gen.rows(bs), f"{arch}-{mode}-bs{bs} {what}")
    # the two prompts run other kernels, so their logits differ in last bits: the same tokens for as long as the logits are the same
    _same_tokens_while_same_logits(a, b, False, f"{arch}-{mode}-bs{bs} prefill against token by token")
    off = decode.Generation(sampling=decode.Sampling(**S1))
    e1.reset()
    e1.set_generation(off)
    _, plain = _trace(e1, lambda e: e.prefill(prompt))
    assert not torch.equal(plain, ta), "a penalty of 1.3 over 9 .. 24 tokens changed nothing"


# ---------------------------------------------------------------------------------------------------------------- 3. stops
def _stop_sets(plain):
    """two sets of stop ids from a plain run [n, bs]: one that (usually) leaves sequences running, one that ends every sequence early"""
    bs = plain.shape[1]
    some = {int(plain[3, 0])} | ({int(plain[7, 1])} if bs > 1 else set())
    every = {int(plain[2 + b % 3, b]) for b in range(bs)}
    return some, every


@pytest.mark.parametrize("arch,mode,bs", BS4 + [("opt", "v3_head", 1), ("llama", "fused", 1)], ids=BS4_IDS + ["opt-v3_head-bs1", "llama-fused-bs1"])
def test_stop_ids_end_sequences_and_the_result_is_trimmed(arch, mode, bs):
    from quip_amd import decode
    first = _first(bs, 12)
    plain_eng, eng = _engine(arch, mode, bs), _engine(arch, mode, bs)
    plain = plain_eng.generate(first, NTOK).cpu().numpy()
    some, every = _stop_sets(plain)
    for stops in (some, every):
        want, lengths, first_stop = GR.trim(plain, stops, PAD)
        all_stop = all(f is not None for f in first_stop)
        gen = decode.Generation(stop_ids=sorted(stops), pad_id=PAD)
        for poll in (0, 1, 8):
            eng.reset()
            eng.poll = poll
            got = eng.generate(first, NTOK, generation=gen)
            what = (arch, mode, bs, sorted(stops), poll)
            assert got.dtype == torch.int64 and got.shape == want.shape, (what, got.shape, want.shape)
            assert np.array_equal(got.cpu().numpy(), want), what
            assert eng.lengths.tolist() == lengths, what
            assert eng.finished.tolist() == [int(f is not None) for f in first_stop], what
            assert eng.stop_pos.tolist() == [-1 if f is None else 1 + f for f in first_stop], what   # token i is fed at position 1 + i
            if all_stop and poll == 1:
                assert eng._steps == want.shape[0], what                      # it stopped stepping with the last sequence
            if all_stop and poll == 0:
                assert eng._steps == NTOK, what                               # never polled: all n steps ran, the result is the same
            assert eng.generation is None
        assert len(eng._graphs_generation) == 1
    assert all(f is not None for f in GR.trim(plain, every, PAD)[2]) and GR.trim(plain, every, PAD)[0].shape[0] < NTOK
    # reset() clears the flags, and the run repeats
    eng.reset()
    assert not eng.finished.any() and bool((eng.stop_pos == -1).all()) and bool((eng.history == -1).all())
    eng.poll = 8
    again = eng.generate(first, NTOK, generation=decode.Generation(stop_ids=sorted(every), pad_id=PAD))
    assert np.array_equal(again.cpu().numpy(), GR.trim(plain, every, PAD)[0])


# ---------------------------------------------------------------------------------------------------------------- 4. per-sequence parameters
@pytest.mark.parametrize("arch,mode,bs", BS4, ids=BS4_IDS)
def test_every_sequence_has_its_own_sampling_and_penalty(arch, mode, bs):
    from quip_amd import decode
    S = decode.Sampling
    per = [S(**S1), S(temperature=0.0), S(1.4, top_k=0, top_p=0.9, seed=3), S(0.7, top_k=20, seed=S1["seed"])]
    pens = [1.0, 1.25, 1.0, 1.1]
    gen = decode.Generation(sampling=per, repetition_penalty=pens)
    first = _first(bs, 13)
    eng = _engine(arch, mode, bs)
    eng.set_generation(gen)
    tr, toks = _trace(eng, lambda e: e.forward(first))
    _held_to_sample_rows(tr, eng.history, gen.rows(bs), f"{arch}-{mode} per sequence")
    with pytest.raises(ValueError, match="Generation"):
        eng.set_generation(decode.Generation(sampling=per[:3]))               # three settings for four sequences
    assert eng.generation == gen
    if arch == "opt":                                                         # deterministic launches: row b of the uniform run with setting b
        for b in range(bs):
            eng.reset()
            uni = eng.generate(first, NTOK, generation=decode.Generation(sampling=per[b], repetition_penalty=pens[b]))
            assert torch.equal(uni[:, b], toks[:, b]), b
        assert eng.generation == gen and len(eng._graphs_generation) == 1
        eng.reset()
        assert torch.equal(eng.generate(first, NTOK), toks)                   # reset and re-run under the engine's own setting


# ---------------------------------------------------------------------------------------------------------------- 6. one call, and back
@pytest.mark.parametrize("arch,mode,bs", [("opt", "v3_head", 1), ("opt", "fused", 4), ("opt", "plain", 1), ("llama", "v3_head", 4), ("llama", "v3", 1)])
def test_generation_for_one_call_and_back_to_the_engine_without(arch, mode, bs):
    from quip_amd import decode
    first = _first(bs, 14)
    never, eng = _engine(arch, mode, bs), _engine(arch, mode, bs)
    want = never.generate(first, NTOK)
    assert torch.equal(eng.generate(first, NTOK), want)                       # greedy first: today's graph
    g0 = eng._graph
    assert g0 is not None and eng.history is None and eng._gen_params is None  # nothing of generation control exists before it is asked for
    base = decode.Generation(repetition_penalty=1.2)
    eng.set_generation(base)
    eng.reset()
    pen = eng.generate(first, NTOK)
    gg = eng._graphs_generation[0]
    other = decode.Generation(sampling=decode.Sampling(**S1), stop_ids=[5])
    eng.reset()
    eng.generate(first, NTOK, generation=other)
    assert eng.generation == base and eng._graphs_generation[0] is gg
    eng.reset()
    with pytest.raises(RuntimeError, match="KV cache full"):
        eng.generate(first, MAXLEN + 8, generation=decode.Generation(sampling=decode.Sampling(seed=3)))
    assert eng.generation == base                                             # put back after a raise, too
    with pytest.raises(ValueError, match="exclude"):
        eng.generate(first, 2, sampling=decode.Sampling(), generation=other)
    with pytest.raises(ValueError, match="exclude"):
        eng.generate(first, 2, sampling=decode.Sampling())                    # ... also against the engine's own Generation
    with pytest.raises(TypeError):
        eng.set_generation("greedy")
    eng.reset()
    assert torch.equal(eng.generate(first, NTOK), pen)                        # the engine's setting still holds, and repeats
    eng.set_generation(None)
    eng.reset()
    assert torch.equal(eng.generate(first, NTOK), want) and eng._graph is g0 and eng.generation is None
    # switching in mid-sequence: greedy, greedy, then under a Generation -- position, token, logits and caches survive the capture
    eng2, twin = _engine(arch, mode, bs), _engine(arch, mode, bs)
    l0 = eng2.forward(first).clone()
    eng2.step()
    l1 = eng2.logits.clone()
    eng2.set_generation(decode.Generation(stop_ids=[VOCAB - 1]))
    eng2.step()                                                               # the generation graph is captured here, at position 2
    assert int(eng2.pos) == 3 and eng2._steps == 3 and len(eng2._graphs_generation) == 1

    def close(a, b):
        rel = ((a.float() - b.float()).norm(dim=1) / b.float().norm(dim=1)).max().item()
        return rel <= 2e-3 and (arch != "opt" or torch.equal(a, b))
    t0, t1 = l0.float().argmax(-1), l1.float().argmax(-1)
    assert close(twin.forward(first), l0) and close(twin.forward(t0), l1) and close(twin.forward(t1), eng2.logits)
    assert eng2.history[:, :2].tolist() == [[-1, -1]] * bs                    # fed before the Generation was set: not recorded
    assert torch.equal(eng2.history[:, 2], t1.to(torch.int32)) and torch.equal(eng2.history[:, 3], eng2.ids.to(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- 7. no recapture
@pytest.mark.parametrize("arch,mode,bs", [("opt", "v3_head", 4), ("opt", "fused", 1), ("llama", "v3", 4)])
def test_new_parameters_take_effect_through_the_same_graph(arch, mode, bs):
    from quip_amd import decode
    first = _first(bs, 15)
    eng = _engine(arch, mode, bs)
    g1 = decode.Generation(sampling=decode.Sampling(**S1), repetition_penalty=1.3)
    eng.set_generation(g1)
    eng.forward(first)
    for _ in range(3):
        eng.step()
    graph = eng._graphs_generation[0]
    g2 = decode.Generation(sampling=decode.Sampling(1.2, top_k=0, top_p=0.97, seed=99), repetition_penalty=[1.0 + 0.1 * b for b in range(bs)])
    eng.set_generation(g2)                                                    # between two steps of one sequence
    tr = []
    for _ in range(4):
        eng.step()
        tr.append((int(eng.pos), eng.logits.clone(), eng.ids.clone(), eng.logprob.clone()))
    _held_to_sample_rows(tr, eng.history, g2.rows(bs), "after the change")
    stop = int(tr[-1][2][0])
    eng.set_generation(decode.Generation(stop_ids=[stop]))                    # stop ids live on the device as well
    eng.set_generation(g2)
    assert eng._graphs_generation == {0: graph}
    eng.reset()
    a = eng.generate(first, NTOK)
    eng.reset()
    b = eng.generate(first, NTOK, generation=decode.Generation(sampling=g2.sampling, repetition_penalty=g2.repetition_penalty, stop_ids=[int(a[5, 0])]))
    assert eng._graphs_generation == {0: graph} and b.shape[0] <= NTOK
    if arch == "opt":                                                         # (deterministic launches: run b is run a until the stop)
        assert bool(eng.finished[0]) and int(b[eng.lengths[0] - 1, 0]) == int(a[5, 0]) and 1 <= int(eng.lengths[0]) <= 6
