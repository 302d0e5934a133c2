"""-m gpu: the memory contract of the generation-control entry (include/quip_amd_generate.h, _lib.GENERATE_SIGNATURES), with
tests/guard_arena.py as it is -- what tests/test_gpu_sample_contract.py asserts for the sample entry:

  1. out, logprob, kept_n, kept_mass, the `clear` block, done, stop_pos and the history are carved from a guard arena, once filled 0xFF and
     once 0x00: no band changes -- with the counter inside the history, on its last column, and at and behind hist_cap;
  2. of the history exactly the two cells hist[r, c - 1] and hist[r, c] change (those that exist); no output element keeps the 0xFF fill;
     `clear` is -1 everywhere, also for rows that were done on entry;
  3. the results are bit-equal to the unguarded call and to each other; logits, params, counter, stop_ids and fed keep their bits;
  4. every combination of the operands that may be NULL (hist, fed, stop_ids, done, stop_pos) runs under an arena and writes only what it
     was given;
  5. every launching name of GENERATE_SIGNATURES ran under an arena in this file (a ledger of its own).

The shape over-covers as the sample contract's does: n = 1025, rows = 3, row stride n + 3, an unaligned base.  No case tries to make the
kernel overrun."""
import itertools
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import generate_ref as GR  # noqa: E402
import guard_arena as G  # noqa: E402

GENERATE_LEDGER = set()    # entries of GENERATE_SIGNATURES that ran while an arena of this file was installed
EXEMPT = set()             # entries of the table that launch nothing (none)
N, ROWS, CLEAR_N, CAP, LDH = 1025, 3, 256, 40, 43
NAMES = ("out", "logprob", "kept_n", "kept_mass")


def _inputs(dtype, seed):
    from quip_amd import ops
    ld = N + 3
    flat = (3 * torch.randn(1 + ROWS * ld, generator=torch.Generator().manual_seed(seed))).to(dtype).to(DEV)
    logits = flat[1:].view(ROWS, ld)[:, :N]                                  # rows on odd element addresses
    params = ops.write_generate_params(ops.generate_params(ROWS, device=DEV), None, [0.9, 0.0, 0.9], [40, 0, 0], [0.9, 1.0, 1.0], [77, 0, 5],
                                       [1.3, 1.2, 1.0])
    hist = torch.randint(-3, N + 3, (ROWS, LDH), generator=torch.Generator().manual_seed(seed + 1)).to(torch.int32).to(DEV)
    fed = torch.tensor([5, 600, 1024], dtype=torch.int64, device=DEV)
    return flat, logits, params, hist, fed


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=str)
@pytest.mark.parametrize("c", [0, 1, 17, CAP - 1, CAP, CAP + 5])
def test_generate_rows_writes_its_outputs_only(monkeypatch, dtype, c):
    from quip_amd import ops
    flat, logits, params, hist0, fed = _inputs(dtype, c)
    counter = torch.tensor([c], dtype=torch.int64, device=DEV)
    plain = ops.generate_rows(logits, params, counter, hist=hist0.clone()[:, :CAP], fed=fed)[0].tolist()
    stop_ids = torch.tensor([plain[0], N + 7], dtype=torch.int32, device=DEV)        # row 0 stops here; row 2 was done on entry
    done0 = torch.tensor([0, 0, 1], dtype=torch.int32, device=DEV)
    pos0 = torch.tensor([-1, -1, 4], dtype=torch.int64, device=DEV)
    clear0 = torch.arange(ROWS * CLEAR_N, dtype=torch.int32, device=DEV).view(ROWS, CLEAR_N)
    fz = G.freeze(logits=flat, params=params, counter=counter, stop_ids=stop_ids, fed=fed)

    def state(take):
        return (take(hist0, "hist"), take(done0, "done"), take(pos0, "stop_pos"), take(clear0, "clear"))
    r_hist, r_done, r_pos, r_clear = state(lambda t, name: t.clone())
    ref = ops.generate_rows(logits, params, counter, hist=r_hist[:, :CAP], fed=fed, stop_ids=stop_ids, pad_id=9, done=r_done, stop_pos=r_pos,
                            clear=r_clear)
    torch.cuda.synchronize()
    fz.assert_frozen()
    want_out, want_done, want_pos = GR.stop_step(plain, [0, 0, 1], [-1, -1, 4], {plain[0], N + 7}, c, 9)
    assert want_out[0] == plain[0] and want_out[2] == 9 and want_done[0] == want_done[2] == 1 and want_pos[0] == c and want_pos[2] == 4
    assert ref[0].tolist() == want_out and r_done.tolist() == want_done and r_pos.tolist() == want_pos
    assert bool((r_clear == -1).all())
    want_hist = hist0.clone()
    if 0 <= c - 1 < CAP:
        want_hist[:, c - 1] = fed.to(torch.int32)
    if c < CAP:
        want_hist[:, c] = ref[0].to(torch.int32)
    assert torch.equal(r_hist, want_hist)                                    # the two cells; the columns CAP .. LDH - 1 are not the kernel's
    runs = []
    for uninit in (0xFF, 0x00):
        arena = G.GuardArena(8 << 20, DEV, uninit=uninit)
        hist, done, pos, clear = state(lambda t, name: arena.copy_of(t, name=name))
        with G.installed(monkeypatch, arena, ops, ledger=GENERATE_LEDGER):
            got = ops.generate_rows(logits, params, counter, hist=hist[:, :CAP], fed=fed, stop_ids=stop_ids, pad_id=9, done=done, stop_pos=pos,
                                    clear=clear)                             # out, logprob, kept_n, kept_mass: carved by the wrapper
            torch.cuda.synchronize()
        tag = f"[fill {uninit:#04x}] "
        assert arena.check() == [], tag + repr(arena.check())
        assert len(arena.regions) == 8, tag + "the four outputs must come from the arena"
        for t in got:
            assert any(t.data_ptr() == arena.buf.data_ptr() + r["start"] for r in arena.regions), tag + "an output was not carved"
        fz.assert_frozen()
        if uninit == 0xFF:
            for name, t in zip(NAMES, got):
                assert G.count_fill(t) == 0, tag + f"{name}: {G.count_fill(t)} elements still hold the fill"
        assert bool((clear == -1).all()), tag + "a word of the clear block was not set"
        for name, a, b in zip(NAMES, got, ref):
            assert G.bit_equal(a, b), tag + f"{name} differs from the unguarded call"
        assert torch.equal(hist, want_hist) and torch.equal(done, r_done) and torch.equal(pos, r_pos), tag
        runs.append(got)
    for a, b in zip(*runs):
        assert G.bit_equal(a, b), "the result depends on what the outputs held before the call"


OPERANDS = ("hist", "fed", "stop_ids", "done", "stop_pos")


@pytest.mark.parametrize("given", [s for k in range(6) for s in itertools.combinations(OPERANDS, k)], ids=lambda s: "+".join(s) or "none")
def test_every_combination_of_the_optional_operands(monkeypatch, given):
    from quip_amd import ops
    c = 6
    flat, logits, params, hist0, fed = _inputs(torch.float16, 3)
    counter = torch.tensor([c], dtype=torch.int64, device=DEV)
    plain = ops.generate_rows(logits, params, counter, hist=hist0.clone()[:, :CAP] if "hist" in given else None, fed=fed if "fed" in given else None)
    stop_ids = torch.tensor([plain[0][1].item()], dtype=torch.int32, device=DEV)     # row 1 draws it
    fz = G.freeze(logits=flat, params=params, counter=counter, stop_ids=stop_ids, fed=fed)
    arena = G.GuardArena(4 << 20, DEV)
    hist = arena.copy_of(hist0, name="hist") if "hist" in given else None
    done = arena.copy_of(torch.tensor([1, 0, 0], dtype=torch.int32, device=DEV), name="done") if "done" in given else None
    pos = arena.copy_of(torch.tensor([2, -1, -1], dtype=torch.int64, device=DEV), name="stop_pos") if "stop_pos" in given else None
    with G.installed(monkeypatch, arena, ops, ledger=GENERATE_LEDGER):
        got = ops.generate_rows(logits, params, counter, hist=None if hist is None else hist[:, :CAP], fed=fed if "fed" in given else None,
                                stop_ids=stop_ids if "stop_ids" in given else None, pad_id=2, done=done, stop_pos=pos)
        torch.cuda.synchronize()
    assert arena.check() == [] and len(arena.regions) == 4 + sum(t is not None for t in (hist, done, pos))
    fz.assert_frozen()
    assert all(G.count_fill(t) == 0 for t in got)
    toks = [int(t) for t in plain[0]]
    want_tok, want_done, want_pos = GR.stop_step(toks, [1, 0, 0] if done is not None else [0, 0, 0], [2, -1, -1],
                                                 {toks[1]} if "stop_ids" in given else set(), c, 2)
    assert got[0].tolist() == want_tok and (want_pos[1] == c) == ("stop_ids" in given)
    if done is not None:
        assert done.tolist() == want_done and (got[2][0].item(), got[1][0].item(), got[3][0].item()) == (0, 0.0, 1.0)
    if pos is not None:
        assert pos.tolist() == want_pos
    if hist is not None:
        want_hist = hist0.clone()
        if "fed" in given:
            want_hist[:, c - 1] = fed.to(torch.int32)
        want_hist[:, c] = got[0].to(torch.int32)
        assert torch.equal(hist, want_hist)
    for name, a, b in zip(NAMES, got, plain):                                # rows 1 and 2 never see what was switched on around them
        assert G.bit_equal(a[1:], b[1:]), name


def test_zz_every_launching_generate_entry_point_ran_under_an_arena():
    """reads this file's ledger (every C ABI call goes through quip_amd._lib.call): a new entry of GENERATE_SIGNATURES fails here until it
    has a guarded case above"""
    from quip_amd import _lib
    assert EXEMPT <= set(_lib.GENERATE_SIGNATURES)
    missing = sorted(set(_lib.GENERATE_SIGNATURES) - EXEMPT - GENERATE_LEDGER)
    assert not missing, f"entry points without a guarded case: {missing}"
