"""-m gpu: the memory contract of the scoring entries (include/quip_amd_score.h, _lib.SCORE_SIGNATURES), with tests/guard_arena.py as it
is -- what tests/test_gpu_prefill_contract.py asserts for the prompt-side entries:

  1. the three outputs and the workspace are carved from a guard arena, once filled 0xFF and once 0x00: no band changes;
  2. no element of logprob / lse / greedy is left holding the fill; x, W and targets keep their bits;
  3. the results are bit-equal to the unguarded call and to each other (nothing depends on what outputs or workspace held before);
  4. the shapes over-cover: rows not a multiple of the 128-row tile (17, 200, 130), vocab not a multiple of the 128-entry tile nor of
     the 256-entry slice (257, 1000, 50272), h of one and of several 64-wide steps, both dtypes;
  5. a refused call writes nothing; every launching name of SCORE_SIGNATURES ran under an arena in this file.

No case tries to make a kernel overrun."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import guard_arena as G  # noqa: E402

F16, BF16 = torch.float16, torch.bfloat16
SCORE_LEDGER = set()                                     # entries of SCORE_SIGNATURES that ran while an arena of this file was installed
EXEMPT = {"quipamd_head_score_workspace_bytes"}          # launches nothing (host arithmetic)


def _inputs(rows, h, vocab, dtype):
    g = torch.Generator().manual_seed(rows + h + vocab)
    x = torch.randn(rows, h, generator=g).to(dtype).to(DEV)
    W = (torch.randn(vocab + 3, h, generator=g) / h ** 0.5).to(dtype).to(DEV)      # a table longer than the vocabulary
    t = torch.randint(-1, vocab + 2, (rows,), generator=g).to(DEV)                 # ignored, in range, past the vocabulary
    return x, W, t


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("rows,h,vocab", [(17, 64, 257), (200, 256, 1000), (130, 128, 50272)])
def test_head_score_writes_its_outputs_and_workspace_only(monkeypatch, dtype, rows, h, vocab):
    from quip_amd import ops
    x, W, t = _inputs(rows, h, vocab, dtype)
    fz = G.freeze(x=x, W=W, targets=t)
    ref = ops.head_score(x, W, t, vocab=vocab)
    torch.cuda.synchronize()
    fz.assert_frozen()
    runs = []
    for uninit in (0xFF, 0x00):
        arena = G.GuardArena(64 << 20, DEV, uninit=uninit)
        with G.installed(monkeypatch, arena, ops, ledger=SCORE_LEDGER):
            out = ops.head_score(x, W, t, vocab=vocab)                              # outputs and workspace: the wrapper's own torch.empty
            torch.cuda.synchronize()
        tag = f"[fill {uninit:#04x}] "
        assert arena.check() == [], tag + repr(arena.check())
        assert len(arena.regions) == 4, tag + "logprob, lse, greedy and the workspace must come from the arena"
        assert any(r["dtype"] == torch.uint8 for r in arena.regions), tag + "the workspace was not carved"
        fz.assert_frozen()
        for name, o, r in zip(("logprob", "lse", "greedy"), out, ref):
            assert uninit != 0xFF or G.count_fill(o) == 0, tag + f"{G.count_fill(o)} elements of {name} still hold the fill"
            assert G.bit_equal(o, r), tag + f"{name} differs from the unguarded call"
        runs.append(out)
    assert all(G.bit_equal(a, b) for a, b in zip(*runs)), "the result depends on what outputs or workspace held before the call"
    assert bool(((ref[2] >= 0) & (ref[2] < vocab)).all()) and bool(torch.isfinite(ref[1]).all())
    assert bool((ref[0][t < 0] == 0).all()) and bool((ref[0][t >= vocab] == float("-inf")).all())


def test_a_refused_call_writes_nothing(monkeypatch):
    from quip_amd import ops, _lib
    rows, h, vocab = 17, 64, 257
    x, W, t = _inputs(rows, h, vocab, F16)
    arena = G.GuardArena(8 << 20, DEV)
    out = (arena.take(rows, torch.float32, name="logprob"), arena.take(rows, torch.float32, name="lse"), arena.take(rows, torch.int64, name="greedy"))
    ws = arena.take(int(_lib.load().quipamd_head_score_workspace_bytes(rows, vocab)), torch.uint8, name="workspace")
    with G.installed(monkeypatch, arena, ops, ledger=SCORE_LEDGER):
        with pytest.raises(_lib.QuipAmdError, match="too small"):
            ops.head_score(x, W, t, vocab=vocab, out=out, workspace=ws[:-16])
        with pytest.raises(_lib.QuipAmdError, match="row strides"):
            ops.head_score(torch.zeros(rows, h + 4, dtype=F16, device=DEV)[:, :h], W, t, vocab=vocab, out=out, workspace=ws)   # ldx = 68
        with pytest.raises(_lib.QuipAmdError, match="multiple of 32"):
            ops.head_score(x[:, :48], W[:, :48], t, vocab=vocab, out=out, workspace=ws)
        torch.cuda.synchronize()
    assert arena.check() == []
    for o in out + (ws,):
        assert G.count_fill(o) == o.numel(), "a refused call wrote to an output or to the workspace"


def test_zz_every_launching_score_entry_point_ran_under_an_arena():
    """reads this file's ledger (every C ABI call goes through quip_amd._lib.call): a new entry of SCORE_SIGNATURES fails here until it
    has a guarded case above"""
    from quip_amd import _lib
    assert EXEMPT <= set(_lib.SCORE_SIGNATURES)
    missing = sorted(set(_lib.SCORE_SIGNATURES) - EXEMPT - SCORE_LEDGER)
    assert not missing, f"entry points without a guarded case: {missing}"
