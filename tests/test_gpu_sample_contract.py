"""-m gpu: the memory contract of the token-sampling entry (include/quip_amd_sample.h, _lib.SAMPLE_SIGNATURES), with tests/guard_arena.py
as it is -- what tests/test_gpu_prefill_contract.py asserts for the prompt-side entries:

  1. out, logprob, kept_n, kept_mass and the `clear` block are carved from a guard arena, once filled 0xFF and once 0x00: no band changes;
  2. no output element is left holding the fill (the 0x00 arena: out / logprob / kept_mass may legitimately be 0, so the fill is counted
     under 0xFF; `clear` must be -1 everywhere under 0x00);
  3. the results are bit-equal to the unguarded call and to each other; logits, params and counter keep their bits;
  4. the shape over-covers: n = 1025 (two full segments of the kernel and one entry), rows = 3, row stride n + 3, an unaligned base, for
     every dtype and for every path of the kernel (greedy, temperature only, top-k, top-p, both);
  5. every launching name of SAMPLE_SIGNATURES ran under an arena in this file (a ledger of its own, not guard_arena.LEDGER).

No case tries to make the kernel overrun."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import guard_arena as G  # noqa: E402

SAMPLE_LEDGER = set()      # entries of SAMPLE_SIGNATURES that ran while an arena of this file was installed
EXEMPT = set()             # entries of the table that launch nothing (none)
N, ROWS, CLEAR_N = 1025, 3, 256
PATHS = [(0.0, 0, 1.0), (0.9, 0, 1.0), (0.9, 40, 1.0), (0.9, 0, 0.9), (0.9, 40, 0.9), (1.0, 1, 1.0)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=str)
@pytest.mark.parametrize("T,k,p", PATHS)
def test_sample_rows_writes_its_outputs_only(monkeypatch, dtype, T, k, p):
    from quip_amd import ops
    ld = N + 3
    flat = (3 * torch.randn(1 + ROWS * ld, generator=torch.Generator().manual_seed(k + int(10 * p)))).to(dtype).to(DEV)
    logits = flat[1:].view(ROWS, ld)[:, :N]                                  # rows on odd element addresses
    params = ops.sample_params(T, top_k=k, top_p=p, seed=77, device=DEV)
    counter = torch.tensor([41], dtype=torch.int64, device=DEV)
    fz = G.freeze(logits=flat, params=params, counter=counter)
    clear0 = torch.arange(ROWS * CLEAR_N, dtype=torch.int32, device=DEV).view(ROWS, CLEAR_N)
    ref_clear = clear0.clone()
    ref = ops.sample_rows(logits, params, counter, clear=ref_clear)
    torch.cuda.synchronize()
    fz.assert_frozen()
    assert bool((ref_clear == -1).all()) and bool((ref[0] >= 0).all()) and bool((ref[0] < N).all())
    runs = []
    for uninit in (0xFF, 0x00):
        arena = G.GuardArena(8 << 20, DEV, uninit=uninit)
        clear = arena.take((ROWS, CLEAR_N), torch.int32, name="clear")
        with G.installed(monkeypatch, arena, ops, ledger=SAMPLE_LEDGER):
            got = ops.sample_rows(logits, params, counter, clear=clear)      # out, logprob, kept_n, kept_mass: carved by the wrapper
            torch.cuda.synchronize()
        tag = f"[fill {uninit:#04x}] "
        assert arena.check() == [], tag + repr(arena.check())
        assert len(arena.regions) == 5, tag + "the four outputs and the clear block must come from the arena"
        for t in got:
            assert any(t.data_ptr() == arena.buf.data_ptr() + r["start"] for r in arena.regions), tag + "an output was not carved"
        fz.assert_frozen()
        if uninit == 0xFF:
            for name, t in zip(("out", "logprob", "kept_n", "kept_mass"), got):
                assert G.count_fill(t) == 0, tag + f"{name}: {G.count_fill(t)} elements still hold the fill"
        assert bool((clear == -1).all()), tag + "a word of the clear block was not set"
        for name, a, b in zip(("out", "logprob", "kept_n", "kept_mass"), got, ref):
            assert G.bit_equal(a, b), tag + f"{name} differs from the unguarded call"
        runs.append(got)
    for a, b in zip(*runs):
        assert G.bit_equal(a, b), "the result depends on what the outputs held before the call"


def test_given_outputs_are_used_and_nothing_else_is_allocated(monkeypatch):
    from quip_amd import ops
    logits = torch.randn(ROWS, N, device=DEV).half()
    params = ops.sample_params(0.8, top_k=20, top_p=0.9, seed=1, device=DEV)
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)
    arena = G.GuardArena(8 << 20, DEV)
    outs = (arena.take(ROWS, torch.int64, name="out"), arena.take(ROWS, torch.float32, name="logprob"), arena.take(ROWS, torch.int32, name="kept_n"),
            arena.take(ROWS, torch.float32, name="kept_mass"))
    with G.installed(monkeypatch, arena, ops, ledger=SAMPLE_LEDGER):
        got = ops.sample_rows(logits, params, counter, *outs)
        torch.cuda.synchronize()
    assert arena.check() == [] and len(arena.regions) == 4
    assert all(a is b for a, b in zip(got, outs)) and all(G.count_fill(t) == 0 for t in outs)


def test_zz_every_launching_sample_entry_point_ran_under_an_arena():
    """reads this file's ledger (every C ABI call goes through quip_amd._lib.call): a new entry of SAMPLE_SIGNATURES fails here until it
    has a guarded case above"""
    from quip_amd import _lib
    assert EXEMPT <= set(_lib.SAMPLE_SIGNATURES)
    missing = sorted(set(_lib.SAMPLE_SIGNATURES) - EXEMPT - SAMPLE_LEDGER)
    assert not missing, f"entry points without a guarded case: {missing}"
