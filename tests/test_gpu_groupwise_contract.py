"""-m gpu: the memory contract of the group-wise dequant-GEMM (include/quip_amd_groupwise.h, _lib.GROUPWISE_SIGNATURES), with
tests/guard_arena.py as it is -- what tests/test_gpu_score_contract.py asserts for the scoring entries:

  1. y is carved from a guard arena, once filled 0xFF and once 0x00: no band changes;
  2. no element of y is left holding the fill; x, the code words, the two tables and the bias keep their bits;
  3. the results are bit-equal to the unguarded call and to each other (nothing depends on what y held before);
  4. the shapes over-cover the tiles: 1 / 17 / 130 rows (one row, one past the 16-row regime border, two past the second 64-row batch
     block), m of one and of five row tiles, d of one and of five STREAM tiles, every width and group size, all three output types;
  5. a refused call writes nothing; every launching name of GROUPWISE_SIGNATURES ran under an arena in this file.

No case tries to make a kernel overrun."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import guard_arena as G  # noqa: E402
import groupwise_ref as R  # noqa: E402

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
GW_LEDGER = set()                                        # entries of GROUPWISE_SIGNATURES that ran while an arena of this file was installed
EXEMPT = set()                                           # (every entry of the table launches)


def _inputs(bs, m, d, bits, gsz, act):
    rng = np.random.default_rng(bs + m + d + bits + gsz)
    from quip_amd import ops
    maxq = 2 ** bits - 1
    codes = torch.from_numpy(rng.integers(0, maxq + 1, (m, d)).astype(np.uint8)).to(DEV)
    qs = ops.pack(codes, bits, ops.LAYOUT_STREAM)
    gs = torch.from_numpy(R.group_major(0.01 * 10.0 ** rng.random((m, d // gsz)))).to(DEV)
    gz = torch.from_numpy(R.group_major(rng.random((m, d // gsz)) * maxq)).to(DEV)
    bias = torch.from_numpy(rng.standard_normal(m).astype(np.float32)).to(DEV)
    x = torch.from_numpy(rng.standard_normal((bs, d)).astype(np.float32)).to(act).to(DEV)
    return x, qs, gs, gz, bias


CASES = [(1, 16, 1, 2, 32, F16, F32), (17, 80, 5, 2, 64, BF16, BF16), (130, 80, 1, 2, 128, F16, F16),
         (1, 80, 5, 3, 64, BF16, F32), (17, 16, 1, 3, 128, F16, F16), (130, 80, 5, 4, 32, BF16, F32),
         (17, 80, 5, 4, 128, F16, BF16), (130, 16, 5, 3, 32, F16, F32)]


@pytest.mark.parametrize("bs,m,tiles,bits,gsz,act,ydt", CASES)
def test_groupwise_writes_y_only(monkeypatch, bs, m, tiles, bits, gsz, act, ydt):
    from quip_amd import ops
    d = tiles * ops.stream_chunk(bits)
    x, qs, gs, gz, bias = _inputs(bs, m, d, bits, gsz, act)
    fz = G.freeze(x=x, qweight=qs, gscale=gs, gzero=gz, bias=bias)
    ref = ops.dequant_gemm_groupwise(x, qs, bits, gsz, gs, gz, bias, out_dtype=ydt)
    torch.cuda.synchronize()
    fz.assert_frozen()
    runs = []
    for uninit in (0xFF, 0x00):
        arena = G.GuardArena(8 << 20, DEV, uninit=uninit)
        with G.installed(monkeypatch, arena, ops, ledger=GW_LEDGER):
            y = ops.dequant_gemm_groupwise(x, qs, bits, gsz, gs, gz, bias, out_dtype=ydt)      # y: the wrapper's own torch.empty
            torch.cuda.synchronize()
        tag = f"[fill {uninit:#04x}] "
        assert arena.check() == [], tag + repr(arena.check())
        assert len(arena.regions) == 1 and arena.regions[0]["shape"] == (bs, m), tag + "y must come from the arena (and nothing else: no workspace)"
        fz.assert_frozen()
        assert uninit != 0xFF or G.count_fill(y) == 0, tag + f"{G.count_fill(y)} elements of y still hold the fill"
        assert G.bit_equal(y, ref), tag + "y differs from the unguarded call"
        runs.append(y)
    assert G.bit_equal(*runs), "the result depends on what y held before the call"
    assert bool(torch.isfinite(ref.float()).all())


def test_a_refused_call_writes_nothing(monkeypatch):
    from quip_amd import ops, _lib
    bs, m, d, bits, gsz = 17, 80, 640, 4, 64
    x, qs, gs, gz, bias = _inputs(bs, m, d, bits, gsz, F16)
    arena = G.GuardArena(8 << 20, DEV)
    y = arena.take((bs, m), F32, name="y")
    fz = G.freeze(x=x, qweight=qs, gscale=gs, gzero=gz, bias=bias)
    call = lambda **kw: _lib.call("quipamd_dequant_gemm_groupwise", ops._p(kw.get("x", x)), kw.get("x_dtype", 1), ops._p(qs), kw.get("bits", bits),
                                  kw.get("gsz", gsz), ops._p(gs), ops._p(gz), ops._p(bias), ops._p(y), 0, kw.get("bs", bs), kw.get("m", m),
                                  kw.get("d", d), ops._stream())
    with G.installed(monkeypatch, arena, ops, ledger=GW_LEDGER):
        with pytest.raises(_lib.QuipAmdError, match="groupsize 16"):
            call(gsz=16)
        with pytest.raises(_lib.QuipAmdError, match="bits 5"):
            call(bits=5)
        with pytest.raises(_lib.QuipAmdError, match="multiple of 16"):
            call(m=72)
        with pytest.raises(_lib.QuipAmdError, match="multiple of 128"):
            call(d=576)
        with pytest.raises(_lib.QuipAmdError, match="f16 / bf16 only"):
            call(x_dtype=0)
        with pytest.raises(_lib.QuipAmdError, match="at least one row"):
            call(bs=0)
        with pytest.raises(_lib.QuipAmdError, match="16-byte aligned"):
            call(x=x.view(-1)[4:])
        with pytest.raises(ValueError, match="group-major"):
            ops.dequant_gemm_groupwise(x, qs, bits, gsz, gs.t().contiguous(), gz, bias, out=y)     # the [m, d/G] orientation
        torch.cuda.synchronize()
    assert arena.check() == []
    assert G.count_fill(y) == y.numel(), "a refused call wrote to y"
    fz.assert_frozen()


def test_zz_every_launching_groupwise_entry_point_ran_under_an_arena():
    """reads this file's ledger (every C ABI call goes through quip_amd._lib.call): a new entry of GROUPWISE_SIGNATURES fails here until it
    has a guarded case above"""
    from quip_amd import _lib
    assert EXEMPT <= set(_lib.GROUPWISE_SIGNATURES)
    missing = sorted(set(_lib.GROUPWISE_SIGNATURES) - EXEMPT - GW_LEDGER)
    assert not missing, f"entry points without a guarded case: {missing}"
