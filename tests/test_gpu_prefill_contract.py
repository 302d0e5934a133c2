"""-m gpu: the memory contract of the prompt-side entries (include/quip_amd_prefill.h, _lib.PREFILL_SIGNATURES), with tests/guard_arena.py
as it is -- what tests/test_gpu_memory_contract.py asserts for the entries of include/quip_amd.h:

  1. every output (out, the caches) is carved from a guard arena, once filled 0xFF and once 0x00: no band changes (arena.check());
  2. no element of `out` is left holding the fill; the caches change in rows [start, start + T) only, the inputs keep their bits;
  3. the results are bit-equal to the unguarded call and to each other (nothing depends on what the outputs held before);
  4. the shapes over-cover: T is not a multiple of the 64-row query tile, bs * T is ragged, g = 3, both head dims, with and without
     rotary tables, caches whose unwritten rows hold the fill (NaN) -- and the out-of-range no-op, which writes nothing at all;
  5. every launching name of PREFILL_SIGNATURES ran under an arena in this file (a ledger of its own, not guard_arena.LEDGER).

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
import prefill_ref as R  # noqa: E402

F16, BF16 = torch.float16, torch.bfloat16
PREFILL_LEDGER = set()     # entries of PREFILL_SIGNATURES that ran while an arena of this file was installed
EXEMPT = set()             # entries of the table that launch nothing (none so far)


def _start(s):
    return torch.tensor([s], dtype=torch.int64, device=DEV)


def _rows_mask(maxlen, start, T):
    m = torch.zeros(maxlen, dtype=torch.bool, device=DEV)
    if 0 <= start and start + T <= maxlen:
        m[start:start + T] = True
    return m


def _guarded(monkeypatch, call, caches0, start, T, inputs, noop=False):
    """call(kc, vc) -> out runs ops.prefill_attention on the caches `caches0(arena or None)` makes: once unguarded, then under a 0xFF and
    a 0x00 arena with the points of the module docstring asserted; returns the unguarded (out, kc, vc)"""
    from quip_amd import ops
    fz = G.freeze(**inputs)
    kc, vc = caches0(None)
    ref = (call(kc, vc), kc, vc)
    torch.cuda.synchronize()
    fz.assert_frozen()
    maxlen = kc.shape[2]
    rows = _rows_mask(maxlen, start, T)
    runs = []
    for uninit in (0xFF, 0x00):
        arena = G.GuardArena(256 << 20, DEV, uninit=uninit)
        kc, vc = caches0(arena)
        before = (kc.clone(), vc.clone())
        with G.installed(monkeypatch, arena, ops, ledger=PREFILL_LEDGER):
            out = call(kc, vc)
            torch.cuda.synchronize()
        tag = f"[fill {uninit:#04x}] "
        assert arena.check() == [], tag + repr(arena.check())
        assert len(arena.regions) >= 3, tag + "out and the caches must come from the arena"
        assert any(r["shape"] == tuple(out.shape) and r["dtype"] == out.dtype for r in arena.regions), tag + "out was not carved"
        fz.assert_frozen()
        if noop:
            assert G.count_fill(out, uninit) == out.numel(), tag + "the out-of-range call wrote to out"
        else:
            assert uninit != 0xFF or G.count_fill(out) == 0, tag + f"{G.count_fill(out)} elements of out still hold the fill"
            assert G.bit_equal(out, ref[0]), tag + "out differs from the unguarded call"
        for name, c, c0, cr in (("kcache", kc, before[0], ref[1]), ("vcache", vc, before[1], ref[2])):
            assert G.bit_equal(c[:, :, ~rows], c0[:, :, ~rows]), tag + f"{name}: a row outside [start, start + T) changed"
            assert G.bit_equal(c[:, :, rows], cr[:, :, rows]), tag + f"{name}: the appended rows differ from the unguarded call"
            assert noop or uninit != 0xFF or G.count_fill(c[:, :, rows]) == 0, tag + f"{name}: appended rows still hold the fill"
        runs.append(out)
    assert noop or G.bit_equal(runs[0], runs[1]), "the result depends on what the outputs held before the call"
    return ref


# T not a multiple of 64, bs * T ragged, g = 3 among the groupings, both head dims, with and without tables, unaligned starts
CASES = [(F16, 128, 3, 3, 300, 37, 65, True), (BF16, 64, 3, 2, 200, 0, 130, False), (F16, 64, 1, 5, 128, 64, 1, True), (BF16, 128, 8, 1, 512, 199, 313, True),
         (F16, 128, 16, 2, 256, 1, 77, False), (F16, 64, 4, 3, 64, 0, 64, True)]


@pytest.mark.parametrize("dtype,hd,g,bs,maxlen,start,T,rot", CASES)
def test_prefill_attention_writes_out_and_its_cache_rows_only(monkeypatch, dtype, hd, g, bs, maxlen, start, T, rot):
    from quip_amd import ops
    kv = 2
    heads = kv * g
    gen = torch.Generator().manual_seed(hd + g + T)
    mk = lambda *s: torch.randn(*s, generator=gen).to(dtype).to(DEV)
    q, k, v = mk(bs * T, heads * hd + 8)[:, :heads * hd], mk(bs * T, kv * hd + 16)[:, :kv * hd], mk(bs * T, kv * hd)      # strided q, k
    kc0, vc0 = mk(bs, kv, maxlen, hd), mk(bs, kv, maxlen, hd)
    cos, sin = ((t.to(DEV) for t in R.tables(hd, maxlen)) if rot else (None, None))
    pos = _start(start)

    def caches(A):
        return (kc0.clone(), vc0.clone()) if A is None else (A.copy_of(kc0, name="kcache"), A.copy_of(vc0, name="vcache"))
    out, kc, vc = _guarded(monkeypatch, lambda kc, vc: ops.prefill_attention(q, k, v, kc, vc, pos, T, cos, sin), caches, start, T,
                           dict(q=q, k=k, v=v, kc0=kc0, vc0=vc0, cos=cos, sin=sin, start=pos))
    kc_w, vc_w = R.append_want(k.contiguous(), v, kc0, vc0, start, T, cos, sin)
    assert torch.equal(kc, kc_w) and torch.equal(vc, vc_w)
    qr = R.rope(q.contiguous(), cos, sin, start, T, heads) if rot else q.contiguous()
    assert R.within_gate(out, R.causal_fp64(qr, kc, vc, start, T, g), dtype)[0]


@pytest.mark.parametrize("dtype,hd,g,T,rot", [(F16, 128, 3, 45, True), (BF16, 64, 2, 100, False)])
def test_unwritten_cache_rows_may_hold_anything(monkeypatch, dtype, hd, g, T, rot):
    """start = 0 on caches that were never initialised: under the 0xFF arena every row behind the prompt is NaN, and the kernel reads whole
    64-position tiles -- the result must not see them (bit-equal to the run on finite caches)"""
    from quip_amd import ops
    bs, kv, maxlen = 2, 2, 256
    heads = kv * g
    gen = torch.Generator().manual_seed(T)
    mk = lambda *s: torch.randn(*s, generator=gen).to(dtype).to(DEV)
    q, k, v = mk(bs * T, heads * hd), mk(bs * T, kv * hd), mk(bs * T, kv * hd)
    cos, sin = ((t.to(DEV) for t in R.tables(hd, maxlen)) if rot else (None, None))
    pos = _start(0)

    def caches(A):
        if A is None:
            return mk(bs, kv, maxlen, hd), mk(bs, kv, maxlen, hd)
        return A.take((bs, kv, maxlen, hd), dtype, name="kcache"), A.take((bs, kv, maxlen, hd), dtype, name="vcache")
    out, kc, vc = _guarded(monkeypatch, lambda kc, vc: ops.prefill_attention(q, k, v, kc, vc, pos, T, cos, sin), caches, 0, T,
                           dict(q=q, k=k, v=v, cos=cos, sin=sin, start=pos))
    assert bool(torch.isfinite(out).all())


@pytest.mark.parametrize("start", [-1, 250, 256, 100000])
def test_out_of_range_start_writes_nothing(monkeypatch, start):
    from quip_amd import ops
    dtype, bs, kv, g, hd, maxlen, T = F16, 2, 2, 3, 128, 256, 70
    gen = torch.Generator().manual_seed(9)
    mk = lambda *s: torch.randn(*s, generator=gen).to(dtype).to(DEV)
    q, k, v = mk(bs * T, kv * g * hd), mk(bs * T, kv * hd), mk(bs * T, kv * hd)
    kc0, vc0 = mk(bs, kv, maxlen, hd), mk(bs, kv, maxlen, hd)
    cos, sin = (t.to(DEV) for t in R.tables(hd, maxlen))
    pos = _start(start)

    def caches(A):
        return (kc0.clone(), vc0.clone()) if A is None else (A.copy_of(kc0, name="kcache"), A.copy_of(vc0, name="vcache"))
    _, kc, vc = _guarded(monkeypatch, lambda kc, vc: ops.prefill_attention(q, k, v, kc, vc, pos, T, cos, sin), caches, start, T,
                         dict(q=q, k=k, v=v, kc0=kc0, vc0=vc0, cos=cos, sin=sin, start=pos), noop=True)
    assert torch.equal(kc, kc0) and torch.equal(vc, vc0)


def test_zz_every_launching_prefill_entry_point_ran_under_an_arena():
    """reads this file's ledger (every C ABI call goes through quip_amd._lib.call): a new entry of PREFILL_SIGNATURES fails here until it
    has a guarded case above"""
    from quip_amd import _lib
    assert EXEMPT <= set(_lib.PREFILL_SIGNATURES)
    missing = sorted(set(_lib.PREFILL_SIGNATURES) - EXEMPT - PREFILL_LEDGER)
    assert not missing, f"entry points without a guarded case: {missing}"
