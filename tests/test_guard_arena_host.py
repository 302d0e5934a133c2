"""tests/guard_arena.py on CPU tensors: a guard that can never fire must not pass review.  The GPU module that uses it is
tests/test_gpu_memory_contract.py."""
import math
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard_arena as G  # noqa: E402

DTYPES = [torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.uint8, torch.int16, torch.int32, torch.int64]


def _arena(nbytes=4 << 20, **kw):
    return G.GuardArena(nbytes, "cpu", **kw)


def _region(arena, name):
    return next(r for r in arena.regions if r["name"] == name)


def test_a_fresh_arena_is_clean_and_carved_addresses_are_256_byte_aligned():
    a = _arena()
    ts = [a.take((3, 5), dt, name=str(dt)) for dt in DTYPES] + [a.take(7, torch.uint8), a.take((0, 9), torch.float32), a.take((), torch.float64)]
    for t in ts:
        assert t.data_ptr() % 256 == 0                       # absolute, not relative to the arena's own start
        assert t.is_contiguous()
    assert ts[0].shape == (3, 5) and ts[0].dtype == torch.float16 and ts[-3].shape == (7,) and ts[-2].numel() == 0 and ts[-1].dim() == 0
    assert a.check() == []
    lo = min(t.data_ptr() for t in ts if t.numel())          # (an empty view has no address)
    assert lo - a.buf.data_ptr() >= G.MIN_BAND               # a band lies in front of the first tensor too


def test_the_regions_do_not_overlap_and_every_band_is_outside_every_live_range():
    a = _arena()
    for i in range(6):
        a.take((i + 1, 100 * i + 1), torch.float32)
    spans = sorted((r["start"] - r["band"], r["start"], r["end"], r["end"] + r["band"]) for r in a.regions)
    for (b0, s, e, b1), nxt in zip(spans, spans[1:] + [(a.buf.numel(),) * 4]):
        assert 0 <= b0 < s <= e < b1 <= nxt[0]


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_uninitialised_fill_reads_as_nan_255_or_minus_one(dtype):
    t = _arena().take((4, 6), dtype)
    if dtype.is_floating_point:
        assert bool(torch.isnan(t).all())
    elif dtype == torch.uint8:
        assert bool((t == 255).all())
    else:
        assert bool((t == -1).all())
    assert G.count_fill(t) == t.numel()
    t[1, 2] = 0
    assert G.count_fill(t) == t.numel() - 1


def test_fill_requests_are_carved_and_then_filled_and_a_second_uninit_byte_can_be_chosen():
    a = _arena(uninit=0x00)
    assert bool((a.take((2, 3), torch.float32) == 0).all())
    assert bool((a.take((2, 3), torch.float32, fill=1.5) == 1.5).all())
    assert G.count_fill(a.take(5, torch.int64), 0x00) == 5
    assert a.check() == []


def test_a_changed_byte_at_the_first_and_at_the_last_byte_of_a_band_is_reported_with_name_and_distance():
    a = _arena()
    a.take((2, 8), torch.float32, name="left")
    y = a.take((3, 10), torch.float16, name="y")
    a.take(4, torch.int32, name="right")
    r = _region(a, "y")
    assert r["end"] - r["start"] == y.numel() * 2
    band = r["band"]
    for off, side, dist in [(r["end"], "after", 1), (r["end"] + band - 1, "after", band), (r["start"] - 1, "before", 1), (r["start"] - band, "before", band)]:
        old = int(a.buf[off])
        a.buf[off] = old ^ 0x40
        got = a.check()
        assert len(got) == 1, got
        v = got[0]
        assert (v.name, v.side, v.first, v.last, v.nbytes) == ("y", side, dist, dist, 1)
        assert v.shape == (3, 10) and v.dtype == torch.float16
        text = repr(v)
        assert "y" in text and str(dist) in text and ("after the end" if side == "after" else "before the start") in text and "float16" in text
        a.buf[off] = old
        assert a.check() == []


def test_a_two_byte_overrun_and_a_one_byte_underrun_written_through_the_arena_are_both_reported():
    a = _arena()
    y = a.take((5, 7), torch.float32, name="y")
    z = a.take((2, 2), torch.uint8, name="z")
    ry, rz = _region(a, "y"), _region(a, "z")
    a.buf[ry["end"]:ry["end"] + 2] = 0
    a.buf[rz["start"] - 1] = 0
    got = {(v.name, v.side): (v.first, v.last, v.nbytes) for v in a.check()}
    assert got == {("y", "after"): (1, 2, 2), ("z", "before"): (1, 1, 1)}
    assert bool(torch.isnan(y).all()) and bool((z == 255).all())            # the live regions themselves are untouched


def test_a_change_inside_a_live_region_is_not_reported():
    a = _arena()
    y = a.take((5, 7), torch.float32)
    s = a.take((4, 3), torch.int32, stride=(5, 1))                          # a strided carve: its padding columns are live, not band
    y.fill_(3.0)
    s.fill_(7)
    a.buf[a.regions[0]["start"]] = 1
    a.buf[a.regions[0]["end"] - 1] = 1
    a.buf[a.regions[1]["end"] - 1] = 1
    assert a.check() == []
    assert s.stride() == (5, 1) and a.regions[1]["end"] - a.regions[1]["start"] == (3 * 5 + 3) * 4


def test_the_band_width_rule_holds_for_a_5_by_28672_fp32_tensor():
    assert G.band_bytes((5, 28672), torch.float32) >= 16 * 28672 * 4
    assert G.band_bytes((5, 28672), torch.float32) % 256 == 0
    assert G.band_bytes((5, 3), torch.uint8) >= 64 * 1024                   # small tensors: 64 KiB at the least
    assert G.band_bytes((7,), torch.float64) >= max(64 * 1024, 16 * 8)
    a = _arena(8 << 20)
    a.take((5, 28672), torch.float32, name="big")
    r = _region(a, "big")
    assert r["band"] >= 16 * 28672 * 4 and r["start"] - r["band"] >= 0 and r["end"] + r["band"] <= a.buf.numel()


def test_a_full_arena_raises_instead_of_handing_out_unguarded_memory():
    a = _arena(256 << 10)
    a.take(16, torch.float32)
    with pytest.raises(MemoryError):
        a.take((1 << 20,), torch.uint8)


def test_the_proxy_forwards_torch_and_carves_only_the_allocation_calls():
    a = _arena()
    P = G.TorchProxy(a, carve_cpu=True)
    assert P.float16 is torch.float16 and P.cuda is torch.cuda and P.nn is torch.nn and P.linalg.LinAlgError is torch.linalg.LinAlgError
    x = torch.arange(6.0).reshape(2, 3)
    assert isinstance(x, P.Tensor) and P.equal(P.arange(6.0).reshape(2, 3), x)
    inside = lambda t: a.buf.data_ptr() <= t.data_ptr() < a.buf.data_ptr() + a.buf.numel()
    e = P.empty((2, 3), dtype=torch.float32, device="cpu")
    e2 = P.empty(4, 5, dtype=torch.int32, device=torch.device("cpu"))
    z = P.zeros(7, dtype=torch.float64, device="cpu")
    zl = P.zeros_like(x)
    el = P.empty_like(x.t())                                                 # a dense transposed layout is preserved, as torch does
    elc = P.empty_like(x, dtype=torch.uint8)
    f = P.full((2, 2), 5, dtype=torch.int64, device="cpu")
    f2 = P.full((3,), 0.5, device="cpu")
    o = P.ones((2, 2), dtype=torch.float16, device="cpu")
    es = P.empty_strided((3, 4), (6, 1), dtype=torch.float16, device="cpu")
    for t in (e, e2, z, zl, el, elc, f, f2, o, es):
        assert inside(t) and t.data_ptr() % 256 == 0
    assert e.shape == (2, 3) and bool(torch.isnan(e).all()) and e2.shape == (4, 5) and bool((e2 == -1).all())
    assert bool((z == 0).all()) and z.dtype == torch.float64 and bool((zl == 0).all()) and zl.shape == x.shape
    assert el.shape == (3, 2) and el.stride() == torch.empty_like(x.t()).stride() and bool(torch.isnan(el).all())
    assert elc.dtype == torch.uint8 and bool((elc == 255).all())
    assert bool((f == 5).all()) and f2.dtype == torch.get_default_dtype() and bool((f2 == 0.5).all()) and bool((o == 1).all())
    assert es.stride() == (6, 1) and es.shape == (3, 4)
    assert len(a.regions) == 10 and a.check() == []
    assert "test_guard_arena_host.py" in a.regions[0]["name"]                # a region is named after the line that asked for it


def test_requests_for_another_device_pass_through():
    a = _arena()
    P = G.TorchProxy(a)                                                      # as installed for the GPU tests: CPU requests are torch's own
    t = P.zeros(3, dtype=torch.float32, device="cpu")
    u = P.empty(3)
    v = P.empty_like(t)
    assert not a.regions and bool((t == 0).all()) and u.shape == (3,) and v.shape == (3,)


def test_installed_swaps_the_module_global_records_the_calls_and_puts_everything_back(monkeypatch):
    from quip_amd import _lib
    mod = types.ModuleType("fake_ops")
    mod.torch = torch
    a = _arena()
    ledger = set()
    seen = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *args: seen.append((name, args)))
    stub = _lib.call
    with G.installed(monkeypatch, a, mod, ledger=ledger, carve_cpu=True):
        assert isinstance(mod.torch, G.TorchProxy)
        t = mod.torch.empty(5, dtype=torch.float32, device="cpu")
        _lib.call("quipamd_pack", 1, 2)
        with pytest.raises(AssertionError):
            with G.installed(monkeypatch, a, mod, ledger=ledger):            # no arena inside an arena
                pass
    assert mod.torch is torch and _lib.call is stub and real is not stub
    assert ledger == {"quipamd_pack"} and seen == [("quipamd_pack", (1, 2))]
    assert a.buf.data_ptr() <= t.data_ptr() < a.buf.data_ptr() + a.buf.numel()


def test_freeze_compares_bit_for_bit():
    x = torch.tensor([0.0, float("nan"), 1.0, -2.0])
    idx = torch.arange(12, dtype=torch.int32).reshape(3, 4)[:, :3]          # a strided input
    fz = G.freeze(x, idx=idx, none=None)
    fz.assert_frozen()                                                       # NaN == NaN here
    x[0] = -0.0                                                              # == 0.0 as a number, another bit pattern
    assert fz.changed() == ["input#0"]
    x[0] = 0.0
    idx[2, 2] += 1
    assert fz.changed() == ["idx"]
    with pytest.raises(AssertionError, match="idx"):
        fz.assert_frozen()


def test_the_checksum_of_big_tensors_sees_a_flipped_bit_and_a_swap(monkeypatch):
    monkeypatch.setattr(G, "BIG", 1024)                                      # the checksum path on a small tensor
    x = torch.randn(4096, generator=torch.Generator().manual_seed(0))
    fz = G.freeze(big=x)
    assert isinstance(fz.items[0][2], int)
    fz.assert_frozen()
    x[4095] = -x[4095]
    assert fz.changed() == ["big"]
    x[4095] = -x[4095]
    fz.assert_frozen()
    a, b = float(x[10]), float(x[11])
    assert not math.isclose(a, b)
    x[10], x[11] = b, a                                                      # a plain sum would not notice
    assert fz.changed() == ["big"]


def test_bit_equal_tells_dtype_shape_and_sign_of_zero_apart():
    z = torch.zeros(4)
    assert G.bit_equal(z, z.clone()) and not G.bit_equal(z, -z) and not G.bit_equal(z, z.double()) and not G.bit_equal(z, z.reshape(2, 2))
    n = torch.full((3,), float("nan"))
    assert G.bit_equal(n, n.clone())
