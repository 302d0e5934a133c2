"""-m gpu: the group-wise fused dequant-GEMM (include/quip_amd_groupwise.h, csrc/dqgemm_gw.hip) against the fp64 restatement of its
formula (tests/groupwise_ref.py), on the smallest shapes at which it can still go wrong: m of one / three / five row tiles, d of one /
three / five STREAM tiles (plus seventeen: the decode stream's ring wraps there), rows on both sides of the 16-row regime border and of
the 64-row batch block, every group size, width, activation and output type.

Gates: 1e-3 relative l2 for fp32 y (the K2 contract, tests/test_gpu_dqgemm.py TOL_F32), 3e-3 for 16-bit y (tests/test_gpu_stream3.py);
one-hot columns to 1e-6 per element; constant groups against the per-row kernel and homogeneity to 1e-5; row independence bit for bit."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import groupwise_ref as R  # noqa: E402

TOL_F32, TOL_16 = 1e-3, 3e-3
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
MS, TILES, ROWS, GS, BITS = (16, 48, 80), (1, 3, 5), (1, 5, 16, 17, 70, 130), (32, 64, 128), (2, 3, 4)


def _chunk(bits):
    return 256 if bits == 2 else 128


def _grid():
    """a sampled product of the factors: every 199th point of the full grid of 5832, 30 cases in which every value of every factor, every
    (width, group size) pair and every (rows, group size) pair occurs"""
    full = list(itertools.product(BITS, MS, TILES, ROWS, GS, (F16, BF16), (F32, F16, BF16), (True, False)))
    pick = full[::199]
    for i, values in enumerate((BITS, MS, TILES, ROWS, GS, (F16, BF16), (F32, F16, BF16), (True, False))):
        assert {c[i] for c in pick} == set(values), (i, values)
    assert len({(c[0], c[4]) for c in pick}) == 9 and len({(c[3], c[4]) for c in pick}) == 18
    return pick


def _pattern(m, d, maxq):
    r, k = np.meshgrid(np.arange(m), np.arange(d), indexing="ij")
    return ((5 * r + 3 * k + k // 8) % (maxq + 1)).astype(np.uint8)


def _params(rng, m, ng, maxq, fractional):
    """per (row, group): scale log-uniform over a decade, zero an integer in [0, maxq] -- or anywhere in it"""
    scale = (0.01 * 10.0 ** rng.random((m, ng))).astype(np.float32)
    zero = rng.integers(0, maxq + 1, (m, ng)).astype(np.float32)
    if fractional:
        zero = (rng.random((m, ng)) * maxq).astype(np.float32)
    return scale, zero


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(ops, x, codes, bits, G, scale, zero, bias=None, out_dtype=F32):
    qs = ops.pack(_dev(codes), bits, ops.LAYOUT_STREAM)
    gs, gz = _dev(R.group_major(scale)), _dev(R.group_major(zero))
    return ops.dequant_gemm_groupwise(x, qs, bits, G, gs, gz, None if bias is None else _dev(bias), out_dtype=out_dtype)


@pytest.fixture(scope="module")
def ops():
    from quip_amd import ops as o
    return o


# ---- 1. parity -------------------------------------------------------------------------------------------------------------------------------
def _parity(ops, bits, m, d, bs, G, act, ydt, with_bias, seed):
    rng = np.random.default_rng(seed)
    maxq = 2 ** bits - 1
    codes = rng.integers(0, maxq + 1, (m, d)).astype(np.uint8)
    scale, zero = _params(rng, m, d // G, maxq, fractional=bool(seed & 1))
    bias = rng.standard_normal(m).astype(np.float32) if with_bias else None
    x = torch.from_numpy(rng.standard_normal((bs, d)).astype(np.float32)).to(act).to(DEV)
    ref = R.gemm(R.x64(x), codes, scale, zero, G, bias)
    y = _run(ops, x, codes, bits, G, scale, zero, bias, out_dtype=ydt)
    torch.cuda.synchronize()
    assert y.dtype == ydt and tuple(y.shape) == (bs, m)
    got = y.double().cpu().numpy()
    assert np.isfinite(got).all()
    err = R.rel(got, ref)
    print(f"groupwise parity w{bits} g{G} {m}x{d} bs{bs} {act} -> {ydt} bias={with_bias}: rel {err:.3e}")
    assert err <= (TOL_F32 if ydt == F32 else TOL_16)


@pytest.mark.parametrize("i,case", list(enumerate(_grid())), ids=lambda v: str(v) if isinstance(v, int) else "c")
def test_parity_on_a_sampled_product_of_the_shapes(ops, i, case):
    bits, m, tiles, bs, G, act, ydt, with_bias = case
    _parity(ops, bits, m, tiles * _chunk(bits), bs, G, act, ydt, with_bias, seed=100 + i)


@pytest.mark.parametrize("bits,G,bs", [(2, 32, 5), (4, 128, 16), (3, 64, 1), (2, 64, 17), (4, 32, 70)])
def test_parity_where_the_ring_wraps(ops, bits, G, bs):
    """seventeen STREAM tiles: five ring steps of four stages in the decode stream (a ragged last one), seventeen in the batched regime"""
    _parity(ops, bits, 48, 17 * _chunk(bits), bs, G, F16, F32, True, seed=bits * 7 + G + bs)


# ---- 2. one-hot columns ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("bits,G", [(2, 32), (2, 64), (2, 128), (3, 32), (4, 64), (4, 128)])
def test_one_hot_columns_pin_group_step_and_lane(ops, bits, G, act):
    """x = e_k, one k per row of the call: y[b, r] = scale[r, g(k)] * (code[r, k] - zero[r, g(k)]).  Every k of the middle tile, the first
    and last k of the others; parameters that differ in every row and group (zeros on half-integers: OFF + zero and code - zero are exact
    in fp32, so is the kernel's result up to the one rounding of the product)."""
    m, tiles, maxq = 48, 3, 2 ** bits - 1
    kc = _chunk(bits)
    d = tiles * kc
    codes = _pattern(m, d, maxq)
    r, g = np.meshgrid(np.arange(m), np.arange(d // G), indexing="ij")
    scale = (0.5 + 0.03125 * ((7 * r + 11 * g) % 61)).astype(np.float32)
    zero = (((3 * r + 5 * g) % (maxq + 1)) + 0.5).astype(np.float32)
    ks = [0, kc - 1] + list(range(kc, 2 * kc)) + [2 * kc, d - 1]
    x = torch.zeros((len(ks), d), dtype=act)
    x[torch.arange(len(ks)), torch.tensor(ks)] = 1.0
    y = _run(ops, x.to(DEV), codes, bits, G, scale, zero).double().cpu().numpy()            # len(ks) > 16 rows: the batched regime
    y1 = np.concatenate([_run(ops, x[i:i + 16].to(DEV), codes, bits, G, scale, zero).double().cpu().numpy()
                         for i in range(0, len(ks), 16)])                                   # ... and the decode stream, 16 rows a call
    want = np.stack([scale[:, k // G].astype(np.float64) * (codes[:, k].astype(np.float64) - zero[:, k // G]) for k in ks])
    assert np.abs(want).min() > 0
    for name, got in (("batched", y), ("stream", y1)):
        bad = np.argwhere(np.abs(got - want) > 1e-6 * np.abs(want))
        assert bad.size == 0, f"{name}: {len(bad)} wrong entries, first at (k, row) = ({ks[bad[0][0]]}, {bad[0][1]})"


# ---- 3. constant groups == the per-row kernel -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,G,bs,act", [(2, 64, 5, F16), (3, 128, 16, F16), (4, 32, 40, BF16), (2, 128, 130, F16)])
def test_constant_groups_equal_the_per_row_kernel(ops, bits, G, bs, act):
    """(the per-row kernel takes fp16 rows beyond 16 only for d % 256 == 0 -- QuantLinear.act_dtype --, so the 640-column case runs bf16)"""
    m, maxq = 80, 2 ** bits - 1
    d = 5 * _chunk(bits)
    rng = np.random.default_rng(bits + G + bs)
    codes = rng.integers(0, maxq + 1, (m, d)).astype(np.uint8)
    s_row, z_row = _params(rng, m, 1, maxq, fractional=False)
    scale, zero = np.repeat(s_row, d // G, axis=1), np.repeat(z_row, d // G, axis=1)
    x = torch.from_numpy(rng.standard_normal((bs, d)).astype(np.float32)).to(act).to(DEV)
    y = _run(ops, x, codes, bits, G, scale, zero)
    qs = ops.pack(_dev(codes), bits, ops.LAYOUT_STREAM)
    y_row = ops.dequant_gemm(x, qs, bits, 'a', _dev(s_row.reshape(-1)), _dev(z_row.reshape(-1)), None, out_dtype=F32)
    assert float((y.double() - y_row.double()).norm() / y_row.double().norm()) <= 1e-5


# ---- 4. row independence ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,G,act", [(2, 32, F16), (4, 128, BF16), (3, 64, F16)])
def test_a_row_depends_on_its_own_x_only(ops, bits, G, act):
    m, maxq = 48, 2 ** bits - 1
    d = 5 * _chunk(bits)
    rng = np.random.default_rng(31 + bits)
    codes = rng.integers(0, maxq + 1, (m, d)).astype(np.uint8)
    scale, zero = _params(rng, m, d // G, maxq, fractional=True)
    bias = rng.standard_normal(m).astype(np.float32)
    v = torch.from_numpy(rng.standard_normal(d).astype(np.float32)).to(act)

    def call(rows, at, seed):
        x = torch.from_numpy(np.random.default_rng(seed).standard_normal((rows, d)).astype(np.float32)).to(act)
        x[at] = v
        return _run(ops, x.to(DEV), codes, bits, G, scale, zero, bias)[at].clone()
    eq = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
    # rows <= 16: neither the row count, nor the index, nor the other rows' contents matter
    y1 = call(1, 0, 1)
    assert eq(y1, call(5, 3, 2)) and eq(y1, call(16, 15, 3))
    assert eq(y1, call(5, 3, 4)), "the other rows' contents changed row 3"
    assert eq(y1, call(1, 0, 1)), "two runs of the same call differ"
    # rows > 16
    y17 = call(17, 0, 5)
    assert eq(y17, call(130, 129, 6))
    assert eq(y17, call(130, 129, 7)), "the other rows' contents changed row 129"
    assert eq(y17, call(17, 0, 5)), "two runs of the same call differ"
    # (across the regimes the k-split differs: equal to the contract's tolerance, not bit for bit)
    assert float((y1.double() - y17.double()).norm() / y1.double().norm()) <= 1e-5


# ---- 5. linearity -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,G,bs,act", [(2, 64, 16, BF16), (4, 128, 70, F16)])
def test_homogeneity(ops, bits, G, bs, act):
    m, maxq = 80, 2 ** bits - 1
    d = 5 * _chunk(bits)
    rng = np.random.default_rng(77 + bits)
    codes = rng.integers(0, maxq + 1, (m, d)).astype(np.uint8)
    scale, zero = _params(rng, m, d // G, maxq, fractional=True)
    x = torch.from_numpy(rng.standard_normal((bs, d)).astype(np.float32)).to(act)
    y = _run(ops, x.to(DEV), codes, bits, G, scale, zero)
    yh = _run(ops, (x.float() * 0.5).to(act).to(DEV), codes, bits, G, scale, zero)            # halving is exact in both formats
    assert float((yh - 0.5 * y).norm() / y.norm()) <= 1e-5
