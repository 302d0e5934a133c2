"""-m gpu: the multi-exponent 2-bit dequantisation in the 4 waves x 4 chunks forms of dq_h_kernel / dq_hg_kernel and in dq_hr_kernel
(csrc/dq_h_body.inc, csrc/dq_common.h DeqME2); the 8 x 1 forms, which keep the uniform offset, run beside them at the same bounds.
Three neighbouring 2-bit fields share one shift and land on mantissa positions under three different exponents (offsets 128 / 32 / 8 in
bf16, 64 / 16 / 4 in fp16), and the one row-sum MFMA of a step yields S_1 = sum_k x and S_off = sum_k OFF_k x; the meet computes
alpha ((a - S_off) - z S_1) + bias.

(a) against the oracle (fp64 of the reference formula on the same 16-bit-rounded x), at the tolerances of tests/test_gpu_k2h_pipeline.py:
    d = 4096 (4 waves x 4 chunks), 2048 (8 x 1), 768 (ragged K: 3 chunks), each with the kernel the plan picks and with the 4 x 4 form
    forced (d = 2048: waves 2, 3 idle; d = 768: one wave with 3 of its 4 chunks); m = 16 (one workgroup) and 48; m = 64 with 2 and 4 row
    tiles per workgroup at d = 4096; bs 1 / 8 / 9 / 16 (8 | 9: half slabs | full slabs); bf16 and fp16; qfn a and b; bias; and
    the fp32 `accumulate` contract;
(b) every field of every dword: row r holds one code c != 0 at column 256 q + r of chunks q = 0, 5, 10, 15 (one chunk of each wave) and
    code 0 elsewhere, r = 0..255: all 4 dwords x 8 fields x both halves of a lane's tile.  A field shifted to the wrong place moves
    y[b, r] by O(|x|) and a wrong OFF_k by O(OFF |x|), against |y[b, r]| ~ sqrt(4096): >= 1e-2 of the row, 10 x the bound;
(c) activations with a non-zero mean (where S_off and S_1 are large against y): the contract's 1e-3 on fp32 y;
(d) the grouped launch against the one-problem calls."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL_F32 = 1e-3
TOL_16 = {torch.bfloat16: 3e-3, torch.float16: 1e-3}
DTS = [torch.bfloat16, torch.float16]
FAM_H = 2
_cache = {}


@pytest.fixture(scope="module")
def ops():
    from quip_amd import ops as o
    return o


@pytest.fixture(scope="module")
def O():
    from oracle import quip_oracle
    return quip_oracle


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _layer(ops, O, m, d, qfn, dt, seed=0):
    """one layer per (m, d, qfn, dt, seed), built once: 16 rows of x (a call with bs rows takes the first bs), packed weights, parameters, and the
    oracle's y for all 16 rows"""
    key = (m, d, qfn, dt, seed)
    if key not in _cache:
        rng = np.random.default_rng(1000 * m + d + (7 if qfn == "a" else 0) + (1 if dt == torch.float16 else 0) + 100003 * seed)
        W = (0.02 * rng.standard_normal((m, d))).astype(np.float32)
        xt = torch.from_numpy(rng.standard_normal((16, d)).astype(np.float32)).to(dt)
        if qfn == "b":
            scale, zero = O.qfnb_scale(W), None
            codes = np.clip(np.round(((W / scale + 1) / 2) * 3), 0, 3).astype(np.uint8)
        else:
            scale, zero = O.find_params_qfna(W, 2)
            codes = np.clip(np.round(W / scale) + zero, 0, 3).astype(np.uint8)
        bias = rng.standard_normal(m).astype(np.float32)
        y_ref = O.dequant_linear(xt.float().numpy(), codes, qfn, scale, zero, 3, bias)
        qs = ops.pack(torch.from_numpy(codes).to(DEV), 2, ops.LAYOUT_STREAM)
        sc = torch.tensor(np.asarray(scale, np.float32).reshape(-1)).to(DEV)
        zr = None if zero is None else torch.from_numpy(zero).to(DEV)
        _cache[key] = (xt.to(DEV), qs, sc, zr, torch.from_numpy(bias).to(DEV), y_ref)
    return _cache[key]


def _call(ops, L, bs, qfn, out_dtype=None, cfg=None, **kw):
    x, qs, sc, zr, bias, _ = L
    if out_dtype is not None:
        kw["out_dtype"] = out_dtype
    return ops.dequant_gemm(x[:bs].contiguous(), qs, 2, qfn, sc, zr, bias, cfg=cfg, **kw)


def _check_against_oracle(ops, L, bs, qfn, dt, m, cfg=None):
    y_ref = L[5][:bs]
    y32 = _call(ops, L, bs, qfn, torch.float32, cfg)
    r32 = _rel(y32.cpu().numpy().astype(np.float64), y_ref)
    y16 = _call(ops, L, bs, qfn, None, cfg)
    r16 = _rel(y16.float().cpu().numpy().astype(np.float64), y_ref)
    print(f"rel err fp32 y {r32:.3e}, 16-bit y {r16:.3e}")
    assert y32.shape == (bs, m) and y16.dtype == dt
    assert r32 <= TOL_F32
    assert r16 <= TOL_16[dt]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("qfn", ["a", "b"])
@pytest.mark.parametrize("m", [16, 48])
@pytest.mark.parametrize("d", [4096, 2048, 768])
@pytest.mark.parametrize("bs", [1, 8, 9, 16])
@pytest.mark.parametrize("cfg", [None, (FAM_H, 4, 4)], ids=["plan", "4x4"])
def test_against_the_oracle(ops, O, dt, qfn, m, d, bs, cfg):
    if cfg is not None:
        name, params, _, _ = ops.dequant_gemm_plan(bs, m, d, 2, dt, qfn, cfg=cfg)
        assert (name, tuple(params[:3])) == ("h", (1, 4, 4))
    _check_against_oracle(ops, _layer(ops, O, m, d, qfn, dt), bs, qfn, dt, m, cfg=cfg)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("qfn", ["a", "b"])
@pytest.mark.parametrize("rt", [2, 4])
@pytest.mark.parametrize("bs", [1, 8, 9, 16])
def test_two_and_four_row_tiles_per_workgroup(ops, O, dt, qfn, rt, bs):
    m, d = 64, 4096
    name, params, _, _ = ops.dequant_gemm_plan(bs, m, d, 2, dt, qfn, cfg=(FAM_H, 0, 0, rt))
    assert tuple(params[:3]) == (rt, 4, 4), (name, params)
    _check_against_oracle(ops, _layer(ops, O, m, d, qfn, dt), bs, qfn, dt, m, cfg=(FAM_H, 0, 0, rt))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("qfn", ["a", "b"])
@pytest.mark.parametrize("d", [4096, 2048, 768])
@pytest.mark.parametrize("bs", [8, 16])
def test_accumulate_into_fp32_y(ops, O, dt, qfn, d, bs):
    """the 4 x 4 form adds its result to what y holds (one workgroup per tile finishes a row: no atomics, one pass)"""
    m = 48
    L = _layer(ops, O, m, d, qfn, dt)
    y0 = torch.from_numpy(np.random.default_rng(bs + d).standard_normal((bs, m)).astype(np.float32))
    y = y0.clone().to(DEV)
    _call(ops, L, bs, qfn, cfg=(FAM_H, 4, 4), out=y, accumulate=True)
    r = _rel(y.cpu().numpy().astype(np.float64), y0.numpy().astype(np.float64) + L[5][:bs])
    print(f"rel err {r:.3e}")
    assert r <= TOL_F32


FIELD_CHUNKS = (0, 5, 10, 15)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("bs", [16, 8])
def test_every_field_of_every_dword(ops, O, dt, bs):
    m, d = 256, 4096
    rng = np.random.default_rng(77 + bs)
    xt = torch.from_numpy(rng.standard_normal((bs, d)).astype(np.float32)).to(dt)
    x = xt.float().numpy()
    r = np.arange(m)
    for c in (3, 1, 2):
        codes = np.zeros((m, d), dtype=np.uint8)
        for q in FIELD_CHUNKS:
            codes[r, 256 * q + r] = c
        qs = ops.pack(torch.from_numpy(codes).to(DEV), 2, ops.LAYOUT_STREAM)
        y = ops.dequant_gemm(xt.to(DEV), qs, 2, "b", torch.tensor([1.0]), None, None, out_dtype=torch.float32).cpu().numpy().astype(np.float64)
        want = O.dequant_linear(x, codes, "b", np.float32(1.0), None, 3, None)
        # y[b, r] = (2 c / 3) sum_q x[b, 256 q + r] - sum_k x[b, k]: the oracle's formula, restated
        restated = (2.0 * c / 3.0) * sum(x[:, 256 * q:256 * q + 256].astype(np.float64) for q in FIELD_CHUNKS) - x.astype(np.float64).sum(1, keepdims=True)
        assert _rel(restated, want) <= 1e-6
        per_row = np.linalg.norm(y - want, axis=0) / np.linalg.norm(want, axis=0)
        per_group = [_rel(y[:, g:g + 16], want[:, g:g + 16]) for g in range(0, m, 16)]
        print(f"code {c}: rel err per row <= {per_row.max():.3e} (row {int(per_row.argmax())}), per 16-row group <= {max(per_group):.3e}")
        assert max(per_group) <= TOL_F32, (c, int(np.argmax(per_group)))
        assert per_row.max() <= TOL_F32, (c, int(per_row.argmax()))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("mean", [1.0, 0.0])
def test_activations_with_a_non_zero_mean(ops, O, dt, mean):
    """x ~ N(mean, 1): S_1 and S_off grow with the mean, y does not (random codes: the dequantised weights have mean zero).  A CPU model of the
    kernel's summation order gave 1.6e-4 (mean 1) and 7e-6 (mean 0) for bf16: the contract's 1e-3 leaves 6 x."""
    m, d, bs = 64, 4096, 16
    rng = np.random.default_rng(5 + int(mean))
    codes = rng.integers(0, 4, size=(m, d)).astype(np.uint8)
    xt = torch.from_numpy((mean + rng.standard_normal((bs, d))).astype(np.float32)).to(dt)
    qs = ops.pack(torch.from_numpy(codes).to(DEV), 2, ops.LAYOUT_STREAM)
    want = O.dequant_linear(xt.float().numpy(), codes, "b", np.float32(1.0), None, 3, None)
    for cfg in (None, (FAM_H, 44, 4)):                                # the default kernel and its register-x twin
        y = ops.dequant_gemm(xt.to(DEV), qs, 2, "b", torch.tensor([1.0]), None, None, out_dtype=torch.float32, cfg=cfg)
        r = _rel(y.cpu().numpy().astype(np.float64), want)
        print(f"x ~ N({mean:g}, 1), cfg {cfg}: rel err {r:.3e}")
        assert r <= TOL_F32


@pytest.mark.parametrize("groups", [2, 3])
@pytest.mark.parametrize("form", [0, 1, 2, 4])
def test_grouped_launch_agrees_with_one_problem_calls(ops, O, groups, form):
    """fp16 problems of m = 64, d = 4096, bs 9 (q / k / v, gate / up of a 9-row decode step): the heuristic's choice (0) and the grouped h kernel
    with 1 / 2 / 4 row tiles per workgroup"""
    m, d, bs, dt = 64, 4096, 9, torch.float16
    Ls = [_layer(ops, O, m, d, "b", dt, seed=g) for g in range(groups)]          # each problem its own x, weights and scale
    xs = [L[0][:bs].contiguous() for L in Ls]
    qws = [L[1] for L in Ls]
    ones = [ops.dequant_gemm(x, L[1], 2, "b", L[2], None, None, out_dtype=torch.float32) for x, L in zip(xs, Ls)]
    outs = [torch.full((bs, m), float("nan"), dtype=torch.float32, device=DEV) for _ in range(groups)]
    ops.dequant_gemm_grouped_config(form)
    try:
        ops.dequant_gemm_grouped(xs, qws, 2, "b", [L[2] for L in Ls], None, outs, m)
        torch.cuda.synchronize()
    finally:
        ops.dequant_gemm_grouped_config(0)
    for g in range(groups):
        got, one = outs[g].cpu().numpy().astype(np.float64), ones[g].cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all(), g
        r = _rel(got, one)
        print(f"problem {g}: rel err against the one-problem call {r:.3e}")
        assert r <= TOL_F32
