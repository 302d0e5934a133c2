"""-m gpu: dq_h_kernel with its arguments as a flat, preloaded list and the weight tiles requested first (csrc/dqgemm_v2.h K2_FLAT_ARGS,
csrc/dq_h_body.inc K2_HEAD / K2_TAIL).  The change moves where arguments come from and the order of requests, never arithmetic, so this is
parity against the fp64 product of the dequantised weights (the oracle's formula on the same 16-bit-rounded x) at the tolerances of
tests/test_gpu_dqgemm_v2.py, on the smallest shapes that reach the headline instantiations: d = 4096 (16 chunks of 256 = 4 waves x 4), m = 16
(one workgroup) and 48 (three), bs 1 / 8 (half slabs) and 9 / 16 (full slabs).

Every preloaded pointer is exercised null and non-null (qfn b: zero and bias null; qfn a with zero and bias; qfn a with bias null), and as a
view at a non-zero storage offset, so both halves of a 64-bit pointer matter.  One 4-bit case reaches h<4, RT 1, 8 x 4>; grouped launches
of 2 and 3 problems reach dq_hg_kernel (same body text, struct arguments); a serial graph of three launches with three weight copies
delivers the arguments through graph nodes and must reproduce the eager launches bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = 4096
TOL_F32 = 1e-3
TOL_16 = {torch.bfloat16: 3e-3, torch.float16: 1e-3}
DTS = [torch.bfloat16, torch.float16]
QUANT = ["b", "a_zero_bias", "a_no_bias"]
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


def _layer(ops, O, m, quant, dt, bits=2):
    """one layer per (m, quantiser, dt, bits), built once and never written: 16 rows of x (a call with bs rows takes the first bs), packed
    weights, parameters, the oracle's y for all 16 rows"""
    key = (m, quant, dt, bits)
    if key not in _cache:
        maxq = (1 << bits) - 1
        rng = np.random.default_rng(77 * m + 13 * QUANT.index(quant) + (1 if dt == torch.float16 else 0) + bits)
        W = (0.02 * rng.standard_normal((m, D))).astype(np.float32)
        xt = torch.from_numpy(rng.standard_normal((16, D)).astype(np.float32)).to(dt)
        if quant == "b":
            qfn, (scale, zero) = "b", (O.qfnb_scale(W), None)
            codes = np.clip(np.round(((W / scale + 1) / 2) * maxq), 0, maxq).astype(np.uint8)
        else:
            qfn = "a"
            scale, zero = O.find_params_qfna(W, bits)
            codes = np.clip(np.round(W / scale) + zero, 0, maxq).astype(np.uint8)
        bias = rng.standard_normal(m).astype(np.float32) if quant == "a_zero_bias" else None
        y_ref = O.dequant_linear(xt.float().numpy(), codes, qfn, scale, zero, maxq, bias)
        qs = ops.pack(torch.from_numpy(codes).to(DEV), bits, ops.LAYOUT_STREAM)
        sc = torch.tensor(np.asarray(scale, np.float32).reshape(-1)).to(DEV)
        zr = None if zero is None else torch.from_numpy(np.asarray(zero, np.float32)).to(DEV)
        bi = None if bias is None else torch.from_numpy(bias).to(DEV)
        _cache[key] = dict(x=xt.to(DEV), qs=qs, sc=sc, zr=zr, bias=bi, y_ref=y_ref, qfn=qfn, bits=bits)
    return _cache[key]


def _run(ops, L, bs, **kw):
    return ops.dequant_gemm(L["x"][:bs].contiguous(), L["qs"], L["bits"], L["qfn"], L["sc"], L["zr"], L["bias"], **kw)


def _headline_plan(ops, bs, m, dt, quant, out_dtype=None, accumulate=False):
    kern, par, _, launches = ops.dequant_gemm_plan(bs, m, D, 2, x_dtype=dt, qfn="b" if quant == "b" else "a", out_dtype=out_dtype,
                                                   accumulate=accumulate)
    assert (kern, par[:3], launches) == ("h", (1, 4, 4), 1), (kern, par, launches)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("quant", QUANT)
@pytest.mark.parametrize("m", [16, 48])
@pytest.mark.parametrize("bs", [1, 8, 9, 16])
def test_parity_with_every_output_type(ops, O, dt, quant, m, bs):
    L = _layer(ops, O, m, quant, dt)
    y_ref = L["y_ref"][:bs]
    _headline_plan(ops, bs, m, dt, quant)
    _headline_plan(ops, bs, m, dt, quant, torch.float32, True)
    y16 = _run(ops, L, bs)
    y32 = _run(ops, L, bs, out_dtype=torch.float32)
    base = torch.from_numpy(np.random.default_rng(bs + m).standard_normal((bs, m)).astype(np.float32)).to(DEV)
    yacc = base.clone()
    _run(ops, L, bs, out=yacc, accumulate=True)
    r16 = _rel(y16.float().cpu().numpy().astype(np.float64), y_ref)
    r32 = _rel(y32.cpu().numpy().astype(np.float64), y_ref)
    racc = _rel(yacc.cpu().numpy().astype(np.float64), y_ref + base.cpu().numpy().astype(np.float64))
    print(f"rel err: 16-bit y {r16:.3e}, fp32 y {r32:.3e}, fp32 accumulate {racc:.3e}")
    assert y16.dtype == dt and y16.shape == (bs, m)
    assert r16 <= TOL_16[dt]
    assert r32 <= TOL_F32
    assert racc <= TOL_F32


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("quant", QUANT)
@pytest.mark.parametrize("bs", [8, 16])
def test_views_at_a_storage_offset(ops, O, dt, quant, bs):
    """x, qw and y inside larger allocations, 16-byte aligned but not at their start: the pointers the kernel gets differ from the
    allocations' in their low halves, and the result must be the one of the plain call, bit for bit"""
    m = 48
    L = _layer(ops, O, m, quant, dt)
    want = _run(ops, L, bs)
    xb = torch.zeros(3 * D + bs * D, dtype=dt, device=DEV)
    xv = xb[3 * D:].view(bs, D)
    xv.copy_(L["x"][:bs])
    qb = torch.zeros(L["qs"].numel() + 260, dtype=L["qs"].dtype, device=DEV)
    qv = qb[260:].view(L["qs"].shape)
    qv.copy_(L["qs"])
    yb = torch.full((5 * m + bs * m,), float("nan"), dtype=dt, device=DEV)
    yv = yb[5 * m:].view(bs, m)
    assert xv.storage_offset() and qv.storage_offset() and yv.storage_offset()
    assert xv.data_ptr() % 16 == 0 and qv.data_ptr() % 16 == 0
    ops.dequant_gemm(xv, qv, 2, L["qfn"], L["sc"], L["zr"], L["bias"], out=yv)
    assert torch.equal(yv, want), int((yv != want).sum())
    assert torch.isnan(yb[:5 * m].float()).all(), "wrote in front of y"
    assert _rel(yv.float().cpu().numpy().astype(np.float64), L["y_ref"][:bs]) <= TOL_16[dt]


def test_four_bit_eight_by_four(ops, O):
    """h<4, RT 1, 8 waves x 4 chunks>: d = 4096 is 32 chunks of 128"""
    m, bs, dt = 16, 16, torch.bfloat16
    kern, par, _, _ = ops.dequant_gemm_plan(bs, m, D, 4, x_dtype=dt)
    assert (kern, par[:3]) == ("h", (1, 8, 4)), (kern, par)
    L = _layer(ops, O, m, "a_zero_bias", dt, bits=4)
    y32 = _run(ops, L, bs, out_dtype=torch.float32)
    y16 = _run(ops, L, bs)
    assert _rel(y32.cpu().numpy().astype(np.float64), L["y_ref"]) <= TOL_F32
    assert _rel(y16.float().cpu().numpy().astype(np.float64), L["y_ref"]) <= TOL_16[dt]


@pytest.mark.parametrize("groups", [2, 3])
@pytest.mark.parametrize("bs", [8, 16])
def test_grouped_launch(ops, O, groups, bs):
    """dq_hg_kernel: the same body text behind struct arguments"""
    m, dt = 32, torch.float16
    kern, _, _, launches = ops.dequant_gemm_plan(bs, m, D, 2, x_dtype=dt, out_dtype=torch.float32, ngroups=groups)
    assert (kern, launches) == ("hg", 1), (kern, launches)
    # distinct problems: every group has its own layer (weights, scale: qfn b on m, m + 16 and m + 32 rows, the first m of each are used
    # -- a 16-row tile is self-contained in the STREAM layout) and its own x (rolled by g rows; the reference rolls with it)
    Ls = [_layer(ops, O, m + 16 * g, "b", dt) for g in range(groups)]
    nwords = Ls[0]["qs"].numel()
    qws = [L["qs"].reshape(-1)[:nwords].contiguous() for L in Ls]
    assert len({q.data_ptr() for q in qws}) == groups and len({L["sc"].data_ptr() for L in Ls}) == groups
    xs = [torch.roll(Ls[g]["x"], g, 0)[:bs].contiguous() for g in range(groups)]
    outs = [torch.full((bs, m), float("nan"), dtype=torch.float32, device=DEV) for _ in range(groups)]
    ops.dequant_gemm_grouped(xs, qws, 2, "b", [L["sc"] for L in Ls], None, outs, m)
    torch.cuda.synchronize()
    for g in range(groups):
        want = np.roll(Ls[g]["y_ref"], g, 0)[:bs, :m]
        got = outs[g].cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all(), g
        assert _rel(got, want) <= TOL_F32, g


@pytest.mark.parametrize("dt", DTS)
def test_graph_replay_delivers_the_arguments(ops, O, dt):
    """three launches with three weight copies in one serial graph, replayed twice: each output equals the eager launch of the same call"""
    m, bs = 48, 16
    L = _layer(ops, O, m, "a_zero_bias", dt)
    x = L["x"][:bs].contiguous()
    copies = [L["qs"].clone() for _ in range(3)]
    copies[1] = torch.roll(copies[1], 64)                                # different weights, not only different addresses
    copies[2] = torch.roll(copies[2], 128)
    eager = [ops.dequant_gemm(x, q, 2, "a", L["sc"], L["zr"], L["bias"]) for q in copies]
    assert not torch.equal(eager[0], eager[1]) and not torch.equal(eager[1], eager[2])
    outs = [torch.empty((bs, m), dtype=dt, device=DEV) for _ in copies]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        for q, y in zip(copies, outs):                                   # warm-up outside the capture (the first launch raises dynamic LDS)
            ops.dequant_gemm(x, q, 2, "a", L["sc"], L["zr"], L["bias"], out=y)
    stream.synchronize()
    with torch.cuda.graph(graph, stream=stream):
        for q, y in zip(copies, outs):
            ops.dequant_gemm(x, q, 2, "a", L["sc"], L["zr"], L["bias"], out=y)
    for _ in range(2):
        for y in outs:
            y.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for y, want in zip(outs, eager):
            assert torch.equal(y, want), int((y != want).sum())
