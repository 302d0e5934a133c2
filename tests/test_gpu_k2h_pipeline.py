"""-m gpu: the issue-ahead schedule of dq_h_kernel <2 bit, RT 1, 4 waves x 4 chunks> (csrc/dq_h_body.inc, K2_AHEAD): the slabs of x for
later chunks are requested between the MFMA steps of earlier ones.  d = 4096 (the only K with 16 chunks of 256), bf16 and fp16, qfn a and b,
with bias; m = 16 is one workgroup (the smallest grid) and 48 three; bs 8 / 9 straddle the half-slab form (HALF: bs <= 8).

(a) against the oracle (fp64 of the reference formula on the same 16-bit-rounded x) at the tolerances of tests/test_gpu_dqgemm_v2.py;
(b) one-hot codes at a random column of every k-chunk: y[b, r] picks x[b, col[r]] out of the row sum, so a slab paired with the wrong
    chunk's weight tile cannot pass;
(c) bit-identical to cfg (2, 44, 4), dq_hr_kernel: x straight into registers, the same chunks per wave, the same MFMA order, the same meet --
    the arithmetic twin that has no slabs and no schedule to get wrong;
(d) rows 0..7 of a bs 16 call are bit-identical to a bs 8 call on the same rows (full slabs against half slabs).
(c) and (d) held at the parent commit too (checked with the parent's library before the schedule changed), so no recorded fixture is needed:
the schedule moves requests and waits, never arithmetic."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = 4096
TOL_F32 = 1e-3
TOL_16 = {torch.bfloat16: 3e-3, torch.float16: 1e-3}
CFG_REGISTER_X = (2, 44, 4)
DTS = [torch.bfloat16, torch.float16]
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


def _layer(ops, O, m, qfn, dt):
    """one layer per (m, qfn, dt), built once: 16 rows of x (a call with bs rows takes the first bs), packed weights, parameters, and the
    oracle's y for all 16 rows"""
    key = (m, qfn, dt)
    if key not in _cache:
        rng = np.random.default_rng(1000 * m + (7 if qfn == "a" else 0) + (1 if dt == torch.float16 else 0))
        W = (0.02 * rng.standard_normal((m, D))).astype(np.float32)
        xt = torch.from_numpy(rng.standard_normal((16, D)).astype(np.float32)).to(dt)
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


def _call(ops, L, bs, qfn, out_dtype=None, cfg=None):
    x, qs, sc, zr, bias, _ = L
    kw = {} if out_dtype is None else {"out_dtype": out_dtype}
    return ops.dequant_gemm(x[:bs].contiguous(), qs, 2, qfn, sc, zr, bias, cfg=cfg, **kw)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("qfn", ["a", "b"])
@pytest.mark.parametrize("m", [16, 48])
@pytest.mark.parametrize("bs", [1, 8, 9, 16])
def test_against_the_oracle(ops, O, dt, qfn, m, bs):
    L = _layer(ops, O, m, qfn, dt)
    y_ref = L[5][:bs]
    y32 = _call(ops, L, bs, qfn, torch.float32)
    r32 = _rel(y32.cpu().numpy().astype(np.float64), y_ref)
    y16 = _call(ops, L, bs, qfn)
    r16 = _rel(y16.float().cpu().numpy().astype(np.float64), y_ref)
    print(f"rel err fp32 y {r32:.3e}, 16-bit y {r16:.3e}")
    assert y32.shape == (bs, m) and y16.dtype == dt
    assert r32 <= TOL_F32
    assert r16 <= TOL_16[dt]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("m", [16, 48])
@pytest.mark.parametrize("bs", [1, 8, 9, 16])
def test_one_hot_codes_pair_every_chunk_with_its_slab(ops, O, dt, m, bs):
    """row r holds code 3 at one random column of chunk perm[r % 16] (a random permutation of the 16 chunks, so every chunk of every wave is
    probed by some row of every 16-row tile) and code 0 elsewhere: with qfn b and scale 1, y[b, r] = 2 x[b, col[r]] - sum_k x[b, k]"""
    rng = np.random.default_rng(9 + m + bs)
    chunk = np.concatenate([rng.permutation(16) for _ in range(m // 16)])
    cols = chunk * 256 + rng.integers(0, 256, size=m)
    assert sorted(set(cols // 256)) == list(range(16))
    codes = np.zeros((m, D), dtype=np.uint8)
    codes[np.arange(m), cols] = 3
    xt = torch.from_numpy(rng.standard_normal((bs, D)).astype(np.float32)).to(dt)
    x = xt.float().numpy()
    qs = ops.pack(torch.from_numpy(codes).to(DEV), 2, ops.LAYOUT_STREAM)
    y = ops.dequant_gemm(xt.to(DEV), qs, 2, "b", torch.tensor([1.0]), None, None, out_dtype=torch.float32).cpu().numpy().astype(np.float64)
    want = O.dequant_linear(x, codes, "b", np.float32(1.0), None, 3, None)
    r = _rel(y, want)
    print(f"rel err {r:.3e}")
    # a slab paired with another chunk's tile moves y[b, r] by 2 (x[b, other] - x[b, col[r]]) ~ 2.8 against |y| ~ sqrt(4096): 4e-2 relative
    assert r <= TOL_F32


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("qfn", ["a", "b"])
@pytest.mark.parametrize("m", [16, 48])
@pytest.mark.parametrize("bs", [9, 16])
def test_bit_identical_to_the_register_x_twin(ops, O, dt, qfn, m, bs):
    L = _layer(ops, O, m, qfn, dt)
    for out_dtype in (torch.float32, None):
        y = _call(ops, L, bs, qfn, out_dtype)
        twin = _call(ops, L, bs, qfn, out_dtype, cfg=CFG_REGISTER_X)
        assert torch.equal(y, twin), (out_dtype, int((y != twin).sum()))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("qfn", ["a", "b"])
@pytest.mark.parametrize("m", [16, 48])
def test_full_slabs_and_half_slabs_agree_on_rows_0_to_7(ops, O, dt, qfn, m):
    L = _layer(ops, O, m, qfn, dt)
    for out_dtype in (torch.float32, None):
        y16 = _call(ops, L, 16, qfn, out_dtype)
        y8 = _call(ops, L, 8, qfn, out_dtype)
        assert torch.equal(y16[:8], y8), (out_dtype, int((y16[:8] != y8).sum()))
