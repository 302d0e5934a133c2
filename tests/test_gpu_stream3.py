"""-m gpu: the STREAM3 layout (3-bit codes at 3 bits per weight) through every layer -- K1 pack / unpack / repack bit for bit against
the NumPy specification (tests/stream3_spec.py), the fused dequant-GEMM of csrc/dqgemm_w3.hip against the fp64 oracle at the project's
own gates (1e-3 fp32 y, 3e-3 y in x's dtype), structure tests no tolerance can blur, the packed layers, the reference checkpoint,
the multi-layer decode helpers."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream3_spec as S3  # noqa: E402
from k2_rules import w3_nw as nw  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL_F32 = 1e-3
TOL_BF16 = 3e-3
BITS = 3


@pytest.fixture(scope="module")
def ops():
    from quip_amd import ops as o
    return o


@pytest.fixture(scope="module")
def O():
    from oracle import quip_oracle
    return quip_oracle


def _case(O, m, d, bs, bits, qfn, seed):
    """the construction of tests/test_gpu_dqgemm.py::_case"""
    rng = np.random.default_rng(seed)
    maxq = 2 ** bits - 1
    W = (0.02 * rng.standard_normal((m, d))).astype(np.float32)
    x = O.bf16_round(rng.standard_normal((bs, d)).astype(np.float32))
    if qfn == "b":
        scale = O.qfnb_scale(W)
        codes = np.clip(np.round(((W / scale + 1) / 2) * maxq), 0, maxq).astype(np.uint8)
        zero = None
    else:
        scale, zero = O.find_params_qfna(W, bits)
        codes = np.clip(np.round(W / scale) + zero, 0, maxq).astype(np.uint8)
    return W, x, codes, scale, zero, maxq


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _pattern(m, d):
    r, k = np.meshgrid(np.arange(m), np.arange(d), indexing="ij")
    return ((5 * r + 3 * k + k // 8) % 8).astype(np.uint8)


# ---- K1 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,d", [(16, 256), (48, 768), (64, 11008), (4096, 4096)])
def test_pack_equals_the_spec_bit_for_bit_and_unpack_inverts_it(ops, m, d):
    rng = np.random.default_rng(m * 7 + d)
    for codes in (rng.integers(0, 8, (m, d), dtype=np.uint8), _pattern(m, d)):
        cd = torch.from_numpy(codes).to(DEV)
        pk = ops.pack(cd, 3, ops.LAYOUT_STREAM3)
        assert pk.dtype == torch.int32 and pk.numel() == m * d * 3 // 32
        assert np.array_equal(pk.cpu().numpy(), S3.pack_stream3(codes))
        assert torch.equal(ops.unpack(pk, 3, ops.LAYOUT_STREAM3, m, d), cd)
    # the container path is untouched by the new layout
    assert ops.pack(cd, 3, ops.LAYOUT_STREAM).numel() == m * d * 4 // 32


@pytest.mark.parametrize("m,d", [(64, 1024), (48, 2048)])
def test_repack_from_the_reference_words(ops, O, m, d):
    codes = np.random.default_rng(d).integers(0, 8, (m, d), dtype=np.uint8)
    canon = torch.from_numpy(O.pack3(codes)).to(DEV)
    got = ops.repack_canonical_to_stream3(canon, m, d)
    assert got.numel() == canon.numel() == m * d * 3 // 32
    assert torch.equal(got, ops.pack(torch.from_numpy(codes).to(DEV), 3, ops.LAYOUT_STREAM3))
    assert np.array_equal(got.cpu().numpy(), S3.pack_stream3(codes))


# ---- K2 --------------------------------------------------------------------------------------------------------------------
SHAPES = [(16, 256, 1), (64, 512, 4), (128, 1024, 16), (48, 768, 17), (256, 512, 64), (2048, 2048, 16), (11008, 4096, 5),
          (4096, 11008, 16), (8192, 8192, 16),
          # every workgroup shape the dispatch can choose (row tiles per workgroup NW by m / 16: csrc/k2_plan.h k2_plan_w3) is checked, not only
          # the ones the shapes above reach (NW 1 and 2): 1024 row tiles -> NW 4 (the D = 4 ring), odd chunk count; 2000 -> NW 8 (two stages per
          # wave and ring step, ragged last ring step, unpaired high chunk); 257 -> NW 2 and 1745 -> NW 7, both with dead waves in the last
          # workgroup; 1792 -> NW 7 exactly
          (16384, 768, 16), (32000, 768, 5), (4112, 512, 16), (27920, 512, 16), (28672, 1024, 7)]


def test_the_added_shapes_reach_every_workgroup_shape(ops):
    """the dispatch rule (tests/k2_rules.py: cost = rounds of 256 workgroups x NW, ties to the larger NW), and the library asked for its plan"""
    assert {ops.dequant_gemm_plan(bs, m, d, 3, layout=ops.LAYOUT_STREAM3)[1][0] for m, d, bs in SHAPES} == {1, 2, 4, 7, 8}
    assert {nw(m) for m, _, _ in SHAPES} == {1, 2, 4, 7, 8}
    assert nw(16384) == 4 and nw(32000) == 8 and nw(4112) == 2 and 257 % 2 and nw(27920) == 7 and 1745 % 7 and nw(28672) == 7


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("qfn", ["a", "b"])
@pytest.mark.parametrize("m,d,bs", SHAPES)
def test_dequant_gemm_matches_oracle(ops, O, m, d, bs, qfn, dtype):
    W, x, codes, scale, zero, maxq = _case(O, m, d, bs, BITS, qfn, seed=m + d + bs + BITS)
    bias = np.random.default_rng(1).standard_normal(m).astype(np.float32)
    xd = torch.from_numpy(x).to(DEV).to(dtype)
    y_ref = O.dequant_linear(xd.float().cpu().numpy(), codes, qfn, scale, zero, maxq, bias)     # the rounded x
    qs = ops.pack(torch.from_numpy(codes).to(DEV), 3, ops.LAYOUT_STREAM3)
    sc = torch.tensor(np.asarray(scale, np.float32).reshape(-1))
    zr = None if zero is None else torch.from_numpy(zero)
    y32 = ops.dequant_gemm(xd, qs, 3, qfn, sc, zr, torch.from_numpy(bias), out_dtype=torch.float32, layout=ops.LAYOUT_STREAM3)
    assert y32.shape == (bs, m)                                   # m derived from numel * 32 // 3 // d
    r32 = _rel(y32.cpu().numpy().astype(np.float64), y_ref)
    y16 = ops.dequant_gemm(xd, qs, 3, qfn, sc, zr, torch.from_numpy(bias), out_dtype=dtype, layout=ops.LAYOUT_STREAM3)
    r16 = _rel(y16.float().cpu().numpy().astype(np.float64), y_ref)
    print(f"[stream3] {m}x{d} bs {bs} qfn {qfn} {dtype}: rel {r32:.2e} (fp32 y) {r16:.2e} (16-bit y)")
    assert r32 <= TOL_F32
    assert y16.dtype == dtype and r16 <= TOL_BF16


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_fc1_of_a_30b_model_on_sampled_rows(ops, dtype):
    """28672 x 7168, bs 16 (the weight-stream shape): 256 sampled output rows -- first, a ragged middle, last -- against fp64"""
    m, d, bs = 28672, 7168, 16
    torch.manual_seed(3)
    W = (0.02 * torch.randn(m, d, device=DEV)).half()
    s = ops.qfnb_scale(W)
    _, codes = ops.quantize(W, 'b', s, None, 7, want_codes=True)
    del W
    x = torch.randn(bs, d, device=DEV).to(dtype)
    qs = ops.pack(codes, 3, ops.LAYOUT_STREAM3)
    y = ops.dequant_gemm(x, qs, 3, 'b', s, None, None, out_dtype=torch.float32, layout=ops.LAYOUT_STREAM3)
    rows = torch.cat([torch.arange(0, 96), torch.arange(14213, 14277), torch.arange(m - 96, m)]).to(DEV)
    What = (codes[rows].double() / 7 * 2 - 1) * float(s.item())
    want = x.double() @ What.T
    rel = float((y[:, rows].double() - want).norm() / want.norm())
    print(f"[stream3] 28672x7168 bs 16 {dtype}: rel {rel:.2e} on {rows.numel()} rows")
    assert rows.numel() == 256 and rel <= TOL_F32


@pytest.mark.parametrize("code", [4, 3, 7])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_one_hot_weights_detect_planes_and_transposes(ops, O, code, dtype):
    """code 4 lives in the high plane only, 3 in the low plane only, 7 in both: y[b, r] = code * x[b, perm[r]]"""
    m, d, bs = 64, 512, 16
    rng = np.random.default_rng(5 + code)
    codes = np.zeros((m, d), dtype=np.uint8)
    cols = rng.permutation(d)[:m]
    codes[np.arange(m), cols] = code
    x = O.bf16_round(rng.standard_normal((bs, d)).astype(np.float32))
    y_ref = float(code) * x[:, cols]
    qs = ops.pack(torch.from_numpy(codes).to(DEV), 3, ops.LAYOUT_STREAM3)
    y = ops.dequant_gemm(torch.from_numpy(x).to(DEV).to(dtype), qs, 3, "a", torch.ones(m), torch.zeros(m), None,
                         out_dtype=torch.float32, layout=ops.LAYOUT_STREAM3)
    np.testing.assert_allclose(y.cpu().numpy(), y_ref, rtol=0, atol=2e-4 * np.abs(x).sum(1, keepdims=True).max())


def test_accumulate_contract_and_determinism(ops, O):
    W, x, codes, scale, zero, maxq = _case(O, 64, 512, 1, BITS, "a", seed=11)
    bias = np.random.default_rng(2).standard_normal(64).astype(np.float32)
    qs = ops.pack(torch.from_numpy(codes).to(DEV), 3, ops.LAYOUT_STREAM3)
    xd = torch.from_numpy(x).to(DEV).to(torch.bfloat16)
    y = torch.from_numpy(bias.copy()).reshape(1, -1).to(DEV)
    ops.dequant_gemm(xd, qs, 3, "a", torch.from_numpy(scale), torch.from_numpy(zero), None, out=y, accumulate=True,
                     layout=ops.LAYOUT_STREAM3)
    y_ref = O.dequant_linear(x, codes, "a", scale, zero, maxq, bias)
    assert _rel(y.cpu().numpy().astype(np.float64), y_ref) <= TOL_F32
    # two identical calls give identical bits (no atomics, a fixed reduction order)
    W, x, codes, scale, zero, maxq = _case(O, 2048, 2048, 16, BITS, "b", seed=12)
    qs = ops.pack(torch.from_numpy(codes).to(DEV), 3, ops.LAYOUT_STREAM3)
    xd = torch.from_numpy(x).to(DEV).to(torch.float16)
    sc = torch.tensor([float(scale)])
    a = ops.dequant_gemm(xd, qs, 3, "b", sc, None, None, out_dtype=torch.float32, layout=ops.LAYOUT_STREAM3)
    b = ops.dequant_gemm(xd, qs, 3, "b", sc, None, None, out_dtype=torch.float32, layout=ops.LAYOUT_STREAM3)
    assert torch.equal(a, b)


def test_grouped_call_and_empty_batch(ops, O):
    m, d, bs = 256, 1024, 7
    xs, qws, scs, refs = [], [], [], []
    for i in range(3):
        W, x, codes, scale, zero, maxq = _case(O, m, d, bs, BITS, "b", seed=20 + i)
        xs.append(torch.from_numpy(x).to(DEV).to(torch.float16))
        qws.append(ops.pack(torch.from_numpy(codes).to(DEV), 3, ops.LAYOUT_STREAM3))
        scs.append(torch.tensor([float(scale)], device=DEV))
        refs.append(O.dequant_linear(x, codes, "b", scale, None, maxq))
    ys = [torch.empty((bs, m), dtype=torch.float32, device=DEV) for _ in range(3)]
    ops.dequant_gemm_grouped(xs, qws, 3, "b", scs, None, ys, m, layout=ops.LAYOUT_STREAM3)
    for y, ref in zip(ys, refs):
        assert _rel(y.cpu().numpy().astype(np.float64), ref) <= TOL_F32
    empty = ops.dequant_gemm(torch.empty((0, d), dtype=torch.float16, device=DEV), qws[0], 3, "b", scs[0], None, None,
                             out_dtype=torch.float32, layout=ops.LAYOUT_STREAM3)
    assert empty.shape == (0, m)


def test_error_paths_on_the_device(ops):
    from quip_amd._lib import QuipAmdError
    x = torch.zeros((4, 384), dtype=torch.float16, device=DEV)
    qw = torch.zeros(16 * 384 * 3 // 32, dtype=torch.int32, device=DEV)
    one = torch.ones(1, device=DEV)
    with pytest.raises(QuipAmdError, match="STREAM3 layout needs"):
        ops.dequant_gemm(x, qw, 3, "b", one, None, None, out_dtype=torch.float32, m=16, layout=ops.LAYOUT_STREAM3)
    x = torch.zeros((4, 256), dtype=torch.float16, device=DEV)
    qw = torch.zeros(16 * 256 * 4 // 32, dtype=torch.int32, device=DEV)
    with pytest.raises(QuipAmdError, match=r"code 4\)"):          # bits = 4 with STREAM3
        ops.dequant_gemm(x, qw, 4, "b", one, None, None, out_dtype=torch.float32, m=16, layout=ops.LAYOUT_STREAM3)
    qw = torch.zeros(16 * 256 * 3 // 32, dtype=torch.int32, device=DEV)
    with pytest.raises(QuipAmdError, match=r"code 4\)"):          # a forced kernel configuration
        ops.dequant_gemm(x, qw, 3, "b", one, None, None, out_dtype=torch.float32, m=16, cfg=(3, 4, 2), layout=ops.LAYOUT_STREAM3)
    with pytest.raises(QuipAmdError, match="STREAM3 layout needs"):
        ops.pack(torch.zeros((16, 384), dtype=torch.uint8, device=DEV), 3, ops.LAYOUT_STREAM3)
    with pytest.raises(ValueError, match="STREAM3"):
        ops.pack(torch.zeros((16, 256), dtype=torch.uint8, device=DEV), 4, ops.LAYOUT_STREAM3)


# ---- layers ----------------------------------------------------------------------------------------------------------------
def _dense(op, transpose=False):
    """the operator as a dense fp64 matrix from its generator tuple (as tests/test_gpu_decode_fused.py::_dense)"""
    (B, p_in, p_out) = op.state()
    n, p, q = op.n, op.p, op.q
    B0 = B[0].to(DEV, torch.float64).reshape(-1, p, p)
    B1 = B[1].to(DEV, torch.float64).reshape(-1, q, q)
    B0 = B0.expand(q, p, p) if B0.shape[0] == 1 else B0
    B1 = B1.expand(p, q, q) if B1.shape[0] == 1 else B1
    x = torch.eye(n, device=DEV, dtype=torch.float64)
    z = x[p_in.to(DEV)].reshape(p, q, n)
    z = torch.einsum('bac,cbk->abk', B0, z)
    z = torch.einsum('abc,ack->abk', B1, z)
    Q = z.reshape(n, n)[p_out.to(DEV)]
    return (Q.t() if transpose else Q).contiguous()


def _pair(d, m, seed, bias=True):
    """the same codes, grid, bias and U / V operators packed once as the container and once as native3"""
    from quip_amd import ops, method
    from quip_amd.quant import QuantLinear
    np.random.seed(seed)
    torch.manual_seed(seed)
    W = (0.02 * torch.randn(m, d, device=DEV)).half()
    s = ops.qfnb_scale(W)
    What, codes = ops.quantize(W, 'b', s, None, 7, want_codes=True)
    U = ops.OrthoOp(method.gen_rand_ortho_butterfly_noblock(m), DEV)
    V = ops.OrthoOp(method.gen_rand_ortho_butterfly_noblock(d), DEV)
    sWH = (0.5 + torch.rand(d)).to(DEV)
    b = (0.1 * torch.randn(m, device=DEV)) if bias else None
    cont = QuantLinear(d, m, bits=3, qfn='b').to(DEV).pack(codes, s, None, bias=b, scaleWH=sWH, U=U, V=V)
    nat = QuantLinear(d, m, bits=3, qfn='b', native3=True).to(DEV).pack(codes, s, None, bias=b, scaleWH=sWH, U=U, V=V)
    return cont, nat, What.double(), codes


def test_native3_layer_against_the_container_layer(ops):
    d, m = 2048, 2048
    cont, nat, What, codes = _pair(d, m, seed=1)
    assert nat.qweight.numel() * 4 == 0.75 * cont.qweight.numel() * 4 and nat.packed_bytes() * 4 == cont.packed_bytes() * 3
    assert np.array_equal(nat.qweight.cpu().numpy(), S3.pack_stream3(codes.cpu().numpy()))
    dense = _dense(cont.U, transpose=True) @ What @ _dense(cont.V) @ torch.diag(cont.inv_scaleWH.double())
    for rows in (5, 16):
        x = torch.randn(rows, d, device=DEV).half()
        want = x.double() @ dense.T + cont.bias.double()
        for ql in (cont, nat):
            got = ql(x)
            rel = float((got.double() - want).norm() / want.norm())
            print(f"[stream3] layer {'native3' if ql.native3 else 'container'} rows {rows}: rel {rel:.2e}")
            assert rel < 2e-3
    # conversion in place gives the words of packing natively; the decode-order copy is the container's, word for word
    conv, _, _, _ = _pair(d, m, seed=1)
    assert conv.to_native3() is conv and conv.native3 and torch.equal(conv.qweight, nat.qweight)
    assert conv.to_native3() is conv
    assert torch.equal(nat.decode_qweight(), cont.decode_qweight())
    assert nat.packed_bytes() == nat.qweight.numel() * 4 + cont.decode_qweight().numel() * 4
    with pytest.raises(ValueError):
        type(cont)(d, m, bits=2, qfn='b').to(DEV).to_native3()


def test_reference_checkpoint_loads_into_a_native3_layer(ops, O):
    from quip_amd import quant as Q
    m, d = 64, 1024
    rng = np.random.default_rng(4)
    W = (0.02 * rng.standard_normal((m, d))).astype(np.float32)
    sc, zr = O.find_params_qfna(W, 3)
    codes = np.clip(np.round(W / sc) + zr, 0, 7).astype(np.uint8)
    bias = rng.standard_normal(m).astype(np.float32)
    sd = {"0.qweight": torch.from_numpy(O.pack3(codes)), "0.scales": torch.from_numpy(sc).reshape(-1, 1),
          "0.zeros": torch.from_numpy(zr * sc).reshape(-1, 1), "0.bias": torch.from_numpy(bias)}
    x = torch.from_numpy(O.bf16_round(rng.standard_normal((5, d)).astype(np.float32)))
    y_ref = O.dequant_linear(x.numpy(), codes, "a", sc, zr, 7, bias)
    # (a) the skeleton already on the GPU
    holder = torch.nn.Sequential(torch.nn.Linear(d, m))
    Q.make_quant3(holder, ["0"], native3=True)
    holder.to(DEV)
    assert holder[0].native3
    holder.load_state_dict({k: v.clone() for k, v in sd.items()})
    # (b) the reference's flow: make_quant3 and load_state_dict on the CPU, then .to(dev)
    lazy = torch.nn.Sequential(torch.nn.Linear(d, m))
    Q.make_quant3(lazy, ["0"], native3=True)
    lazy.load_state_dict({k: v.clone() for k, v in sd.items()})
    lazy.to(DEV)
    # (c) from the buffers
    direct = Q.from_reference_packed(sd["0.qweight"], sd["0.scales"], sd["0.zeros"], sd["0.bias"], 3, device=DEV, native3=True)
    for ql in (holder[0], lazy[0], direct):
        assert ql.native3 and ql.qweight.numel() == m * d * 3 // 32
        assert np.array_equal(ops.unpack(ql.qweight, 3, ops.LAYOUT_STREAM3, m, d).cpu().numpy(), codes)
        got = ql(x.to(DEV).bfloat16())
        assert _rel(got.double().cpu().numpy(), y_ref) <= TOL_BF16  # the layer answers in x's dtype (bf16)
    # the default stays the container
    plain = torch.nn.Sequential(torch.nn.Linear(d, m))
    Q.make_quant3(plain, ["0"])
    assert not plain[0].native3 and plain[0].qweight.numel() == m * d * 4 // 32


def test_model_checkpoint_round_trip_keeps_layout_and_words(ops, tmp_path):
    from quip_amd import quant as Q
    cont, nat, _, _ = _pair(512, 256, seed=2)
    model = torch.nn.Sequential(torch.nn.Linear(512, 256), torch.nn.Linear(512, 256)).to(DEV)
    path = str(tmp_path / "m.pt")
    Q.save_model(model, {"0": nat, "1": cont}, path)
    fresh = torch.nn.Sequential(torch.nn.Linear(512, 256), torch.nn.Linear(512, 256))
    layers = Q.load_model(fresh, path, DEV)
    assert layers["0"].native3 and not layers["1"].native3
    assert torch.equal(layers["0"].qweight, nat.qweight) and torch.equal(layers["1"].qweight, cont.qweight)
    x = torch.randn(4, 512, device=DEV).half()
    for new, old in ((fresh[0], nat), (fresh[1], cont)):
        a, b = new(x).double(), old(x).double()
        assert float((a - b).norm() / b.norm()) <= 1e-3


@pytest.mark.parametrize("rows", [5, 16])
@pytest.mark.parametrize("mixed", [False, True], ids=["native3", "mixed"])
def test_multi_layer_decode_helpers_follow_the_layout(ops, rows, mixed):
    """q / k / v-like group at hidden 2048: packed_forward_fused and packed_gemm_stage on native3 layers (or one native3 beside two
    container layers) against the same group as container layers"""
    from quip_amd import quant as Q
    d = m = 2048
    pairs = [_pair(d, m, seed=10 + i) for i in range(3)]
    conts = [p[0] for p in pairs]
    group = [p[1] if (not mixed or i == 0) else p[0] for i, p in enumerate(pairs)]
    assert [q.native3 for q in group] == ([True, False, False] if mixed else [True, True, True])
    x = torch.randn(rows, d, device=DEV).half()
    ln = torch.nn.LayerNorm(d).to(DEV).half()
    for a, b in zip(Q.packed_forward_fused(group, x, ln=ln), Q.packed_forward_fused(conts, x, ln=ln)):
        rel = float((a.double() - b.double()).norm() / b.double().norm())
        print(f"[stream3] packed_forward_fused rows {rows} mixed {mixed}: {rel:.2e}")
        assert rel <= 3e-3
    xts = [torch.randn(rows, d, device=DEV).half() for _ in range(3)]
    for a, b in zip(Q.packed_gemm_stage(group, xts), Q.packed_gemm_stage(conts, xts)):
        rel = float((a.double() - b.double()).norm() / b.double().norm())
        print(f"[stream3] packed_gemm_stage rows {rows} mixed {mixed}: {rel:.2e}")
        assert rel <= 3e-3
