"""-m gpu: WHERE every kernel-launching entry point of the C ABI writes (tests/guard_arena.py).

The parity tests tie every kernel's values to an fp64 reference; here every output and every workspace of a call is carved out of a guard
arena (a known byte pattern on either side, the tensor itself filled with 0xFF), and each case asserts

  1. no byte outside a carved tensor changed (`arena.check()`);
  2. no element of an output still holds the 0xFF fill, except the parts the header documents as not written (PARTIAL below: the padding
     columns of strided outputs, the strict lower part of a triangular inverse, the tiles above the block-lower triangle of `Hacc`), which
     must still hold what they held;
  3. every `const` input has its bits; in-place arguments changed only where documented;
  4. the result is, bit for bit, what the same call gives on ordinary torch tensors (the calls the parity tests tie to fp64) -- for the
     entry points that accumulate with floating-point atomics (NONDETERMINISTIC below) the existing gate against fp64 instead;
  5. a second guarded run whose "uninitialised" fill is 0x00 gives the same bits: nothing depends on what an output or a workspace held.

The last test reads the call ledger: every name of quip_amd._lib.SIGNATURES ran under an arena, except EXEMPT (functions that launch nothing).
No case tries to make a kernel overrun; that the guard can fire is shown by tests/test_guard_arena_host.py and the positive control below."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import guard_arena as G  # noqa: E402
from k2_rules import k2_branch, plan_branch, w3_nw as nw  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32

# entry points whose result depends on the order of floating-point atomics: held to the project's gate against fp64 instead of bit equality
NONDETERMINISTIC = {
    "dequant_gemm accumulate=True": "dqgemm.hip: under the accumulate contract K is split over workgroups that meet in y through fp32 atomics "
                                    "(gate 1e-3 relative, test_gpu_dqgemm.py)",
    "vecquant3matmul / vecquant4matmul": "vecquant.hip: two accumulate-mode dequant-GEMMs into `mul` (gate 1e-4, test_gpu_refformats.py)",
    "decode_bigp_v_gemm without partials / xt": "decode_bigp.hip: the K-slices are added into y with fp32 atomics (gate 3e-3, test_gpu_decode_bigp.py)",
}
# (quipamd_qfnb_scale adds its per-workgroup sums into ONE fp64 word with an atomic and rounds the mean to fp32 / fp16: test_gpu_pack_grid.py
#  asserts it bit-exact against the reference, and so it is held to bit equality here.)

# functions of the C ABI that launch nothing
EXEMPT = {
    "quipamd_version", "quipamd_last_error", "quipamd_probe_set", "quipamd_decode_prefetch_next", "quipamd_tune_dequant_gemm",
    "quipamd_vecquant_invalidate", "quipamd_vecquant_workspace_bytes", "quipamd_ortho_apply_tiles_supported", "quipamd_ortho_apply_bigp_supported",
    "quipamd_ortho_blocked_supported", "quipamd_decode_bigp_supported", "quipamd_ortho_blocked_config", "quipamd_decode_attention_config",
    "quipamd_dequant_gemm_grouped_config", "quipamd_cholesky_config", "quipamd_ldlq_config", "quipamd_decode_attention_fused_max_len",
    "quipamd_preproc_workspace_bytes", "quipamd_gptq_qfnb_workspace_bytes", "quipamd_gptq_qfnb_info_offset", "quipamd_gptq_qfnb_debug",
    "quipamd_hessian_fast_workspace", "quipamd_decode_attention_grouped_workspace_bytes", "quipamd_dequant_gemm_plan",
}


# ------------------------------------------------------------------------------------------------------------------------ harness
class Plain:
    """the allocator of the unguarded run: ordinary torch tensors with the interface of GuardArena"""
    device = torch.device(DEV)

    def take(self, shape, dtype, fill=None, name=None, stride=None):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        t = torch.empty(shape, dtype=dtype, device=DEV) if stride is None else torch.empty_strided(shape, stride, dtype=dtype, device=DEV)
        return t if fill is None else t.fill_(fill)

    def copy_of(self, t, name=None):
        out = torch.empty_like(t)
        out.copy_(t)
        return out


def _mods(*names):
    import importlib
    return [importlib.import_module("quip_amd." + n) for n in names]


def window(n):
    """a strided output [rows, ld]: the first n columns are written, the padding columns are not"""
    def mask(t):
        w = torch.zeros(t.shape, dtype=torch.bool, device=t.device)
        w[..., :n] = True
        return w
    return mask


def block_lower(t):
    """Hacc [d, d]: whatever the tile (64 or 128 columns), the elements with column // 128 > row // 128 lie in tiles above the block-lower triangle"""
    i = torch.arange(t.shape[0], device=t.device)
    return ~((i[None, :] // 128) > (i[:, None] // 128))


def upper_and_diagonal_blocks(t):
    i = torch.arange(t.shape[0], device=t.device)
    return (i[None, :] >= i[:, None]) | ((i[None, :] // 128) == (i[:, None] // 128))


# outputs that include/quip_amd.h (or the wrapper's docstring) documents as PARTLY written: output -> (what is written, its mask).  Everything
# outside the mask must still hold what it held before the call; every other output of every case must be written completely.
PARTIAL = {
    "ortho_apply_tiles out [rows, ldo]": ("the first n columns of every row (`ldo` is a leading dimension)", window),
    "ortho_apply_small_ops out [rows, ldo]": ("the first n columns of every row", window),
    "decode_fused_gemm t_out [bs, ld_t]": ("the first d columns of every row (`ld_t` is a row stride)", window),
    "decode_bigp_u out [rows, ld_out]": ("the n columns `dest` names, all below n here; the padding columns of every row are not written", window),
    "decode_head logits [bs, ld_logits]": ("the first `vocab` columns of every row", window),
    "decode_embed out [bs, ld_out]": ("the first n columns of every row", window),
    "decode_attention out [bs, ld]": ("the first heads * hd columns of every row (ops.decode_attention allocates [bs, ld] for strided q / k / v)", window),
    "hessian_accum Hacc [d, d]": ("the tiles of the block-lower triangle; \"the tiles above it are left untouched\"", block_lower),
    "unit_upper_inverse X [d, d]": ("the upper triangle and the 128 x 128 diagonal blocks (zeros below the diagonal); \"the blocks below them are NOT written\"",
                                    upper_and_diagonal_blocks),
}


def contract(monkeypatch, case, inputs, modules=("ops",), arena_mb=192, partial=None, gate=None, prepare=None, min_regions=1):
    """run `case(alloc) -> {name: tensor}` (outputs and in-place arguments) on plain tensors, under a 0xFF arena and under a 0x00 arena and
    assert the five points of the module docstring.  inputs: {name: tensor} that must keep their bits.  partial: {output name: mask
    function} for outputs the header documents as partly written.  gate: for NONDETERMINISTIC calls, gate(outs) asserts the existing
    tolerance against fp64 (bit equality is then not asked).  prepare(): called before every run (drop address- or layer-keyed caches)."""
    partial = partial or {}
    mods = _mods(*modules)
    fz = G.freeze(**inputs)
    if prepare:
        prepare()
    ref = {k: v.clone() for k, v in case(Plain()).items()}
    torch.cuda.synchronize()
    fz.assert_frozen()
    if gate:
        gate(ref)
    runs, problems = [], []
    for uninit in (0xFF, 0x00):
        if prepare:
            prepare()
        arena = G.GuardArena(arena_mb << 20, DEV, uninit=uninit)
        with G.installed(monkeypatch, arena, *mods):
            outs = case(arena)
            torch.cuda.synchronize()
        tag = f"[fill {uninit:#04x}] "
        problems += [tag + repr(v) for v in arena.check()]
        problems += [tag + "input changed: " + n for n in fz.changed()]
        if len(arena.regions) < min_regions:
            problems.append(tag + f"only {len(arena.regions)} tensors came from the arena: the call is not guarded")
        for name, t in outs.items():
            if name in partial:
                w = partial[name](t)
                left, kept, want = G.count_fill(t[w]), G.count_fill(t[~w], uninit), int((~w).sum())
                if kept != want:
                    problems.append(tag + f"{name}: {want - kept} elements outside the documented part were written")
            else:
                left = G.count_fill(t)
            if uninit == 0xFF and left:
                problems.append(tag + f"{name}: {left} of {t.numel()} elements still hold the 0xFF fill")
            if gate is None:
                if name in partial:
                    w = partial[name](t)
                    same = G.bit_equal(t[w], ref[name][w])
                else:
                    same = G.bit_equal(t, ref[name])
                if not same:
                    problems.append(tag + f"{name}: differs from the unguarded call")
        if gate:
            gate(outs)
        runs.append(outs)
    if gate is None:
        for name in runs[0]:
            a, b = runs[0][name], runs[1][name]
            if name in partial:
                w = partial[name](a)
                a, b = a[w], b[w]
            if not G.bit_equal(a, b):
                problems.append(f"{name}: the result depends on what the outputs / workspaces held before the call")
    if prepare:
        prepare()                                         # nothing a cached layer derived keeps a view of the last arena alive
    assert not problems, "\n".join(problems)
    return ref, runs


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


# The two entry points that synchronise workgroups through memory (quipamd_gptq_round_qfnb, quipamd_decode_attention_grouped) get a time limit
# of their own where the pytest-timeout plugin is installed: 120 s, method "thread" -- a host thread blocked in a device synchronisation
# takes no signal, so the plugin ends the whole process and nothing more runs on the GPU.  Without the plugin the mark would be a silent
# no-op: it is then not applied, and the limit of such a case is the one of the command that runs the suite (`timeout -k 10 N python -m
# pytest ...`, README.md).
import importlib.util  # noqa: E402

own_time_limit = pytest.mark.timeout(120, method="thread") if importlib.util.find_spec("pytest_timeout") else (lambda f: f)


@pytest.fixture(scope="module")
def ops():
    from quip_amd import ops as o
    return o


# ------------------------------------------------------------------------------------------------------------------------ controls
def test_positive_control_a_byte_behind_a_carved_tensor_is_reported_on_the_device():
    """an ordinary in-bounds torch write on the arena tensor itself, one byte past the end of a carved view: check() names it"""
    arena = G.GuardArena(4 << 20, DEV)
    arena.take((3, 40), F16, name="left")
    y = arena.take((5, 28), F32, name="y")
    assert y.is_cuda and y.data_ptr() % 256 == 0 and bool(torch.isnan(y).all()) and arena.check() == []
    r = next(r for r in arena.regions if r["name"] == "y")
    arena.buf[r["end"]] = 0
    arena.buf[r["start"] - 2] = 1
    got = {(v.name, v.side): (v.first, v.last, v.nbytes) for v in arena.check()}
    assert got == {("y", "after"): (1, 1, 1), ("y", "before"): (2, 2, 1)}
    assert "1 byte(s) changed 1..1 bytes after the end of y" in repr([v for v in arena.check() if v.side == "after"][0])
    y.fill_(1.0)                                              # writes inside the live range are the kernel's business
    assert len(arena.check()) == 2


def test_the_proxy_guards_a_wrapper_allocation_and_the_ledger_sees_the_call(monkeypatch, ops):
    codes = torch.randint(0, 4, (16, 256), dtype=torch.uint8, device=DEV)
    arena = G.GuardArena(8 << 20, DEV)
    ledger = set()
    with G.installed(monkeypatch, arena, ops, ledger=ledger):
        out = ops.pack(codes, 2, ops.LAYOUT_STREAM)
        torch.cuda.synchronize()
    assert ops.torch is torch and ledger == {"quipamd_pack"}
    assert arena.buf.data_ptr() <= out.data_ptr() < arena.buf.data_ptr() + arena.buf.numel() and len(arena.regions) == 1
    assert arena.check() == [] and torch.equal(out, ops.pack(codes, 2, ops.LAYOUT_STREAM))


# ------------------------------------------------------------------------------------------------------------------------ K1
@pytest.mark.parametrize("m,d", [(16, 256), (48, 768)])
@pytest.mark.parametrize("bits,layout", [(2, 0), (3, 0), (4, 0), (2, 1), (3, 1), (4, 1), (3, 2)])
def test_pack_unpack(monkeypatch, ops, m, d, bits, layout):
    g = torch.Generator().manual_seed(m + bits + layout)
    codes = torch.randint(0, 2 ** bits, (m, d), generator=g, dtype=torch.uint8).to(DEV)

    def case(A):
        packed = ops.pack(codes, bits, layout)
        return {"packed": packed, "codes": ops.unpack(packed, bits, layout, m, d)}
    ref, _ = contract(monkeypatch, case, {"codes": codes}, min_regions=2)
    assert torch.equal(ref["codes"], codes)


@pytest.mark.parametrize("m,d", [(16, 256), (48, 768)])
@pytest.mark.parametrize("bits", [2, 3, 4])
def test_repack_canonical_to_stream_and_stream3(monkeypatch, ops, m, d, bits):
    g = torch.Generator().manual_seed(m + bits)
    codes = torch.randint(0, 2 ** bits, (m, d), generator=g, dtype=torch.uint8).to(DEV)
    canon = ops.pack(codes, bits, ops.LAYOUT_CANONICAL)

    def case(A):
        out = {"stream": ops.repack_canonical_to_stream(canon, bits, m, d)}
        if bits == 3:
            out["stream3"] = ops.repack_canonical_to_stream3(canon, m, d)
        return out
    ref, _ = contract(monkeypatch, case, {"canonical": canon})
    assert torch.equal(ref["stream"], ops.pack(codes, bits, ops.LAYOUT_STREAM))
    if bits == 3:
        assert torch.equal(ref["stream3"], ops.pack(codes, 3, ops.LAYOUT_STREAM3))


# ------------------------------------------------------------------------------------------------------------------------ K5
@pytest.mark.parametrize("dtype", [F16, BF16, F32])
@pytest.mark.parametrize("m,d", [(1, 1), (37, 100)])                      # neither a multiple of 64
def test_grid_functions(monkeypatch, ops, dtype, m, d):
    g = torch.Generator().manual_seed(m + d)
    W = (0.02 * torch.randn(m, d, generator=g)).to(dtype).to(DEV)
    sa = (0.01 + 0.01 * torch.rand(m, generator=g)).to(DEV)
    za = torch.randint(0, 8, (m,), generator=g).float().to(DEV)

    def case(A):
        s = ops.qfnb_scale(W)
        out = {"scale": s, "grid_b": ops.gridmap(W, "b", s, None, 7), "grid_a": ops.gridmap(W, "a", sa, za, 7),
               "q_only": ops.quantize(W, "c", sa, za, 7)}
        out["q_b"], out["codes_b"] = ops.quantize(W, "b", s, None, 7, want_codes=True)
        out["q_a"], out["codes_a"] = ops.quantize(W, "a", sa, za, 15, want_codes=True)
        for dt in (F16, BF16, F32):
            out[f"w_b_{dt}"] = ops.codes_to_weight(out["codes_b"], "b", s, None, 7, out_dtype=dt)
        out["w_a"] = ops.codes_to_weight(out["codes_a"], "a", sa, za, 15, out_dtype=F32)
        return out
    contract(monkeypatch, case, {"W": W, "scale_a": sa, "zero_a": za}, min_regions=12)      # (qfnb_scale: its one-double workspace too)


# ------------------------------------------------------------------------------------------------------------------------ K2, container
FAM_OLD, FAM_H, FAM_S, FAM_MB = 1, 2, 3, 4


def _k2(ops, m, d, bs, bits, dt, seed, layout=None):
    """random codes, x, grid and bias of a packed layer + its fp64 result (the formula of include/quip_amd.h on the rounded x)"""
    layout = ops.LAYOUT_STREAM if layout is None else layout
    g = torch.Generator().manual_seed(seed)
    maxq = 2 ** bits - 1
    codes = torch.randint(0, maxq + 1, (m, d), generator=g, dtype=torch.uint8).to(DEV)
    x = torch.randn(bs, d, generator=g).to(dt).to(DEV)
    bias = torch.randn(m, generator=g).to(DEV)
    if bits == 4:                                                         # qfn a: per-row scale and zero
        qfn, scale, zero = "a", (0.01 + 0.01 * torch.rand(m, generator=g)).to(DEV), torch.randint(0, maxq + 1, (m,), generator=g).float().to(DEV)
        What = scale.double()[:, None] * (codes.double() - zero.double()[:, None])
    else:
        qfn, scale, zero = "b", torch.tensor([0.05], device=DEV), None
        What = (codes.double() / maxq * 2 - 1) * 0.05
    qs = ops.pack(codes, bits, layout)
    want = x.double() @ What.T + bias.double()
    return dict(x=x, qs=qs, qfn=qfn, scale=scale, zero=zero, bias=bias, want=want, bits=bits, m=m, layout=layout)


def _k2_inputs(c):
    return {k: c[k] for k in ("x", "qs", "scale", "zero", "bias")}


def _k2_call(ops, c, out_dtype, cfg=None):
    return ops.dequant_gemm(c["x"], c["qs"], c["bits"], c["qfn"], c["scale"], c["zero"], c["bias"], out_dtype=out_dtype, m=c["m"], cfg=cfg,
                            layout=c["layout"])


K2_DEFAULT = [(16, 256, 1), (48, 768, 17), (176, 4096, 11), (2048, 8192, 9), (1040, 768, 100), (3072, 512, 300),
              (2048, 8192, 5), (96, 6144, 3), (16384, 512, 5), (8192, 256, 897),
              (8192, 2048, 16), (8192, 4096, 16), (12288, 4096, 16)]          # family h with 2 / 2 / 4 row tiles per workgroup


def test_the_default_shapes_reach_every_branch_of_the_dispatch(ops):
    """every branch is reached -- by the rules (tests/k2_rules.py) and by the library, asked for its plan"""
    got = {k2_branch(2, f16, m, d, bs) for m, d, bs in K2_DEFAULT for f16 in (False, True)}
    assert got == {plan_branch(ops.dequant_gemm_plan(bs, m, d, 2, x_dtype=F16 if f16 else BF16), 2) for m, d, bs in K2_DEFAULT for f16 in (False, True)}
    assert got == {"h", "h rt2 8x1", "h rt2 4x4", "h rt4 4x4", "h-half", "h-half x 2", "s", "mb", "round-1"}
    assert k2_branch(2, True, 8192, 2048, 16) == "h rt2 8x1" and k2_branch(2, False, 8192, 4096, 16) == "h rt2 4x4" and k2_branch(2, True, 12288, 4096, 16) == "h rt4 4x4"
    assert k2_branch(2, False, 48, 768, 17) == "round-1" and k2_branch(2, True, 48, 768, 17) == "mb" and k2_branch(2, False, 8192, 256, 897) == "mb"
    assert k2_branch(2, True, 2048, 8192, 9) == "h-half x 2" and k2_branch(2, True, 16384, 512, 5) == "s" and k2_branch(2, True, 96, 6144, 3) == "h-half"


@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("bits", [2, 4])
@pytest.mark.parametrize("m,d,bs", K2_DEFAULT)
def test_dequant_gemm_default_dispatch(monkeypatch, ops, m, d, bs, bits, dt):
    c = _k2(ops, m, d, bs, bits, dt, seed=m + d + bs + bits)

    def case(A):
        # the plan of this very call, asked under the arena as well: it launches nothing and carves nothing
        assert plan_branch(ops.dequant_gemm_plan(bs, m, d, bits, x_dtype=dt), bits) == k2_branch(bits, dt == F16, m, d, bs)
        return {"y32": _k2_call(ops, c, F32), "y16": _k2_call(ops, c, dt)}
    ref, _ = contract(monkeypatch, case, _k2_inputs(c), min_regions=2)
    assert _rel(ref["y32"], c["want"]) <= 1e-3


FORCED = ([((FAM_H, 8, 1), (176, 2048, 11), 2), ((FAM_H, 8, 2), (176, 2048, 11), 2), ((FAM_H, 4, 4), (176, 2048, 11), 2), ((FAM_H, 4, 4), (48, 768, 9), 2),
           ((FAM_H, 44, 4), (176, 4096, 11), 2), ((FAM_H, 44, 4), (16, 4096, 5), 2), ((FAM_H, 8, 2), (176, 1024, 11), 4), ((FAM_H, 8, 4), (48, 768, 9), 4)]
          + [((FAM_S, a, b), shape, 2) for (a, b) in ((7, 2), (4, 2), (8, 1), (2, 4), (1, 8)) for shape in ((1808, 1024, 16), (16, 768, 5))]
          + [((FAM_S, 7, 2), (112, 256, 1), 4)]
          + [((FAM_MB, p), (1040, 768, 100), 2) for p in (44, 22, 45, 23, 48, 49, 46, 47)]
          + [((FAM_MB, 44), (3072, 512, 300), 4), ((FAM_MB, 22), (256, 256, 17), 4), ((FAM_OLD,), (48, 768, 17), 2), ((FAM_OLD,), (1040, 768, 100), 4)])


@pytest.mark.parametrize("cfg,shape,bits,dt", [(c, s_, b, dt) for c, s_, b in FORCED for dt in (BF16, F16) if not (c[0] == FAM_OLD and dt == F16)])
def test_dequant_gemm_forced_kernels(monkeypatch, ops, cfg, shape, bits, dt):
    """one instantiation of every family and form test_gpu_dqgemm_v2.py forces, at a shape that over-covers (ragged row tiles, ragged batch,
    odd stage counts); bf16 and fp16 x (the round-1 family: bf16, its only dtype), fp32 and 16-bit y"""
    m, d, bs = shape
    c = _k2(ops, m, d, bs, bits, dt, seed=m + d + bs)

    def case(A):
        return {"y32": _k2_call(ops, c, F32, cfg), "y16": _k2_call(ops, c, dt, cfg)}
    ref, _ = contract(monkeypatch, case, _k2_inputs(c), min_regions=2)
    assert _rel(ref["y32"], c["want"]) <= 1e-3


ROUND1 = ([((512, 2048, 16), t) for t in [(1, 0, 16, 0), (2, 0, 8, 0), (4, 0, 4, 0), (8, 0, 16, 200), (4, 0, 16, 200), (1, 1, 8, 0), (4, 1, 4, 0), (2, 2, 4, 0), (1, 4, 4, 0)]]
          # 3 row tiles: a forced row-tile count that does not divide them falls back to 1 (dqgemm.hip launch<>), the waves stay as forced
          + [((48, 768, 9), t) for t in [(1, 0, 16, 0), (2, 0, 8, 0), (4, 0, 4, 0), (1, 1, 8, 0), (2, 2, 4, 0), (1, 4, 4, 0)]])


@pytest.mark.parametrize("shape,tune", ROUND1)
def test_dequant_gemm_round1_workgroup_shapes(monkeypatch, ops, shape, tune):
    """the round-1 kernels (bf16) through quipamd_tune_dequant_gemm: tile kernel and per-wave kernel in their forced workgroup shapes"""
    m, d, bs = shape
    from quip_amd import _lib
    c = _k2(ops, m, d, bs, 2, BF16, seed=m + bs)
    lib = _lib.load()

    def case(A):
        lib.quipamd_tune_dequant_gemm(*tune)
        try:
            return {"y32": _k2_call(ops, c, F32), "y16": _k2_call(ops, c, BF16)}
        finally:
            lib.quipamd_tune_dequant_gemm(0, 0, 0, 0)
    ref, _ = contract(monkeypatch, case, _k2_inputs(c), min_regions=2)
    assert _rel(ref["y32"], c["want"]) <= 1e-3


@pytest.mark.parametrize("rt,nw,split", [(0, 0, 0), (4, 16, 4), (2, 8, 3), (1, 16, 1)])       # 0: the heuristic; else row tiles, waves, k-slices forced
@pytest.mark.parametrize("m,d,bs,bits", [(64, 512, 3, 2), (2048, 2048, 7, 2), (1024, 4096, 16, 4)])
def test_dequant_gemm_accumulate_into_the_callers_y(monkeypatch, ops, rt, nw, split, m, d, bs, bits):
    """accumulate=True: y carved by hand, pre-filled by the caller; split-K with fp32 atomics (NONDETERMINISTIC): the 1e-3 gate"""
    from quip_amd import _lib
    c = _k2(ops, m, d, bs, bits, BF16, seed=m + bs)
    y0 = torch.randn(bs, m, device=DEV)
    want = y0.double() + c["want"]
    lib = _lib.load()

    def case(A):
        y = A.copy_of(y0, name="y")
        if rt:
            lib.quipamd_tune_dequant_gemm(rt, 0, nw, split)
        try:
            ops.dequant_gemm(c["x"], c["qs"], bits, c["qfn"], c["scale"], c["zero"], c["bias"], out=y, accumulate=True)
        finally:
            lib.quipamd_tune_dequant_gemm(0, 0, 0, 0)
        return {"y": y}

    def gate(outs):
        assert _rel(outs["y"], want) <= 1e-3
    contract(monkeypatch, case, dict(_k2_inputs(c), y0=y0), gate=gate)


GROUPED = ([(form, 2064, 2, 9, 4096) for form in (74, 72, 81, 4, 2, 1, 0)] + [(form, 4096, 3, 5, 4096) for form in (74, 72, 81, 4, 0)]
           + [(0, 176, 3, 16, 2048), (2, 176, 2, 1, 2048), (0, 11008, 2, 16, 4096)])


@pytest.mark.parametrize("form,m,groups,bs,d", GROUPED)
def test_dequant_gemm_grouped(monkeypatch, ops, form, m, groups, bs, d):
    """the grouped call in the forms of the weight-stream kernel (129 row tiles: ragged at 4 / 7 / 8 per workgroup) and of the grouped h kernel"""
    cs = [_k2(ops, m, d, bs, 2, F16, seed=10 * g + bs + m) for g in range(groups)]

    def case(A):
        outs = [A.take((bs, m), F32, name=f"y{g}") for g in range(groups)]
        ops.dequant_gemm_grouped_config(form)
        try:
            ops.dequant_gemm_grouped([c["x"] for c in cs], [c["qs"] for c in cs], 2, "b", [c["scale"] for c in cs], None, outs, m)
        finally:
            ops.dequant_gemm_grouped_config(0)
        return {f"y{g}": o for g, o in enumerate(outs)}
    inputs = {f"{k}{g}": c[k] for g, c in enumerate(cs) for k in ("x", "qs", "scale")}
    ref, _ = contract(monkeypatch, case, inputs, min_regions=groups)
    for g, c in enumerate(cs):
        assert _rel(ref[f"y{g}"], c["want"] - c["bias"].double()) <= 1e-3


# ------------------------------------------------------------------------------------------------------------------------ K2, STREAM3
W3_SHAPES = [(16, 256, 1), (48, 768, 17), (4112, 512, 16), (27920, 512, 16), (32000, 768, 5), (16384, 768, 16), (2048, 2048, 16)]


def test_the_stream3_shapes_reach_every_workgroup_shape(ops):
    """the dispatch rule of the STREAM3 layout (tests/k2_rules.py, as in test_gpu_stream3.py), and the library asked for its plan"""
    assert {ops.dequant_gemm_plan(bs, m, d, 3, layout=ops.LAYOUT_STREAM3)[1][0] for m, d, bs in W3_SHAPES} == {1, 2, 4, 7, 8}
    assert {nw(m) for m, _, _ in W3_SHAPES} == {1, 2, 4, 7, 8}
    assert nw(4112) == 2 and 257 % 2 and nw(27920) == 7 and 1745 % 7 and nw(32000) == 8 and 2000 % 8 == 0 and nw(16384) == 4


@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("m,d,bs", W3_SHAPES)
def test_stream3_dequant_gemm(monkeypatch, ops, m, d, bs, dt):
    c = _k2(ops, m, d, bs, 3, dt, seed=m + d + bs, layout=ops.LAYOUT_STREAM3)

    def case(A):
        return {"y32": _k2_call(ops, c, F32), "y16": _k2_call(ops, c, dt)}
    ref, _ = contract(monkeypatch, case, _k2_inputs(c), min_regions=2)
    assert _rel(ref["y32"], c["want"]) <= 1e-3


def test_stream3_grouped_accumulate_and_empty_batch(monkeypatch, ops):
    m, d, bs = 256, 1024, 7
    cs = [_k2(ops, m, d, bs, 3, F16, seed=20 + i, layout=ops.LAYOUT_STREAM3) for i in range(3)]
    y0 = torch.randn(bs, m, device=DEV)

    def case(A):
        ys = [A.take((bs, m), F32, name=f"y{i}") for i in range(3)]
        ops.dequant_gemm_grouped([c["x"] for c in cs], [c["qs"] for c in cs], 3, "b", [c["scale"] for c in cs], None, ys, m, layout=ops.LAYOUT_STREAM3)
        acc = A.copy_of(y0, name="acc")                      # STREAM3 under the accumulate contract: no atomics, a fixed reduction order
        ops.dequant_gemm(cs[0]["x"], cs[0]["qs"], 3, "b", cs[0]["scale"], None, cs[0]["bias"], out=acc, accumulate=True, layout=ops.LAYOUT_STREAM3)
        empty = ops.dequant_gemm(cs[0]["x"][:0], cs[0]["qs"], 3, "b", cs[0]["scale"], None, None, out_dtype=F32, m=m, layout=ops.LAYOUT_STREAM3)
        assert empty.shape == (0, m)
        return dict({f"y{i}": y for i, y in enumerate(ys)}, acc=acc)
    inputs = {f"{k}{i}": c[k] for i, c in enumerate(cs) for k in ("x", "qs", "scale")}
    ref, _ = contract(monkeypatch, case, dict(inputs, y0=y0), min_regions=4)
    assert _rel(ref["acc"], y0.double() + cs[0]["want"]) <= 1e-3


# ------------------------------------------------------------------------------------------------------------------------ vecquant
@pytest.mark.parametrize("bits", [3, 4])
@pytest.mark.parametrize("prepared", [True, False])
def test_vecquant_matmul_with_a_workspace_of_exactly_the_queried_bytes(monkeypatch, ops, bits, prepared):
    """the wrapper allocates quipamd_vecquant_workspace_bytes and not a byte more: the guard band starts right behind it.  prepared: the
    first call registers the workspace (quipamd_vecquant_prepare), the second runs on it; unprepared: a strided `mat` takes the stateless path"""
    from quip_amd import _lib
    m, d = 48, 1024
    g = torch.Generator().manual_seed(bits)
    codes = torch.randint(0, 2 ** bits, (m, d), generator=g, dtype=torch.uint8).to(DEV)
    canon = ops.pack(codes, bits, ops.LAYOUT_CANONICAL)
    if not prepared:
        wide = torch.zeros((canon.shape[0], 2 * m), dtype=torch.int32, device=DEV)
        wide[:, :m] = canon
        canon = wide[:, :m]
        assert not canon.is_contiguous()
    vec = torch.randn(d, generator=g).to(DEV)
    scales = (0.01 + 0.01 * torch.rand(m, generator=g)).to(DEV)
    zeros = (torch.randint(0, 2 ** bits, (m,), generator=g).float().to(DEV) * scales)
    bias = torch.randn(m, generator=g).to(DEV)
    want = bias.double() + (scales.double()[:, None] * codes.double() - zeros.double()[:, None]) @ vec.double()
    nbytes = _lib.load().quipamd_vecquant_workspace_bytes(bits, m, d)

    def case(A):
        mul = A.copy_of(bias, name="mul")
        ops.vecquantmatmul(bits, vec, canon, mul, scales, zeros)
        if prepared:
            mul.copy_(bias)
            ops.vecquantmatmul(bits, vec, canon, mul, scales, zeros)
        if not isinstance(A, Plain):
            assert any(r["end"] - r["start"] == nbytes and r["dtype"] == torch.uint8 for r in A.regions), "the workspace did not come from the arena"
        return {"mul": mul}

    def gate(outs):
        assert _rel(outs["mul"], want) <= 1e-4
    try:
        contract(monkeypatch, case, dict(vec=vec, mat=canon, scales=scales, zeros=zeros, bias=bias), gate=gate, prepare=ops.vecquant_forget, min_regions=2)
    finally:
        ops.vecquant_forget()


# ------------------------------------------------------------------------------------------------------------------------ K3
def _op(n, seed, blocked=False):
    from quip_amd import ops, method
    np.random.seed(seed)
    torch.manual_seed(seed)
    gen = method.gen_rand_ortho_butterfly if blocked else method.gen_rand_ortho_butterfly_noblock
    return ops.OrthoOp(gen(n), DEV)


ROWS = [1, 5, 16, 17]


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("n,blocked", [(2048, True), (11008, False), (1536, False)])
def test_ortho_apply_rows_general_launches(monkeypatch, ops, n, blocked, transpose, rows):
    """quipamd_ortho_apply_rows: its fp32 workspace of 16 * ceil(rows / 16) rows comes from the wrapper (ops.BIGP_ROWS forced to 0 keeps the
    p x 16 operator on the general path)"""
    op = _op(n, n + rows, blocked)
    g = torch.Generator().manual_seed(rows)
    x = torch.randn(rows, n, generator=g).to(DEV)
    x16 = x.half()
    cs = (0.5 + torch.rand(n, generator=g)).to(DEV)
    bias = torch.randn(n, generator=g).to(DEV)
    monkeypatch.setattr(ops, "BIGP_ROWS", 0)
    monkeypatch.setattr(op, "small_ok", False)

    def case(A):
        return {"f32": op.apply_rows(x, transpose=transpose, bias=bias), "f16_to_bf16": op.apply_rows(x16, transpose=transpose, colscale=cs, out_dtype=BF16),
                "cols": op.apply_cols(x.t().contiguous(), transpose=transpose)}
    contract(monkeypatch, case, dict(x=x, x16=x16, cs=cs, bias=bias), min_regions=6)
    assert "quipamd_ortho_apply_rows" in G.LEDGER


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("n", [1024, 2048, 8192])
def test_ortho_small_launches(monkeypatch, ops, n, transpose, rows):
    """quipamd_ortho_apply_small (direct), quipamd_ortho_apply_small_ops (fp32 and split-bf16 factors, the two operand sets of a decode step)"""
    from quip_amd import _lib
    op = _op(n, n + rows)
    g = torch.Generator().manual_seed(rows)
    x = torch.randn(rows, n, generator=g).to(DEV)
    x16 = x.half()
    cs = (0.5 + torch.rand(n, generator=g)).to(DEV)
    bias = torch.randn(n, generator=g).to(DEV)
    res = torch.randn(rows, n + 12, generator=g).to(DEV).half()[:, :n]       # the residual shares the output's leading dimension (header)
    M0, M1 = op._M[transpose]
    ld, st = (op.pout, op.inv_pin) if transpose else (op.inv_pin, op.pout)

    def case(A):
        direct = A.take((rows, n), F32, name="direct")
        _lib.call("quipamd_ortho_apply_small", ops._p(M0), ops._p(M1), ops._p(ld), ops._p(st), op.p, op.q, int(transpose), ops._p(cs), ops._p(bias),
                  ops._p(x), 0, n, ops._p(direct), 0, n, rows, ops._stream())
        v = A.take((rows, n + 8), BF16, name="v")                         # ldo = n + 8: strided windows as outs
        u = A.take((rows, n + 12), F16, name="u")
        ops.ortho_small_ops([op.small_op(x16, v[:, :n], transpose=transpose, colscale=cs)], rows)
        ops.ortho_small_ops([op.small_op(x, u[:, :n], transpose=transpose, bias=bias, residual=res, relu=True)], rows)
        return {"direct": direct, "v": v, "u": u}
    w = PARTIAL["ortho_apply_small_ops out [rows, ldo]"][1](n)
    contract(monkeypatch, case, dict(x=x, x16=x16, cs=cs, bias=bias, res=res, M0=M0, M1=M1), partial={"v": w, "u": w})


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("n", [2048, 4096, 8192])
def test_ortho_tile_launches(monkeypatch, ops, n, transpose, rows):
    """quipamd_ortho_apply_tiles: three operators in one launch (with LayerNorm) and the output side with residual + relu; strided outputs"""
    opsl = [_op(n, n + rows + i) for i in range(3)]
    g = torch.Generator().manual_seed(rows)
    x = torch.randn(rows, n, generator=g).to(DEV)
    x16 = x.half()
    cs = (0.5 + torch.rand(n, generator=g)).to(DEV)
    bias = torch.randn(n, generator=g).to(DEV)
    res = torch.randn(rows, n, generator=g).to(DEV).half()
    gam, bet = (1 + 0.1 * torch.randn(n, generator=g)).to(DEV).half(), (0.1 * torch.randn(n, generator=g)).to(DEV).half()

    def case(A):
        vs = [A.take((rows, n + 8), BF16, name=f"v{i}", stride=(n + 8, 1)) for i in range(3)]
        ops.ortho_tile_ops([o.small_op(x16, v[:, :n], transpose=transpose, colscale=cs, ln=(gam, bet, 1e-5)) for o, v in zip(opsl, vs)],
                           [o.store_inv(transpose) for o in opsl], rows)
        u = A.take((rows, n), F16, name="u")
        ops.ortho_tile_ops([opsl[0].small_op(x, u, transpose=transpose, bias=bias, residual=res, relu=True)], [opsl[0].store_inv(transpose)], rows)
        return dict({f"v{i}": v for i, v in enumerate(vs)}, u=u)
    contract(monkeypatch, case, dict(x=x, x16=x16, cs=cs, bias=bias, res=res, gam=gam, bet=bet), partial={f"v{i}": PARTIAL["ortho_apply_tiles out [rows, ldo]"][1](n) for i in range(3)})


@pytest.mark.parametrize("rows", ROWS + [40])
@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("n", [11008, 1280])
def test_ortho_bigp_launches(monkeypatch, ops, n, transpose, rows):
    """quipamd_ortho_apply_bigp: activation side (also with silu(gate) * up on load), output side with residual + relu"""
    op = _op(n, n % 97 + rows)
    assert op.bigp_ok and (op.p, op.q) == (n // 16, 16)
    g = torch.Generator().manual_seed(rows)
    x = torch.randn(rows, n, generator=g).to(DEV)
    x16, up = x.half(), torch.randn(rows, n, generator=g).to(DEV).half()
    cs = (0.5 + torch.rand(n, generator=g)).to(DEV)
    bias = torch.randn(n, generator=g).to(DEV)
    res = torch.randn(rows, n, generator=g).to(DEV).half()

    def case(A):
        v, gated, u = A.take((rows, n), F32, name="v"), A.take((rows, n), BF16, name="gated"), A.take((rows, n), F16, name="u")
        inv = [op.store_inv(transpose)]
        ops.ortho_bigp_ops([op.small_op(x16, v, transpose=transpose, colscale=cs)], inv, rows)
        ops.ortho_bigp_ops([op.small_op(x16, gated, transpose=transpose, colscale=cs, residual=up, relu=True)], inv, rows)
        ops.ortho_bigp_ops([op.small_op(x, u, transpose=transpose, bias=bias, residual=res, relu=True)], inv, rows)
        return {"v": v, "gated": gated, "u": u}
    contract(monkeypatch, case, dict(x=x, x16=x16, up=up, cs=cs, bias=bias, res=res))


@pytest.mark.parametrize("rows", ROWS + [64])
@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("fused_form", [True, False], ids=["one-launch", "two-launch"])
@pytest.mark.parametrize("n", [2048, 1536])
def test_ortho_blocked_launches(monkeypatch, ops, n, fused_form, transpose, rows):
    """csrc/ortho_blk.hip: quipamd_ortho_blocked_rows (direct, a workspace of exactly rows * n floats) and the multi call through
    apply_rows_blocked / ortho_blocked_multi (its workspace of len(entries) * rows * n floats), one-launch and two-launch forms"""
    from quip_amd import _lib
    opsl = [_op(n, n + rows + i, blocked=True) for i in range(3)]
    assert all(o.blk_ok for o in opsl)
    g = torch.Generator().manual_seed(rows)
    x = torch.randn(rows, n, generator=g).to(DEV).half()
    up = torch.randn(rows, n, generator=g).to(DEV).half()
    y = torch.randn(rows, n, generator=g).to(DEV)
    cs = (0.5 + torch.rand(n, generator=g)).to(DEV)
    bias = torch.randn(n, generator=g).to(DEV)
    res = torch.randn(rows, n, generator=g).to(DEV).half()
    gam = (1 + 0.1 * torch.randn(n, generator=g)).to(DEV).half()

    def case(A):
        ops.ortho_blocked_config(True if fused_form else 0, 64 if fused_form else 0)
        try:
            one = A.take((rows, n), F16, name="one")
            ws = A.take(rows * n, F32, name="workspace")
            desc, keep = opsl[0].blk_desc(x, one, transpose=transpose, colscale=cs, gate_up=up)
            _lib.call("quipamd_ortho_blocked_rows", ctypes.byref(desc), ops._p(ws), ops._stream())
            three = ops.ortho_blocked_multi([(o, x, dict(transpose=transpose, colscale=cs, ln=(gam, None, 1e-5))) for o in opsl], F16)
            u = opsl[0].apply_rows_blocked(y, transpose=transpose, out_dtype=F16, bias=bias, residual=res, relu=True)
            fast = opsl[1].apply_rows(x, transpose=transpose, fast16=True)
        finally:
            ops.ortho_blocked_config()
        return dict({f"three{i}": t for i, t in enumerate(three)}, one=one, u=u, fast=fast)
    contract(monkeypatch, case, dict(x=x, up=up, y=y, cs=cs, bias=bias, res=res, gam=gam), min_regions=9)


# ---- packed layers: the multi-launch stages of quip_amd.quant ---------------------------------------------------------------------
_LAYERS = {}


def _layer(d, m, seed, bias=True, bits=2):
    """a packed layer with random Kronecker operators (tests/test_gpu_decode_fused.py builds them), one per (shape, seed) for the module.
    What a layer derives lazily (decode-order codes, scratch, pair tables) lands where its first use runs: cases that want it inside the
    bands pass prepare=_fresh(...), which drops it before every run and after the last (no cached view pins an arena)."""
    from test_gpu_decode_fused import _layer as build
    key = (d, m, seed, bias, bits)
    if key not in _LAYERS:
        _LAYERS[key] = build(d, m, seed, bias=bias, bits=bits)
    return _LAYERS[key]


def _fresh(*qls):
    """forget what a layer derived under an earlier arena (decode-order codes, scratch buffers, pair tables): the next run rebuilds them"""
    def prepare():
        for q in qls:
            q._drop_derived()
    return prepare


def _layer_inputs(*qls):
    out = {}
    for i, q in enumerate(qls):
        out.update({f"qweight{i}": q.qweight, f"scales{i}": q.scales, f"bias{i}": q.bias, f"inv_scaleWH{i}": q.inv_scaleWH})
    return out


class _LN(torch.nn.Module):
    def __init__(self, g, b, eps):
        super().__init__()
        self.weight, self.bias, self.eps = g, b, eps


class _RMS(torch.nn.Module):
    def __init__(self, g, eps):
        super().__init__()
        self.weight, self.variance_epsilon = g, eps


def _norms(d, seed):
    g = torch.Generator().manual_seed(seed)
    gam, bet = (1 + 0.1 * torch.randn(d, generator=g)).to(DEV).half(), (0.05 * torch.randn(d, generator=g)).to(DEV).half()
    return {"ln": _LN(gam, bet, 1e-5), "rms": _RMS(gam, 1e-5), None: None}, gam, bet


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("d", [2048, 4096])
def test_three_launch_stages_chain_and_operator_fused_gemm(monkeypatch, rows, d):
    """quant.packed_forward_fused (operator / grouped GEMM / operator), packed_u_then_v (quipamd_ortho_apply_small_chain) and
    packed_vgemm_stage (quipamd_dequant_gemm_vop; d = 2048, <= 8 rows)"""
    from quip_amd import quant
    qls = [_layer(d, d, 300 + i)[0] for i in range(3)]
    norms, gam, bet = _norms(d, rows)
    g = torch.Generator().manual_seed(rows + d)
    x = torch.randn(rows, d, generator=g).to(DEV).half()
    y = torch.randn(rows, d, generator=g).to(DEV)
    res = torch.randn(rows, d, generator=g).to(DEV).half()

    def case(A):
        out = {}
        for i, o in enumerate(quant.packed_forward_fused(qls, x, ln=norms["ln"], residual=res)):
            out[f"fwd{i}"] = o
        t, xts = quant.packed_u_then_v(qls[0], y, F16, qls[1:], residual=res, relu=True, ln=norms["rms"])
        out.update(t=t, xt0=xts[0], xt1=xts[1])
        if quant.vgemm_fusable(qls, rows):
            for i, o in enumerate(quant.packed_vgemm_stage(qls, x, ln=norms["ln"])):
                out[f"vgemm{i}"] = o
        return out
    ref, _ = contract(monkeypatch, case, dict(_layer_inputs(*qls), x=x, y=y, res=res, gam=gam, bet=bet), modules=("ops", "quant"), prepare=_fresh(*qls),
                      min_regions=9)
    assert ("vgemm0" in ref) == (d == 2048 and rows <= 8)


# ------------------------------------------------------------------------------------------------------------------------ K4 / K8 and preprocessing
def _spd(d, seed):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(2 * d + 8, d, generator=g, dtype=torch.float64) * torch.arange(1, d + 1, dtype=torch.float64) ** -0.5
    H = X.T @ X / X.shape[0]
    return (H + 0.01 * H.diagonal().mean() * torch.eye(d, dtype=torch.float64)).float().to(DEV).contiguous()


RAGGED = [(16, 5), (400, 37)]             # d a multiple of 16 (the smallest; one that is no multiple of the 128-column lazy block), m no multiple of 16


@pytest.mark.parametrize("d,m", RAGGED)
def test_ldlq_rounders(monkeypatch, ops, d, m):
    H = _spd(d, d + m)
    LT = ops.cholesky_lt(H)
    C = torch.linalg.cholesky(H.double()).float().contiguous()
    g = torch.Generator().manual_seed(d)
    Wg = (torch.rand(m, d, generator=g) * 3.6 - 0.3).clamp(0, 3).to(DEV)
    eta = torch.rand(m, d, generator=g).to(DEV)
    sH = torch.randn(m, d, generator=g).to(DEV)
    Hn = H / H.diagonal().max()
    negH = (-torch.triu(Hn, 1)).contiguous()
    hdiag = Hn.diagonal().contiguous()

    def case(A):
        out = {"unit_lower_t": ops.unit_lower_t(C)}
        out["codes"], out["err"] = ops.ldlq_round(Wg, LT, 2, return_err=True)
        out["codes_eta"], out["err_eta"] = ops.ldlq_round(Wg, LT, 4, eta=eta, return_err=True)
        out["greedy"], out["eps"] = ops.ldlq_greedy_pass(Wg, sH, negH, hdiag)
        return out
    contract(monkeypatch, case, dict(H=H, LT=LT, C=C, Wg=Wg, eta=eta, sH=sH, negH=negH, hdiag=hdiag), min_regions=7)


@pytest.mark.parametrize("row_groups", [1, 2])
def test_ldlq_round_forced_row_groups(monkeypatch, ops, row_groups):
    d, m = 400, 37
    LT = ops.cholesky_lt(_spd(d, 3))
    Wg = (torch.rand(m, d, generator=torch.Generator().manual_seed(1)) * 3.6 - 0.3).clamp(0, 3).to(DEV)

    def case(A):
        ops.ldlq_config(row_groups)
        try:
            codes, err = ops.ldlq_round(Wg, LT, 2, return_err=True)
        finally:
            ops.ldlq_config(0)
        return {"codes": codes, "err": err}
    contract(monkeypatch, case, dict(LT=LT, Wg=Wg), min_regions=2)


@pytest.mark.parametrize("d,m", RAGGED)
def test_gptq_rounders_feedback_and_inverse(monkeypatch, ops, d, m):
    from quip_amd import _lib
    H = _spd(d, 2 * d + m)
    g = torch.Generator().manual_seed(d + 1)
    W = (0.02 * torch.randn(m, d, generator=g)).to(DEV)
    Wg = (torch.rand(m, d, generator=g) * 3.6 - 0.3).to(DEV)
    scale = (0.01 + 0.005 * torch.rand(m, generator=g)).to(DEV)
    zero = torch.full((m,), 2.0, device=DEV)
    N = torch.triu(torch.randn(d, d, generator=g), 1).to(DEV).contiguous() * 0.05
    FT0 = ops.gptq_feedback(H)

    def case(A):
        out = {"FT": ops.gptq_feedback(H), "inverse": ops.unit_upper_inverse(N)}
        X, work = A.take((d, d), F32, name="X"), A.take((d, d), F32, name="work")          # the C entry point itself: X not zeroed by a wrapper
        _lib.call("quipamd_unit_upper_inverse", ops._p(N), ops._p(X), ops._p(work), d, ops._stream())
        out["X"] = X
        out["codes"], out["err"] = ops.gptq_round(Wg, None, 2, return_err=True, FT=FT0)
        out["Qg"], out["scale_g"], out["zero_g"], out["codes_g"] = ops.gptq_round_groups(W, None, 4, groupsize=16, return_codes=True, FT=FT0)
        out["Qr"], out["scale_r"], out["zero_r"] = ops.gptq_round_groups(W, None, 2, groupsize=-1, qfn="c", scale=scale, zero=zero, FT=FT0)
        return out
    ref, _ = contract(monkeypatch, case, dict(H=H, W=W, Wg=Wg, scale=scale, zero=zero, N=N, FT0=FT0), min_regions=12,
                      partial={"X": PARTIAL["unit_upper_inverse X [d, d]"][1]})
    assert G.bit_equal(ref["FT"], FT0) and G.bit_equal(ref["scale_r"], scale)
    assert torch.equal(torch.triu(ref["X"]), ref["inverse"]) and float(torch.tril(ref["inverse"], -1).abs().max()) == 0.0


@own_time_limit
@pytest.mark.parametrize("m,d,bits", [(40, 384, 2), (24, 128, 4), (37, 400, 2), (48, 80, 3)])
def test_gptq_round_qfnb_with_a_workspace_of_exactly_the_queried_bytes(monkeypatch, ops, m, d, bits):
    """the wrapper hands the sweep a torch.empty workspace of quipamd_gptq_qfnb_workspace_bytes: arbitrary contents are the contract (0xFF and
    0x00 here), the info word lives inside it, and a wrong assumption ends as an error code behind the bounded poll, not a hang"""
    from quip_amd import _lib
    H = _spd(d, 5 * d + m)
    FT = ops.gptq_feedback(H)
    W = (0.02 * torch.randn(m, d, generator=torch.Generator().manual_seed(m))).to(DEV)
    lib = _lib.load()
    nbytes, off = int(lib.quipamd_gptq_qfnb_workspace_bytes(m, d)), int(lib.quipamd_gptq_qfnb_info_offset(m, d))
    assert 0 <= off and off + 4 <= nbytes

    def case(A):
        Q, cs = ops.gptq_round_qfnb(W, FT, bits)
        if not isinstance(A, Plain):
            assert any(r["end"] - r["start"] == nbytes and r["dtype"] == torch.uint8 for r in A.regions), "the workspace did not come from the arena"
        return {"Q": Q, "colscale": cs}
    contract(monkeypatch, case, dict(W=W, FT=FT), min_regions=3)


CHOLESKY_CONFIGS = [dict(), dict(old_syrk=True), dict(unblocked_diag=True), dict(old_syrk=True, unblocked_diag=True), dict(lookahead=True), dict(lookahead=False)]


@pytest.mark.parametrize("cfg", CHOLESKY_CONFIGS, ids=lambda c: "-".join(f"{k}={v}" for k, v in c.items()) or "default")
@pytest.mark.parametrize("d", [16, 203, 1100])                           # 203, 1100: no multiples of 16 (1100: the two-stream schedule from d = 1024)
def test_cholesky_lt_in_each_config(monkeypatch, ops, d, cfg):
    H = _spd(d, d)

    def case(A):
        ops.cholesky_config(**cfg)
        try:
            return {"LT": ops.cholesky_lt(H)}
        finally:
            ops.cholesky_config()
    ref, _ = contract(monkeypatch, case, dict(H=H), min_regions=2)
    L = torch.linalg.cholesky(H.double())
    want = torch.triu((L / L.diagonal()[None, :]).T, 1)
    assert float((ref["LT"].double() - want).abs().max()) <= 1e-3 * float(want.abs().max())


@pytest.mark.parametrize("dtype", [F16, BF16, F32])
@pytest.mark.parametrize("tokens,d", [(1, 16), (37, 96), (130, 203), (300, 520)])
def test_hessian_accum_and_finish(monkeypatch, ops, dtype, tokens, d):
    """tokens no multiple of 128, d no multiple of 16, a strided x; the fast variant with a workspace of exactly quipamd_hessian_fast_workspace"""
    from quip_amd import _lib
    g = torch.Generator().manual_seed(tokens + d)
    buf = (torch.randn(tokens, d + 24, generator=g)).to(dtype).to(DEV)
    x, xs = buf[:, :d].contiguous(), buf[:, 8:8 + d]
    fast = dtype != F32
    nws = int(_lib.load().quipamd_hessian_fast_workspace(tokens, d)) if fast else 0

    def case(A):
        Hacc = A.take((d, d), torch.float64, fill=0, name="Hacc")
        ops.hessian_accum(Hacc, x)
        ops.hessian_accum(Hacc, xs)
        out = {"Hacc": Hacc, "H": ops.hessian_finish(Hacc, 2 * tokens)}
        if fast:
            Hf = A.take((d, d), torch.float64, fill=0, name="Hacc_fast")
            ops.hessian_accum(Hf, xs, fast=True)
            ops.hessian_accum(Hf, x, fast=True)
            out["Hacc_fast"] = Hf
            if not isinstance(A, Plain):
                assert any(r["end"] - r["start"] == nws * x.element_size() for r in A.regions), "the fast workspace did not come from the arena"
        return out
    ref, runs = contract(monkeypatch, case, dict(buf=buf, x=x), min_regions=4 if fast else 2)
    # Hacc is zero-initialised by contract, so it is carved with zeros and an unwritten tile INSIDE the triangle shows only through the values
    # (the fp64 comparison below, bit equality of the guarded runs).  The kernel tiles by 64 or by 128 columns: the mask is the 128-column
    # rule for both, because what is above the 128-block triangle is above the 64-block one too (the upper half of a diagonal 128-block is
    # written with one tile and not with the other, and is asserted neither way).
    written = PARTIAL["hessian_accum Hacc [d, d]"][1]
    for out in [ref] + runs:                       # Hacc is the caller's (zero-initialised by contract): above the block-lower triangle it still holds the zeros
        for name in ("Hacc", "Hacc_fast"):
            if name in out and d > 128:
                assert float(out[name][~written(out[name])].abs().max()) == 0.0 and float(out[name][written(out[name])].abs().max()) > 0.0
    want = (x.double().T @ x.double() + xs.double().T @ xs.double())
    lo = torch.tril(torch.ones(d, d, dtype=torch.bool, device=DEV))
    assert float((ref["Hacc"] - want)[lo].abs().max()) <= 1e-12 * float(want.abs().max())


@pytest.mark.parametrize("m,d,dtype", [(300, 130, F32), (37, 203, F16), (64, 16, BF16), (2048, 2048, F16)])
def test_preproc_chains_with_workspaces_of_exactly_the_queried_bytes(monkeypatch, ops, m, d, dtype):
    from quip_amd import _lib
    torch.manual_seed(m + d)
    w0 = (0.02 * torch.randn(m, d, device=DEV) * (0.2 + torch.rand(d, device=DEV))).to(dtype)
    H0 = _spd(d, m)
    nbytes = int(_lib.load().quipamd_preproc_workspace_bytes(m, d))

    def case(A):
        w, H, H2 = A.copy_of(w0, name="w"), A.copy_of(H0, name="H"), A.copy_of(H0, name="H2")
        s = ops.preproc_rescale(w, H)
        ops.preproc_trace_ridge(H2, 1e-2)
        if not isinstance(A, Plain):
            assert any(r["end"] - r["start"] == nbytes and r["dtype"] == torch.uint8 for r in A.regions), "the workspace did not come from the arena"
        return {"w": w, "H": H, "s": s, "H2": H2}
    ref, _ = contract(monkeypatch, case, dict(w0=w0, H0=H0), min_regions=6)
    want = H0 * (d / (torch.trace(H0) + 1e-8)) + 1e-2 * torch.eye(d, device=DEV)
    assert float((ref["H2"] - want).abs().max()) <= 2e-6 * float(want.abs().max())


# ------------------------------------------------------------------------------------------------------------------------ decode launches
@pytest.mark.parametrize("d,m,groups,has_u,norm,relu,residual,bs", [
    (2048, 2048, 3, False, "ln", False, False, 1), (2048, 2048, 3, True, "ln", False, True, 1), (2048, 2048, 1, False, None, False, False, 2),
    (2048, 8192, 1, True, "ln", False, True, 4), (8192, 2048, 1, True, None, True, False, 1), (8192, 2048, 1, True, None, True, False, 3),
    (4096, 4096, 3, True, "rms", False, True, 1), (4096, 4096, 2, True, "rms", False, True, 2),
    # ops_only: the prologue as its own launch (one workgroup per row) + the grouped dequant-GEMM
    (2048, 2048, 3, False, "ln", False, False, 16), (2048, 2048, 3, True, "ln", False, True, 5), (2048, 8192, 1, True, "ln", False, True, 16),
    (8192, 2048, 1, True, None, True, False, 16), (4096, 4096, 3, True, "rms", False, True, 16), (4096, 4096, 2, True, "rms", False, True, 5)])
def test_decode_fused_gemm(monkeypatch, d, m, groups, has_u, norm, relu, residual, bs):
    """quant.fused_stage: 1, 2, 3 groups, with the U prologue and t_out, fp32 and fp16 y, the layer-pair form (d = 8192, <= 2 rows), ops_only"""
    from quip_amd import quant
    qls = [_layer(d, m, 100 + 7 * i + d % 97)[0] for i in range(groups)]
    prev = _layer(2048 if d == 8192 else d, d, 55)[0] if has_u else None
    norms, gam, bet = _norms(d, bs)
    assert quant.fused_ok(qls, bs, prev=prev, norm=norm is not None, residual=residual)
    g = torch.Generator().manual_seed(d + m + bs)
    x = torch.randn(bs, d, generator=g).to(DEV).half()
    y_prev = (torch.randn(bs, d, generator=g) * 0.5).to(DEV).half()
    res = torch.randn(bs, d, generator=g).to(DEV).half() if residual else None
    layers = qls + ([prev] if prev is not None else [])

    def case(A):
        out = {}
        if has_u:
            ys, t = quant.fused_stage(qls, prev=prev, y_prev=y_prev, residual=res, relu=relu, ln=norms[norm], store=True)
            ys16, _ = quant.fused_stage(qls, prev=prev, y_prev=y_prev, residual=res, relu=relu, ln=norms[norm], store=False, y_dtype=F16)
            out["t"] = t
        else:
            ys, _ = quant.fused_stage(qls, x=x, ln=norms[norm])
            ys16, _ = quant.fused_stage(qls, x=x, ln=norms[norm], y_dtype=F16)
        for i, (a, b) in enumerate(zip(ys, ys16)):
            out[f"y{i}"], out[f"y16_{i}"] = a, b
        return out
    contract(monkeypatch, case, dict(_layer_inputs(*layers), x=x, y_prev=y_prev, res=res, gam=gam, bet=bet), modules=("ops", "quant"),
             prepare=_fresh(*layers), min_regions=2 * groups)


@pytest.mark.parametrize("d,m,groups,norm,relu,residual,bs", [
    (2048, 2048, 3, "ln", False, True, 1), (2048, 8192, 1, "ln", False, True, 2), (4096, 4096, 2, "rms", False, True, 4), (8192, 2048, 1, None, True, False, 2),
    (2048, 2048, 3, "ln", False, True, 5), (4096, 4096, 3, "rms", False, True, 16), (8192, 2048, 1, None, True, False, 16)])
def test_decode_fused_gemm_with_a_strided_t_out(monkeypatch, ops, d, m, groups, norm, relu, residual, bs):
    """quipamd_decode_fused_gemm called directly with t_out a window of a [bs, d + 8] carve (ld_t = d + 8), in both prologue forms: the single
    launch (<= 4 rows) and ops_only (one workgroup per row).  The padding columns keep the fill, the window equals the contiguous t bit for bit."""
    from quip_amd import quant
    qls = [_layer(d, m, 100 + 7 * i + d % 97)[0] for i in range(groups)]
    prev = _layer(2048 if d == 8192 else d, d, 55)[0]
    norms, gam, bet = _norms(d, bs)
    assert quant.fused_ok(qls, bs, prev=prev, norm=norm is not None, residual=residual)
    g = torch.Generator().manual_seed(d + m + bs)
    y_prev = (torch.randn(bs, d, generator=g) * 0.5).to(DEV).half()
    res = torch.randn(bs, d + 16, generator=g).to(DEV).half()[:, :d] if residual else None          # a strided residual beside it
    ops_only = bs > ops.FUSED_MAX_ROWS
    layers = qls + [prev]
    for q in layers:
        q._drop_derived()
    kw = dict(V=[q.V.fop(False) for q in qls], colscale=[q.inv_scaleWH for q in qls], qweight=[q.decode_qweight() for q in qls],
              scale=[q.scales for q in qls], m=m, bs=bs, bits=2, ops_only=ops_only, U=prev.U.fop(True), u_y=y_prev, u_bias=quant.bias16(prev),
              u_residual=res, u_relu=relu)
    lnp = quant._ln_params(norms[norm])
    if lnp is not None:
        kw.update(norm=1 if lnp[1] is not None else 2, ln_gamma=lnp[0], ln_beta=lnp[1], ln_eps=lnp[2])

    def case(A):
        shape, dt = ((bs, d), F16) if ops_only else ((bs, m), F32)
        ys, ys2 = [A.take(shape, dt, name=f"y{i}") for i in range(groups)], [A.take(shape, dt, name=f"y{i}_contiguous_t") for i in range(groups)]
        t, tc = A.take((bs, d + 8), F16, name="t_out"), A.take((bs, d), F16, name="t_contiguous")
        ops.decode_fused_gemm(y=ys, t_out=t[:, :d], **kw)
        ops.decode_fused_gemm(y=ys2, t_out=tc, **kw)
        return dict({f"y{i}": y for i, y in enumerate(ys)}, **{f"y{i}_c": y for i, y in enumerate(ys2)}, t=t, tc=tc)
    ins = dict(_layer_inputs(*layers), y_prev=y_prev, res=res, gam=gam, bet=bet, **{f"qd{i}": w for i, w in enumerate(kw["qweight"])})
    ref, runs = contract(monkeypatch, case, ins, partial={"t": PARTIAL["decode_fused_gemm t_out [bs, ld_t]"][1](d)})
    for out in [ref] + runs:
        assert G.bit_equal(out["t"][:, :d].contiguous(), out["tc"]) and all(G.bit_equal(out[f"y{i}"], out[f"y{i}_c"]) for i in range(groups))
    for q in layers:
        q._drop_derived()


@pytest.mark.parametrize("ffn,h,rows", [(1792, 1024, 1), (1792, 1024, 5), (1792, 1024, 16), (11008, 4096, 4), (11008, 4096, 13)])
def test_decode_bigp_launches(monkeypatch, ops, ffn, h, rows):
    """quipamd_decode_bigp_u with `clear` and strided outs, quipamd_decode_bigp_v_gemm in its three forms; the atomics form
    (NONDETERMINISTIC) is held to the 3e-3 gate of test_gpu_decode_bigp.py against the fp64 chain, the other two to bit equality.  (The
    decode-order codes and the tail tables are built beforehand, on ordinary memory: here they are inputs, frozen like the others.)"""
    from quip_amd.quant import _bigp_tail_tables
    from test_gpu_decode_fused import _dense
    gate_l, up_l = _layer(h, ffn, 900 + rows, bias=True)[0], _layer(h, ffn, 901 + rows, bias=False)[0]
    down, What = _layer(ffn, h, 902 + rows, bias=False)
    V = down.V
    g = torch.Generator().manual_seed(ffn + rows)
    yg, yu = torch.randn(rows, ffn, generator=g).to(DEV).half(), torch.randn(rows, ffn, generator=g).to(DEV).half()
    gi = torch.randn(rows, ffn, generator=g).to(DEV).half()
    ui = (torch.randn(rows, ffn, generator=g).to(DEV) * down.inv_scaleWH).half()
    tabs = _bigp_tail_tables([gate_l, up_l], down)
    qd = down.decode_qweight()
    inv_pin = torch.arange(V.n, device=DEV) if V.inv_pin is None else V.inv_pin.long()
    timg = (inv_pin % 16) * V.p + inv_pin // 16
    gnat, unat = gi[:, timg], ui[:, timg]                                # gi / ui are transposed images: natural element k sits at timg[k]
    t = (torch.nn.functional.silu(gnat.float()).half().float() * unat.float()).half().double()
    want = (t @ _dense(V).t()) @ What.t()
    zt_y, zt_u = gate_l.to_zt(yg), up_l.to_zt(yu)

    def case(A):
        imgs = A.take((2, rows, ffn + 8), F16, name="imgs")              # ld_out = ffn + 8: every `out` is a strided window
        clear = A.take((rows, h), F32, fill=7.0, name="clear")
        ops.decode_bigp_u([(q.U, y, b_, p_, d_, imgs[i][:, :ffn]) for i, (q, y, (d_, b_, p_)) in enumerate(zip((gate_l, up_l), (zt_y, zt_u), tabs))], rows, clear=clear)
        partials = A.take((V.p // 16, rows, h), F32, name="partials")
        y_fixed, y_two = A.take((rows, h), F32, name="y_fixed"), A.take((rows, h), F32, name="y_two")
        xt = A.take((rows, ffn), F16, name="xt")
        ops.decode_bigp_v_gemm(V, gi, ui, qd, down.scales, y_fixed, partials=partials)
        ops.decode_bigp_v_gemm(V, gi, ui, qd, down.scales, y_two, xt=xt)
        return {"imgs": imgs, "clear": clear, "partials": partials, "y_fixed": y_fixed, "y_two": y_two, "xt": xt}
    ins = dict(_layer_inputs(gate_l, up_l, down), zt_y=zt_y, zt_u=zt_u, gi=gi, ui=ui, qd=qd)
    ref, _ = contract(monkeypatch, case, ins, arena_mb=512, partial={"imgs": PARTIAL["decode_bigp_u out [rows, ld_out]"][1](ffn)})
    dense = torch.empty((2, rows, ffn), dtype=F16, device=DEV)          # the same launch on contiguous outs: the same bits
    ops.decode_bigp_u([(q.U, y, b_, p_, d_, dense[i]) for i, (q, y, (d_, b_, p_)) in enumerate(zip((gate_l, up_l), (zt_y, zt_u), tabs))], rows)
    assert G.bit_equal(ref["imgs"][:, :, :ffn].contiguous(), dense)
    assert float(ref["clear"].abs().max()) == 0.0
    assert _rel(down.from_zt(ref["y_fixed"]), want) <= 3e-3 and _rel(down.from_zt(ref["y_two"]), want) <= 3e-3

    def atomics(A):
        y = A.take((rows, h), F32, fill=0, name="y")
        ops.decode_bigp_v_gemm(V, gi, ui, qd, down.scales, y)
        return {"y": y}

    def gate(outs):
        assert _rel(down.from_zt(outs["y"]), want) <= 3e-3
    contract(monkeypatch, atomics, ins, gate=gate)


@pytest.mark.parametrize("rows", [1, 2, 5, 16])
def test_fused_bigp_tail_chain(monkeypatch, rows):
    """quant.fused_bigp_tail: its images, accumulator and scratch allocated by the wrapper; the atomics form below two_launch_from rows"""
    from quip_amd import quant
    h, ffn = 1024, 1792
    gate_l, up_l, down = _layer(h, ffn, 40, bias=False)[0], _layer(h, ffn, 41, bias=False)[0], _layer(ffn, h, 42, bias=False)[0]
    g = torch.Generator().manual_seed(rows)
    ygu = [torch.randn(rows, ffn, generator=g).to(DEV).half() for _ in range(2)]
    atom = rows < quant.two_launch_from(down)
    ref_holder = {}

    def case(A):
        return {"yd": quant.fused_bigp_tail([gate_l, up_l], down, ygu)}

    def gate(outs):
        ref_holder.setdefault("yd", outs["yd"].clone())
        assert float((outs["yd"] - ref_holder["yd"]).abs().max()) <= 1e-5 * float(ref_holder["yd"].abs().max())     # test_gpu_decode_bigp.py: two runs
    contract(monkeypatch, case, dict(_layer_inputs(gate_l, up_l, down), yg=ygu[0], yu=ygu[1]), modules=("ops", "quant"), gate=gate if atom else None,
             prepare=_fresh(gate_l, up_l, down), min_regions=2)


@pytest.mark.parametrize("n,m_in,relu,residual,bs", [(2048, 8192, False, True, 1), (8192, 2048, True, False, 5), (4096, 4096, False, True, 16)])
def test_decode_u_only(monkeypatch, n, m_in, relu, residual, bs):
    from quip_amd.quant import fused_u_only
    ql = _layer(m_in, n, 900 + n % 11)[0]
    g = torch.Generator().manual_seed(n)
    y = (0.5 * torch.randn(bs, n, generator=g)).to(DEV).half()
    res = torch.randn(bs, n + 8, generator=g).to(DEV).half()[:, :n] if residual else None

    def case(A):
        return {"out": fused_u_only(ql, y, residual=res, relu=relu)}
    contract(monkeypatch, case, dict(_layer_inputs(ql), y=y, res=res), modules=("ops", "quant"), prepare=_fresh(ql))


@pytest.mark.parametrize("n,norm,bs,vocab,y32", [(2048, "ln", 1, 1000, False), (4096, "rms", 4, 777, True), (2048, "rms", 2, 512, True), (4096, "ln", 3, 4099, False)])
def test_decode_head_and_embed_on_strided_buffers(monkeypatch, ops, n, norm, bs, vocab, y32):
    """quipamd_decode_head with strided logits, the 256 partials per row and pos_inc; quipamd_decode_embed with a strided out"""
    from quip_amd.quant import fused_head
    ql = _layer(512, n, 31 + n % 7 + bs, bias=(norm == "ln"))[0]
    norms, gam, bet = _norms(n, vocab)
    g = torch.Generator().manual_seed(vocab + bs)
    W = (0.02 * torch.randn(vocab, n, generator=g)).to(DEV).half()
    y = (torch.randn(bs, n, generator=g) * 0.5).to(DEV)
    y = ql.to_zt(y if y32 else y.half())
    res = torch.randn(bs, n, generator=g).to(DEV).half()
    tok, ptab = (0.02 * torch.randn(vocab, n, generator=g)).to(DEV).half(), (0.02 * torch.randn(64, n, generator=g)).to(DEV).half()
    pos0 = torch.tensor([5], dtype=torch.int64, device=DEV)
    ld = vocab + 9                                                          # rows of the logits do not start on a 16-byte boundary

    def case(A):
        logits = A.take((bs, ld), F16, name="logits")
        pv, pi = A.take((bs, ops.HEAD_PARTS), F32, name="part_val"), A.take((bs, ops.HEAD_PARTS), torch.int32, name="part_idx")
        pos = A.copy_of(pos0, name="pos")
        fused_head(ql, y, res, norms[norm], W, logits[:, :vocab], pv, pi, pos_inc=pos)
        plain = A.take((bs, vocab), F16, name="logits_x")
        ops.decode_head(W, plain, gam, bet if norm == "ln" else None, 1e-5, x=res)
        ids = A.take(bs, torch.int64, fill=3, name="ids")
        xo = A.take((bs, n + 8), F16, name="embed_out")
        ops.decode_embed(tok, ids, xo[:, :n], pos_table=ptab, pos=pos, pos_offset=2, part_val=pv, part_idx=pi)
        first = A.take(bs, torch.int64, name="argmax")
        ops.argmax_rows(logits[:, :vocab], out=first)
        return {"logits": logits, "part_val": pv, "part_idx": pi, "pos": pos, "logits_x": plain, "ids": ids, "embed_out": xo, "argmax": first}
    ref, _ = contract(monkeypatch, case, dict(_layer_inputs(ql), W=W, y=y, res=res, tok=tok, ptab=ptab, pos0=pos0, gam=gam, bet=bet),
                      partial={"logits": PARTIAL["decode_head logits [bs, ld_logits]"][1](vocab), "embed_out": PARTIAL["decode_embed out [bs, ld_out]"][1](n)},
                      prepare=_fresh(ql))
    assert int(ref["pos"]) == 6 and torch.equal(ref["ids"], ref["logits"][:, :vocab].float().argmax(-1)) and torch.equal(ref["ids"], ref["argmax"])
    assert torch.equal(ref["embed_out"][:, :n], tok[ref["ids"]] + ptab[8])


@pytest.mark.parametrize("bs", [1, 5, 16])
@pytest.mark.parametrize("n,vocab", [(2048, 1000), (4096, 777)])
def test_decode_embed_alone_on_a_strided_out(monkeypatch, ops, n, vocab, bs):
    """the embed launch at the engine's batch sizes: with and without a position table, with and without partials"""
    g = torch.Generator().manual_seed(n + bs)
    tok, ptab = (0.02 * torch.randn(vocab, n, generator=g)).to(DEV).half(), (0.02 * torch.randn(16, n, generator=g)).to(DEV).half()
    ids0 = torch.randint(0, vocab, (bs,), generator=g).to(DEV)
    pv0 = torch.randn(bs, ops.HEAD_PARTS, generator=g).to(DEV)
    pi0 = torch.randint(0, vocab, (bs, ops.HEAD_PARTS), generator=g, dtype=torch.int32).to(DEV)
    pos = torch.tensor([13], dtype=torch.int64, device=DEV)                    # + offset 2: the last row of the position table

    def case(A):
        ids_a, ids_b = A.copy_of(ids0, name="ids_a"), A.copy_of(ids0, name="ids_b")
        a, b = A.take((bs, n + 24), F16, name="with_table"), A.take((bs, n), F16, name="plain")
        ops.decode_embed(tok, ids_a, a[:, :n], pos_table=ptab, pos=pos, pos_offset=2, part_val=pv0, part_idx=pi0)
        ops.decode_embed(tok, ids_b, b)
        return {"ids_a": ids_a, "ids_b": ids_b, "with_table": a, "plain": b}
    ref, _ = contract(monkeypatch, case, dict(tok=tok, ptab=ptab, ids0=ids0, pv0=pv0, pi0=pi0, pos=pos), partial={"with_table": PARTIAL["decode_embed out [bs, ld_out]"][1](n)})
    assert torch.equal(ref["ids_b"], ids0) and torch.equal(ref["plain"], tok[ids0])
    want = pi0.long().gather(1, pv0.argmax(1, keepdim=True)).reshape(-1)
    assert torch.equal(ref["ids_a"], want) and torch.equal(ref["with_table"][:, :n], tok[want] + ptab[15])


@pytest.mark.parametrize("dtype", [F16, BF16, F32])
def test_argmax_rows_on_rows_that_do_not_start_on_a_16_byte_boundary(monkeypatch, ops, dtype):
    g = torch.Generator().manual_seed(3)
    y = torch.randn(5, 50283, generator=g).to(dtype).to(DEV)
    v = y[:, 3:50278]
    v[0, 50274] = 60.0
    v[1] = float("-inf")

    def case(A):
        mine = A.take(5, torch.int64, name="out")
        ops.argmax_rows(v, out=mine)
        return {"theirs": ops.argmax_rows(v), "mine": mine, "aligned": ops.argmax_rows(y[:, :50280])}
    ref, _ = contract(monkeypatch, case, dict(y=y), min_regions=3)
    assert torch.equal(ref["mine"], v.float().argmax(-1)) and torch.equal(ref["theirs"], ref["mine"])


def _tables(hd, rows):
    from quip_amd import decode
    inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd))
    cos, sin = decode.rotary_tables(inv, rows)
    return cos.to(DEV).contiguous(), sin.to(DEV).contiguous()


def _cache_arena_mb(cache, copies):
    """MiB for `copies` carved copies of a KV cache: the tensor plus its two bands of 16 leading-dimension slices each"""
    one = cache.numel() * cache.element_size()
    return 96 + int(copies * (one + 2 * max(G.MIN_BAND, 16 * one // cache.shape[0])) / 2 ** 20)


def _only_row_changed(cache, cache0, pos):
    mask = torch.ones(cache.shape[2], dtype=torch.bool, device=DEV)
    mask[pos] = False
    return bool(torch.equal(cache[:, :, mask], cache0[:, :, mask])) and not bool(torch.equal(cache[:, :, pos], cache0[:, :, pos]))


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("bs", [1, 5, 16])
def test_rope_inplace_on_strided_q_and_k(monkeypatch, ops, dtype, bs):
    heads, kvh, hd, maxpos = 8, 4, 128, 64
    cos, sin = _tables(hd, maxpos)
    g = torch.Generator().manual_seed(bs)
    q0 = torch.randn(bs, heads * hd + 16, generator=g).to(dtype).to(DEV)
    k0 = torch.randn(bs, kvh * hd + 8, generator=g).to(dtype).to(DEV)

    def case(A):
        out = {}
        for p in (0, maxpos - 1, maxpos):                                   # the last row of the tables; one past them: a no-op
            q, k = A.copy_of(q0, name=f"q@{p}"), A.copy_of(k0, name=f"k@{p}")
            ops.rope_inplace(q[:, :heads * hd], k[:, :kvh * hd], cos, sin, torch.tensor([p], device=DEV), heads, kvh)
            out[f"q@{p}"], out[f"k@{p}"] = q, k
        return out
    ref, _ = contract(monkeypatch, case, dict(cos=cos, sin=sin, q0=q0, k0=k0))
    assert torch.equal(ref[f"q@{maxpos}"], q0) and torch.equal(ref[f"k@{maxpos}"], k0)
    for p in (0, maxpos - 1):                                               # only the documented part changed: the padding columns keep their bits
        assert torch.equal(ref[f"q@{p}"][:, heads * hd:], q0[:, heads * hd:]) and torch.equal(ref[f"k@{p}"][:, kvh * hd:], k0[:, kvh * hd:])
    assert torch.equal(ref["q@0"], q0) and not torch.equal(ref[f"q@{maxpos - 1}"], q0)      # position 0 is the identity rotation


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("heads,hd,maxlen", [(8, 64, 512), (4, 128, 300)])
@pytest.mark.parametrize("bs", [1, 5, 16])
def test_decode_attention_at_the_first_and_the_last_cache_slot(monkeypatch, ops, dtype, heads, hd, maxlen, bs):
    """the append into the last slot is the store nearest the end of the cache; strided q / k / v make the wrapper's out [bs, ld] strided too"""
    n = heads * hd
    g = torch.Generator().manual_seed(bs + hd)
    mk = lambda *s: torch.randn(*s, generator=g).to(dtype).to(DEV)
    qkv = mk(3, bs, n + 8)
    q, k, v = (qkv[i][:, :n] for i in range(3))
    kc0, vc0 = mk(bs, heads, maxlen, hd), mk(bs, heads, maxlen, hd)

    def case(A):
        out = {}
        for p in (0, maxlen - 1):
            kc, vc = A.copy_of(kc0, name=f"kcache@{p}"), A.copy_of(vc0, name=f"vcache@{p}")
            o = ops.decode_attention(q, k, v, kc, vc, torch.tensor([p], device=DEV))
            out[f"out@{p}"] = o.as_strided((bs, n + 8), (n + 8, 1)) if bs > 1 else o
            out[f"kcache@{p}"], out[f"vcache@{p}"] = kc, vc
            out[f"contig@{p}"] = ops.decode_attention(q.contiguous(), k.contiguous(), v.contiguous(), A.copy_of(kc0), A.copy_of(vc0), torch.tensor([p], device=DEV))
        return out
    partial = {f"out@{p}": PARTIAL["decode_attention out [bs, ld]"][1](n) for p in (0, maxlen - 1)} if bs > 1 else None
    ref, _ = contract(monkeypatch, case, dict(qkv=qkv, kc0=kc0, vc0=vc0), partial=partial, arena_mb=_cache_arena_mb(kc0, 8))
    for p in (0, maxlen - 1):
        assert _only_row_changed(ref[f"kcache@{p}"], kc0, p) and _only_row_changed(ref[f"vcache@{p}"], vc0, p)
        assert torch.equal(ref[f"kcache@{p}"][:, :, p].reshape(bs, n), k) and torch.equal(ref[f"out@{p}"][:, :n], ref[f"contig@{p}"])


@pytest.mark.parametrize("n,heads,hd,rope,maxlen", [(2048, 32, 64, False, 64), (2048, 32, 64, False, 768), (4096, 32, 128, True, 300), (2048, 16, 128, True, 64)])
@pytest.mark.parametrize("bs", [1, 5, 16])
def test_decode_attention_fused(monkeypatch, n, heads, hd, rope, maxlen, bs):
    from quip_amd.quant import fused_attention, fused_attention_ok
    qkv = [_layer(n, n, 700 + i + n % 13)[0] for i in range(3)]
    g = torch.Generator().manual_seed(n + bs)
    kc0 = (0.5 * torch.randn(bs, heads, maxlen, hd, generator=g)).to(DEV).half()
    vc0 = (0.5 * torch.randn(bs, heads, maxlen, hd, generator=g)).to(DEV).half()
    ys = [(0.5 * torch.randn(bs, n, generator=g)).to(DEV).half() for _ in range(3)]
    cos, sin = _tables(hd, maxlen) if rope else (None, None)
    assert fused_attention_ok(qkv, kc0)

    def case(A):
        out = {}
        for p in (0, maxlen - 1):
            kc, vc = A.copy_of(kc0, name=f"kcache@{p}"), A.copy_of(vc0, name=f"vcache@{p}")
            out[f"out@{p}"] = fused_attention(qkv, ys, kc, vc, torch.tensor([p], device=DEV), cos, sin)
            out[f"kcache@{p}"], out[f"vcache@{p}"] = kc, vc
        return out
    ref, _ = contract(monkeypatch, case, dict(_layer_inputs(*qkv), kc0=kc0, vc0=vc0, y0=ys[0], y1=ys[1], y2=ys[2], cos=cos, sin=sin),
                      modules=("ops", "quant"), prepare=_fresh(*qkv), arena_mb=_cache_arena_mb(kc0, 4))
    for p in (0, maxlen - 1):
        assert _only_row_changed(ref[f"kcache@{p}"], kc0, p) and _only_row_changed(ref[f"vcache@{p}"], vc0, p)


@pytest.mark.parametrize("dtype,hd,g,maxlen", [(F16, 128, 4, 512), (BF16, 64, 8, 700), (F16, 64, 2, 256), (F16, 128, 16, 1024)])
@pytest.mark.parametrize("bs", [1, 5, 16])
@own_time_limit
def test_decode_attention_grouped_on_a_workspace_of_exactly_the_queried_bytes(monkeypatch, ops, dtype, hd, g, maxlen, bs):
    """the workspace holds arrival counters the header wants ZERO-FILLED before the first launch and that every launch re-arms: it is carved
    with exactly the queried bytes, zero-filled once, and serves four launches in a row (positions 0, 1, 300 or so, maxlen - 1)"""
    from quip_amd import _lib
    kv = 2
    heads = kv * g
    gen = torch.Generator().manual_seed(hd + g + bs)
    mk = lambda *s: torch.randn(*s, generator=gen).to(dtype).to(DEV)
    q, k, v = mk(bs, heads * hd + 8)[:, :heads * hd], mk(bs, kv * hd + 16)[:, :kv * hd], mk(bs, kv * hd)
    kc0, vc0 = mk(bs, kv, maxlen, hd), mk(bs, kv, maxlen, hd)
    cos, sin = _tables(hd, maxlen)
    nbytes = int(_lib.load().quipamd_decode_attention_grouped_workspace_bytes(bs, heads, kv, hd, maxlen))
    assert (nbytes > 0) == (maxlen > 256)
    positions = [0, 1, min(300, maxlen - 2), maxlen - 1]

    def case(A):
        ws = A.take(max(nbytes, 16), torch.uint8, fill=0, name="workspace")
        kc, vc = A.copy_of(kc0, name="kcache"), A.copy_of(vc0, name="vcache")
        out = {"kcache": kc, "vcache": vc}
        for p in positions:
            out[f"out@{p}"] = ops.decode_attention_grouped(q, k, v, kc, vc, torch.tensor([p], device=DEV), cos, sin, workspace=ws)
        out["own_ws"] = ops.decode_attention_grouped(q, k, v, A.copy_of(kc0), A.copy_of(vc0), torch.tensor([maxlen - 1], device=DEV))
        return out
    ref, _ = contract(monkeypatch, case, dict(q=q, k=k, v=v, kc0=kc0, vc0=vc0, cos=cos, sin=sin), arena_mb=_cache_arena_mb(kc0, 4))
    mask = torch.ones(maxlen, dtype=torch.bool, device=DEV)
    mask[positions] = False
    assert torch.equal(ref["kcache"][:, :, mask], kc0[:, :, mask]) and torch.equal(ref["vcache"][:, :, mask], vc0[:, :, mask])
    assert torch.equal(ref["vcache"][:, :, maxlen - 1].reshape(bs, kv * hd), v)


# ------------------------------------------------------------------------------------------------------------------------ the engine as a whole
def _pack_blocks(dec, names, bits, native3=False, seed=0):
    from quip_amd import ops, method
    from quip_amd.quant import QuantLinear
    np.random.seed(seed)
    torch.manual_seed(seed)
    for blk in dec.blocks:
        for name in names:
            lin = getattr(blk, name)
            m, d = lin.weight.shape
            W = lin.weight.data
            s = ops.qfnb_scale(W)
            _, codes = ops.quantize(W, "b", s, None, 2 ** bits - 1, want_codes=True)
            U = ops.OrthoOp(method.gen_rand_ortho_butterfly_noblock(m), DEV)
            V = ops.OrthoOp(method.gen_rand_ortho_butterfly_noblock(d), DEV)
            ql = QuantLinear(d, m, bits=bits, qfn="b", native3=native3).to(DEV)
            ql.pack(codes, s, None, bias=lin.bias, scaleWH=(0.5 + torch.rand(d)).to(DEV), U=U, V=V)
            setattr(blk, name, ql)


_MODELS = {}


def _model(kind):
    """random packed decoders with small hidden sizes the fused modes accept (as tests/test_gpu_decode_e2e.py / test_gpu_decode_gqa.py use)"""
    from quip_amd import decode
    if kind in _MODELS:
        return _MODELS[kind]
    torch.manual_seed(0)
    nn, h, vocab, maxpos = torch.nn, 2048, 512, 64
    if kind == "opt":
        blocks = [decode.OPTBlock.random(h, 8192, 32, F16) for _ in range(2)]
        dec = decode.OPTDecoder(nn.Embedding(vocab, h, dtype=F16), nn.Embedding(maxpos + 2, h, dtype=F16), blocks, nn.LayerNorm(h, dtype=F16), 32)
        names, bits, native3 = ["q_proj", "k_proj", "v_proj", "out_proj", "fc1", "fc2"], 2, False
    else:
        heads, kvh = 16, 4
        hd = h // heads
        inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd))
        blocks = [decode.LlamaBlock.random(h, 4096, heads, 1e-5, F16, kv_heads=kvh) for _ in range(2)]
        dec = decode.LlamaDecoder(nn.Embedding(vocab, h, dtype=F16), blocks, decode.RMSNorm(h, 1e-5, F16), nn.Linear(h, vocab, bias=False, dtype=F16), heads, inv, maxpos)
        names, bits, native3 = decode.LlamaDecoder.NAMES, (3 if kind == "llama-native3" else 2), kind == "llama-native3"
    dec = dec.to(DEV).eval()
    for p_ in dec.parameters():
        if p_.dim() > 1:
            p_.data.normal_(0, 0.02)
    _pack_blocks(dec, names, bits, native3=native3)
    _MODELS[kind] = dec
    return dec


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("bs", [1, 5, 16])
@pytest.mark.parametrize("kind", ["opt", "llama-gqa", "llama-native3"])
def test_decode_engine_inside_an_arena(monkeypatch, kind, bs, graph):
    """DecodeEngine built with the proxy on ops, quant and decode: its KV caches, static buffers, workspaces and every activation of every
    step are carved side by side.  From position 0 to max_len - 1: guards clean, tokens and final logits bit-equal to an engine built on
    ordinary tensors (every mode these models take is deterministic: no launch of them meets through atomics)"""
    from quip_amd import decode
    dec = _model(kind)
    max_len = 6
    first = torch.arange(bs, device=DEV) * 7 % 512
    layers = [m for m in dec.modules() if isinstance(m, decode.QuantLinear)]

    def run():
        eng = decode.DecodeEngine(dec, bs=bs, max_len=max_len, graph=graph)
        toks = eng.generate(first, max_len)
        torch.cuda.synchronize()
        assert eng._steps == max_len and (eng._graph is not None) == graph
        return eng, toks.clone(), eng.logits.clone()

    fz = G.freeze(**_layer_inputs(*layers), tok=dec.tok.weight, head=dec.head_weight)
    _fresh(*layers)()
    eng0, toks0, logits0 = run()
    assert kind != "opt" or eng0.mode == ("v3_head" if bs <= 4 else "v3")
    assert kind == "opt" or eng0.mode == "fused"
    for uninit in (0xFF, 0x00):
        _fresh(*layers)()
        arena = G.GuardArena(2 << 30, DEV, uninit=uninit)
        with G.installed(monkeypatch, arena, *_mods("ops", "quant", "decode")):
            eng, toks, logits = run()
        bad = arena.check()
        assert not bad, bad
        fz.assert_frozen()
        inside = lambda t: arena.buf.data_ptr() <= t.data_ptr() < arena.buf.data_ptr() + arena.buf.numel()
        assert all(inside(c) for kv in eng.caches for c in kv) and inside(eng.logits) and inside(eng.ids) and inside(eng.pos)
        assert eng.mode == eng0.mode and int(eng.pos) == max_len
        assert torch.equal(toks, toks0) and G.bit_equal(logits, logits0), f"fill {uninit:#x}: the guarded engine decodes differently"
        for (kc, vc), (kc0, vc0) in zip(eng.caches, eng0.caches):
            assert G.bit_equal(kc, kc0) and G.bit_equal(vc, vc0)
        del eng
    _fresh(*layers)()


# ------------------------------------------------------------------------------------------------------------------------ one quantisation pass
@pytest.mark.parametrize("which", ["ldlq", "gptq"])
def test_one_quantisation_pass_inside_an_arena(monkeypatch, which):
    """a Linear through add_batch / post_batch / preproc with incoherence processing and then LDLQ (Balance) or OPTQ with the qfn-b scale
    (GPTQ), with the proxy on ops and on the host modules that allocate: the codes / the stored weights equal the unguarded run"""
    from quip_amd import quant as Q
    from quip_amd.bal import Balance
    from quip_amd.gptq import GPTQ
    d, mrows = 512, 64
    g = torch.Generator().manual_seed(0)
    W0 = (0.02 * torch.randn(mrows, d, generator=g)).half().to(DEV)
    A_ = torch.randn(d, d, generator=g) / d ** 0.5
    X = ((torch.randn(4, 128, d, generator=g) * torch.arange(1, d + 1) ** -0.5) @ A_).half().to(DEV)

    def run():
        torch.manual_seed(1)
        np.random.seed(1)
        lin = torch.nn.Linear(d, mrows).half().to(DEV)
        lin.weight.data = W0.clone()
        meth = (Balance if which == "ldlq" else GPTQ)(lin)
        if which == "ldlq":
            meth.configure("ldlq", 2, 0, unbiased=False)
        meth.quantizer = Q.Quantizer()
        meth.quantizer.configure(2, perchannel=True, sym=False, qfn="b", mse=False)
        for j in range(X.shape[0]):
            meth.add_batch(X[j].unsqueeze(0), None)
        meth.post_batch()
        meth.preproc(preproc_gptqH=True, percdamp=.01, preproc_rescale=True, preproc_proj=True, preproc_proj_extra=0)
        meth.fasterquant(lazy_batch=False) if which == "ldlq" else meth.fasterquant()
        torch.cuda.synchronize()
        codes = getattr(meth, "codes", None)
        return (None if codes is None else codes.clone()), lin.weight.data.clone()

    codes0, w0 = run()
    assert which != "ldlq" or codes0 is not None
    names = [n for n in ("ops", "quant", "method", "bal", "gptq", "vector_balance") if getattr(_mods(n)[0], "torch", None) is torch]
    assert "ops" in names and "method" in names
    for uninit in (0xFF, 0x00):
        arena = G.GuardArena(512 << 20, DEV, uninit=uninit)
        with G.installed(monkeypatch, arena, *_mods(*names)):
            codes, w = run()
        bad = arena.check()
        assert not bad, bad
        assert len(arena.regions) >= 8
        assert G.bit_equal(w, w0) and (codes0 is None or torch.equal(codes, codes0)), f"fill {uninit:#x}: the guarded pass quantises differently"


# ------------------------------------------------------------------------------------------------------------------------ completeness
def test_zz_every_kernel_launching_entry_point_ran_under_an_arena():
    """reads the ledger (every C ABI call goes through quip_amd._lib.call): a new entry point fails here until it has a guarded case above"""
    from quip_amd import _lib
    assert EXEMPT <= set(_lib.SIGNATURES), sorted(EXEMPT - set(_lib.SIGNATURES))
    launching = set(_lib.SIGNATURES) - EXEMPT
    missing = sorted(launching - G.LEDGER)
    assert not missing, f"entry points without a guarded case: {missing}"
