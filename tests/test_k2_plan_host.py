"""CPU: which kernel a fused dequant-GEMM call runs, asked of the library (quipamd_dequant_gemm_plan -> csrc/k2_plan.h; nothing is launched).

1. Over a lattice of shapes the library's plan equals the rules of tests/k2_rules.py, which were written against the dispatch code before
   k2_plan.h existed.
2. Every (shape, override) the GPU tests run yields the kernel their names and docstrings claim; the lists are the GPU tests' own.
3. The plan follows the calling thread's quipamd_tune_dequant_gemm state, and no other thread's."""
import itertools
import os
import sys
import threading

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import k2_rules as R  # noqa: E402
import test_gpu_dqgemm as T1  # noqa: E402
import test_gpu_dqgemm_v2 as T2  # noqa: E402
import test_gpu_memory_contract as MC  # noqa: E402
import test_gpu_stream3 as T3  # noqa: E402
from quip_amd import _lib, ops  # noqa: E402

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
FAM_OLD, FAM_H, FAM_S, FAM_MB = 1, 2, 3, 4
# family mb, p1 -> <WB, RTw, BTw, NL, T32> at 2 bits (include/quip_amd.h; 4 bits: the 256 x 128 forms take RTw = 2, 46 .. 49 do not exist)
MB_FORMS = {22: (2, 2, 2, 2, 0), 23: (2, 2, 2, 4, 0), 44: (2, 4, 4, 2, 0), 45: (2, 4, 4, 4, 0), 46: (2, 4, 4, 3, 0), 47: (2, 4, 4, 4, 1),
            48: (1, 4, 8, 2, 0), 49: (1, 4, 8, 4, 0)}
S_FORMS = {(1, 8): (1, 8, 1, 2), (2, 4): (2, 4, 1, 3), (4, 2): (4, 2, 1, 4), (7, 2): (7, 2, 1, 3), (8, 1): (8, 1, 2, 3)}
SG_FORMS = {74: (4, 2, 1, 4), 72: (7, 2, 1, 3), 81: (8, 1, 2, 3)}


def plan(m, d, bs, bits, dt=BF16, **kw):
    return ops.dequant_gemm_plan(bs, m, d, bits, x_dtype=dt, **kw)


def branch(m, d, bs, bits, dt=BF16, **kw):
    """the plan in the words of tests/k2_rules.py; "none" for a refused call"""
    try:
        return R.plan_branch(plan(m, d, bs, bits, dt, **kw), 2 if bits == 2 else 4)
    except _lib.QuipAmdError:
        return "none"


@pytest.fixture(autouse=True)
def _no_overrides_left_behind():
    yield
    _lib.load().quipamd_tune_dequant_gemm(0, 0, 0, 0)
    ops.dequant_gemm_grouped_config(0)


# ---------------------------------------------------------------------------------------------------------------- 1. the lattice
# row tiles on both sides of every threshold of the rules (128, 256, 384, 512, 640, 768, 1024 and the 4 / 7 / 8 x 256 rounds of the s and w3
# kernels), counts not divisible by 2 or 4 among them
ROW_TILES = sorted({t + o for t in (128, 256, 384, 512, 640, 768, 1024, 1792, 2048) for o in (-1, 0, 1, 2, 4)} | {1, 3, 4, 1023, 1028, 1793, 2047, 2052})
DS = [256, 512, 1024, 2048, 2304, 4096, 4352, 6144, 8192, 8448, 11008]               # one LDS pass ends at 4096 (2 bit), two at 8192
BSS = [1, 8, 9, 16, 17, 64, 65, 129, 300, 2048]


def test_the_lattice_covers_what_it_claims():
    assert all({t - 1, t, t + 1} <= set(ROW_TILES) for t in (128, 256, 384, 512, 640, 768, 1024, 1792, 2048))
    assert any(t % 2 for t in ROW_TILES) and any(t % 4 == 2 for t in ROW_TILES)
    assert min(DS) == 256 and max(DS) == 11008 and {4096, 4352, 8192, 8448} <= set(DS)


@pytest.mark.parametrize("bits", [2, 3, 4])
def test_single_calls_follow_the_rules_over_the_lattice(bits):
    cbits, bad, seen = (2 if bits == 2 else 4), [], set()
    for nt, d, bs, dt, acc in itertools.product(ROW_TILES, DS, BSS, (BF16, F16), (False, True)):
        m = 16 * nt
        want = R.k2_branch(cbits, dt == F16, m, d, bs, acc)
        got = branch(m, d, bs, bits, dt, accumulate=acc, out_dtype=F32 if acc else None)
        seen.add(want)
        if got != want:
            bad.append((m, d, bs, dt, acc, want, got))
    assert not bad, f"{len(bad)} shapes, the first: {bad[:5]}"
    assert seen >= ({"h", "h rt2 8x1", "h rt2 4x4", "h rt4 4x4", "h-half", "h-half x 2", "s", "mb", "round-1"} if bits == 2 else {"h", "s", "mb", "round-1"})


def test_stream3_follows_the_cost_rule_over_the_lattice():
    for nt, d, bs, dt, groups in itertools.product(ROW_TILES, [256, 768, 4096, 11008], [1, 16, 17, 300], (BF16, F16), (1, 2, 3, 4)):
        kernel, p, kslices, launches = plan(16 * nt, d, bs, 3, dt, layout=ops.LAYOUT_STREAM3, ngroups=groups)
        assert kernel == "w3" and p[0] == R.w3_nw(16 * nt) and p[:4] == S_FORMS[(p[0], p[1])] and launches == groups and kslices == 1


@pytest.mark.parametrize("bits", [2, 4])
def test_groups_follow_the_rules_over_the_lattice(bits):
    bad = []
    for nt, d, bs, dt, acc, groups in itertools.product(ROW_TILES, DS, BSS[:6], (BF16, F16), (False, True), (2, 3, 4)):
        m = 16 * nt
        want = R.grouped_branch(bits, dt == F16, groups, m, d, bs, accumulate=acc)
        try:
            pl = plan(m, d, bs, bits, dt, accumulate=acc, out_dtype=F32 if acc else None, ngroups=groups)
            got = R.plan_branch(pl, bits)
            # one launch for the grouped kernels and the round-1 tile kernel (grid.y), else one per problem
            one = pl[0] in ("hg", "sg", "r1_tile")
            got = got if one or dt == BF16 else "each: " + got
            assert pl[3] == (1 if one else groups), (m, d, bs, pl)
        except _lib.QuipAmdError:
            got = "each: none" if dt == F16 else "none"
        if dt == BF16 and got == "none":
            continue                                                   # a round-1 refusal: the rules do not describe the round-1 instantiations
        if got != want:
            bad.append((m, d, bs, dt, acc, groups, want, got))
    assert not bad, f"{len(bad)} shapes, the first: {bad[:5]}"


# ---------------------------------------------------------------------------------------------------------------- 2. the GPU tests' lists
def test_memory_contract_default_shapes():
    for (m, d, bs), bits, f16 in itertools.product(MC.K2_DEFAULT, (2, 4), (False, True)):
        assert branch(m, d, bs, bits, F16 if f16 else BF16) == R.k2_branch(bits, f16, m, d, bs) != "none"
    got = {branch(m, d, bs, 2, dt) for m, d, bs in MC.K2_DEFAULT for dt in (BF16, F16)}
    assert got == {"h", "h rt2 8x1", "h rt2 4x4", "h rt4 4x4", "h-half", "h-half x 2", "s", "mb", "round-1"}


def check_forced(cfg, m, d, bs, bits, dt):
    """a cfg of quipamd_dequant_gemm_cfg yields the family and form it names"""
    kernel, p, kslices, launches = plan(m, d, bs, bits, dt, cfg=cfg)
    assert launches == 1 and kslices == 1
    if cfg[0] == FAM_OLD:
        assert kernel.startswith("r1_") and dt == BF16
    elif cfg[0] == FAM_H and cfg[1] == 44:
        assert kernel == "hr" and d == 4096
    elif cfg[0] == FAM_H:
        rt = p[0]
        assert kernel == "h" and p[1:3] == cfg[1:3] and d // (512 // bits) <= cfg[1] * cfg[2] and (m // 16) % rt == 0
    elif cfg[0] == FAM_S:
        assert kernel == "s" and p[:4] == S_FORMS[cfg[1:3]]
    else:
        want = MB_FORMS[cfg[1]]
        assert kernel == "mb" and p == (want if bits == 2 or cfg[1] not in (44, 45) else (2, 2, 4, want[3], 0))


def test_memory_contract_forced_kernels():
    for cfg, (m, d, bs), bits in MC.FORCED:
        for dt in (BF16, F16):
            if not (cfg[0] == FAM_OLD and dt == F16):
                check_forced(cfg, m, d, bs, bits, dt)
    assert {c[1] for c, _, _ in MC.FORCED if c[0] == FAM_MB} == set(MB_FORMS)
    assert {c[1:3] for c, _, _ in MC.FORCED if c[0] == FAM_S} == set(S_FORMS)


def check_tuned(tune, m, d, bs, bits, accumulate=False):
    """quipamd_tune_dequant_gemm(rt, bt, nw, split) yields the round-1 kernel and workgroup shape it names; returns the plan"""
    lib = _lib.load()
    rt, bt, nw, split = (tuple(tune) + (0,))[:4]
    lib.quipamd_tune_dequant_gemm(rt, bt, nw, split)
    try:
        kernel, p, kslices, launches = pl = plan(m, d, bs, bits, BF16, accumulate=accumulate, out_dtype=F32 if accumulate else None)
    finally:
        lib.quipamd_tune_dequant_gemm(0, 0, 0, 0)
    rt_eff = rt if rt and (m // 16) % rt == 0 else None               # a row-tile count that does not divide the row tiles is not taken
    if split // 100 == 9:
        assert kernel == "r1_batched" and p[0] == rt
    elif bt == 0 and bs <= 16:
        assert kernel == "r1_tile" and launches == 1
        assert rt_eff is None or p[0] == rt_eff
        assert p[1] == max(nw // p[0], 1) and p[2] == (split // 100 or 1)
        assert kslices == split % 100 if accumulate and split % 100 else accumulate or kslices == 1     # k-slices only under the accumulate contract
    else:
        assert kernel == "r1_wave" and (rt_eff is None or p[0] == rt_eff) and p[1] == (bt or 1) and p[2] == (nw or 16)
    return pl


def test_memory_contract_round1_and_accumulate_cases():
    for (m, d, bs), tune in MC.ROUND1:
        check_tuned(tune, m, d, bs, 2)
    acc = [m_ for m_ in MC.test_dequant_gemm_accumulate_into_the_callers_y.pytestmark if m_.name == "parametrize"]
    tunes = next(m_.args[1] for m_ in acc if m_.args[0] == "rt,nw,split")
    shapes = next(m_.args[1] for m_ in acc if m_.args[0] == "m,d,bs,bits")
    for (rt, nw, split), (m, d, bs, bits) in itertools.product(tunes, shapes):
        if rt:
            assert check_tuned((rt, 0, nw, split), m, d, bs, bits, accumulate=True)[2] == split      # split-K: `split` k-slices meet in y
        else:
            assert branch(m, d, bs, bits, accumulate=True, out_dtype=F32) == R.k2_branch(bits, False, m, d, bs, True)


def check_grouped(form, m, groups, bs, d):
    ops.dequant_gemm_grouped_config(form)
    try:
        kernel, p, kslices, launches = pl = plan(m, d, bs, 2, F16, ngroups=groups, out_dtype=F32)
    finally:
        ops.dequant_gemm_grouped_config(0)
    assert launches == 1 and R.plan_branch(pl, 2) == R.grouped_branch(2, True, groups, m, d, bs, form=form)
    if form in SG_FORMS:
        assert kernel == "sg" and p[:4] == SG_FORMS[form]
    elif form:
        assert kernel == "hg" and (p[0] == form or (m // 16) % form)
    return kernel


def test_grouped_forms():
    assert {check_grouped(*g) for g in MC.GROUPED} == {"hg", "sg"}
    assert {check_grouped(form, m, groups, bs, 4096) for form in T2.GROUPED_FORMS for m, groups, bs in T2.GROUPED_SHAPES} == {"hg", "sg"}
    assert check_grouped(0, 11008, 2, 16, 4096) == "sg" and check_grouped(0, 2064, 2, 9, 4096) == "hg"     # beyond two rounds of workgroups / within


def test_stream3_shapes():
    for shapes in (MC.W3_SHAPES, T3.SHAPES):
        got = set()
        for m, d, bs in shapes:
            for dt in (BF16, F16):
                kernel, p, _, launches = plan(m, d, bs, 3, dt, layout=ops.LAYOUT_STREAM3)
                assert kernel == "w3" and p[0] == R.w3_nw(m) and launches == 1
                got.add(p[0])
        assert got == {1, 2, 4, 7, 8}
    assert plan(256, 1024, 7, 3, F16, layout=ops.LAYOUT_STREAM3, ngroups=3)[3] == 3      # a group: one launch per problem


def test_round1_lists_of_test_gpu_dqgemm():
    m, d, bs, bits = T1.WORKGROUP_SHAPE
    kernels = {check_tuned(t, m, d, bs, bits)[0] for t in T1.WORKGROUP_TUNES}
    assert kernels == {"r1_tile", "r1_wave"}                            # "both K2 kernels"
    assert check_tuned((8, 0, 16, 200), m, d, bs, bits)[1][:3] == (8, 2, 2)
    for (rt, nw, split), (m, d, bs, bits) in itertools.product(T1.SPLIT_K_TUNES, T1.SPLIT_K_SHAPES):
        if rt:
            assert check_tuned((rt, 0, nw, split), m, d, bs, bits, accumulate=True)[2] == split
    # the heuristic under the accumulate contract: the small-m shapes that the v2 kernels decline take the split-K path
    assert plan(4096, 4096, 16, 2, accumulate=True, out_dtype=F32, cfg=(FAM_OLD,)) == ("r1_tile", (2, 4, 1, 0, 0), 4, 1)
    for (rt, sp), (m, d, bs), bits in itertools.product(T1.BATCHED_TUNES, T1.BATCHED_SHAPES, (2, 4)):
        if rt and (m // 16) % (2 * rt) == 0:
            check_tuned((rt, 0, 0, sp), m, d, bs, bits)


def test_forced_lists_of_test_gpu_dqgemm_v2():
    for (m, d, bs), bits, dt in itertools.product(T2.H_SHAPES, (2, 4), (BF16, F16)):
        for cfg in T2.H_CFGS[bits]:
            if d // (512 // bits) <= cfg[1] * cfg[2]:
                check_forced(cfg, m, d, bs, bits, dt)
    for (m, d, bs), bits, dt, cfg in itertools.product(T2.S_SHAPES, (2, 4), (BF16, F16), T2.S_CFGS):
        check_forced(cfg, m, d, bs, bits, dt)
    for (m, d, bs), bits, dt in itertools.product(T2.MB_SHAPES, (2, 4), (BF16, F16)):
        for cfg in T2.MB_CFGS + (T2.MB_CFGS_2BIT if bits == 2 else []):
            check_forced(cfg, m, d, bs, bits, dt)
    for (m, bs), dt in itertools.product(T2.HR_SHAPES, (BF16, F16)):
        check_forced((FAM_H, 44, 4), m, 4096, bs, 2, dt)
    for m, d, bs, cfg in T2.LARGE_FORCED:
        check_forced(cfg, m, d, bs, 2, BF16)
    for (m, d, bs), dt in itertools.product(T2.HALF_SHAPES, (BF16, F16)):   # "9..16 rows of up to 128 row tiles run it as two half-batch problems"
        assert plan(m, d, bs, 2, dt)[:2] == ("h_half" if bs <= 8 else "h_half_x2", (1, 8, 4, 0, 0)) and (bs <= 8 or m // 16 <= 128)


def test_refusals_keep_status_and_message():
    def refused(match, *a, **kw):
        with pytest.raises(_lib.QuipAmdError, match=match):
            plan(*a, **kw)
    refused(r"code 4\).*kernel family 5", 256, 256, 256, 2, cfg=(5, 21))
    refused(r"code 4\).*family h needs", 64, 8192, 4, 2, cfg=(FAM_H, 8, 2))
    refused(r"code 4\).*family s needs", 64, 8192, 40, 2, cfg=(FAM_S, 7, 2))
    refused(r"code 4\).*no s kernel for nw=5 ksp=5", 64, 8192, 4, 2, cfg=(FAM_S, 5, 5))
    refused(r"code 4\).*no mb kernel 46", 256, 256, 17, 4, cfg=(FAM_MB, 46))
    refused(r"code 4\).*register-x form", 176, 2048, 11, 2, cfg=(FAM_H, 44, 4))
    refused(r"code 4\).*no forced kernel configurations for the STREAM3", 16, 256, 1, 3, layout=ops.LAYOUT_STREAM3, cfg=(3, 4, 2))
    refused(r"code 2\).*STREAM3 layout needs", 16, 384, 1, 3, layout=ops.LAYOUT_STREAM3)
    refused(r"code 4\).*3-bit codes only", 16, 256, 1, 4, layout=ops.LAYOUT_STREAM3)
    refused(r"code 4\).*STREAM layout", 16, 256, 1, 2, layout=ops.LAYOUT_CANONICAL)
    refused(r"code 2\).*needs m % 16 == 0 and d % 256 == 0", 24, 256, 1, 2)
    refused(r"code 4\).*fp16 activations need d % 256", 16, 384, 17, 4, F16)
    refused(r"code 4\).*round-1 kernels are bf16 only", 16, 256, 1, 2, F16, cfg=(FAM_OLD,))
    refused(r"code 1\).*1..4 problems", 16, 256, 1, 2, ngroups=5)
    refused(r"code 4\).*accumulate needs f32 y", 16, 256, 1, 2, accumulate=True)
    assert plan(16, 256, 0, 2) == ("none", (0, 0, 0, 0, 0), 1, 0)         # an empty batch: nothing to launch


# ---------------------------------------------------------------------------------------------------------------- 3. the tune state
def test_the_plan_shows_the_tune_state_and_then_the_heuristic():
    lib = _lib.load()
    shape = (4096, 4096, 16, 2)                                           # the headline
    assert plan(*shape) == ("h", (1, 4, 4, 0, 0), 1, 1)
    lib.quipamd_tune_dequant_gemm(2, 0, 8, 0)
    assert plan(*shape) == ("r1_tile", (2, 4, 1, 0, 0), 1, 1)
    assert plan(*shape, cfg=(FAM_H, 8, 2))[:2] == ("h", (1, 8, 2, 0, 0))   # a call that names its family keeps it
    lib.quipamd_tune_dequant_gemm(2, 0, 8, 203)
    assert plan(*shape, accumulate=True, out_dtype=F32) == ("r1_tile", (2, 4, 2, 0, 0), 3, 1)
    lib.quipamd_tune_dequant_gemm(2, 0, 0, 900)
    assert plan(1024, 1024, 256, 2) == ("r1_batched", (2, 0, 0, 0, 0), 1, 1)
    lib.quipamd_tune_dequant_gemm(0, 0, 0, 0)
    assert plan(*shape) == ("h", (1, 4, 4, 0, 0), 1, 1)


def test_a_second_thread_does_not_see_the_first_threads_tune_state():
    lib = _lib.load()
    lib.quipamd_tune_dequant_gemm(2, 0, 8, 0)
    seen = {}

    def other():
        seen["before"] = plan(4096, 4096, 16, 2)
        lib.quipamd_tune_dequant_gemm(4, 0, 16, 0)
        seen["after"] = plan(4096, 4096, 16, 2)
    t = threading.Thread(target=other)
    t.start()
    t.join()
    assert seen["before"] == ("h", (1, 4, 4, 0, 0), 1, 1) and seen["after"] == ("r1_tile", (4, 4, 1, 0, 0), 1, 1)
    assert plan(4096, 4096, 16, 2) == ("r1_tile", (2, 4, 1, 0, 0), 1, 1)   # and this thread keeps its own
