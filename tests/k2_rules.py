"""The dispatch rules of the fused dequant-GEMM restated in Python: ONE copy, imported by tests/test_gpu_memory_contract.py,
tests/test_gpu_stream3.py and tests/test_k2_plan_host.py.

`k2_branch` and `w3_nw` were written against the dispatch code as it stood before csrc/k2_plan.h existed (run_family in dqgemm_v2.hip, run_w3 in
dqgemm_w3.hip), so they are an independent record of that behaviour; tests/test_k2_plan_host.py holds the library's plan
(quipamd_dequant_gemm_plan) to them over a lattice of shapes, and the GPU tests take the branch from the library as well.  `grouped_branch` and
`plan_branch` were added with that test."""


def k2_branch(bits, f16, m, d, bs, accumulate=False):
    """the default dispatch of one problem in the STREAM layout (bits: container bits, 2 | 4): which kernel family serves a call and, inside
    the 2-bit h family, how many row tiles a workgroup takes (launch_h<2, ACT, 2, 8, 1>, <2, ACT, 2, 4, 4>, <2, ACT, 4, 4, 4>)"""
    ntile, nkc = m // 16, d // (512 // bits)
    h_fits = bs <= 16 and nkc <= (16 if bits == 2 else 32)

    def h():
        if bits == 2:
            rt = 4 if (ntile > 512 and ntile % 4 == 0 and nkc > 8) else 2 if (ntile > 256 and ntile % 2 == 0) else 1
            return "h" if rt == 1 else f"h rt{rt} {'8x1' if nkc <= 8 else '4x4'}"
        return "h"
    if bs <= 16:
        if bits == 2 and bs <= 8 and 16 < nkc <= 32 and ntile <= 512:
            return "h-half"
        if bits == 2 and bs > 8 and 16 < nkc <= 32 and ntile <= 128 and not accumulate:
            return "h-half x 2"
        if h_fits and ntile <= 768:
            return h()
        if ntile >= 1024 and d % 256 == 0:
            return "s"
        if f16:                                  # (769 .. 1023 row tiles: the row tiles per workgroup follow the grid here as well; the
            return h() if h_fits else "s" if d % 256 == 0 else "none"      # rule said a bare "h" until the lattice of test_k2_plan_host.py)
        return "round-1"
    tiles = ((m + 255) // 256) * ((bs + 127) // 128)
    if d % 256 == 0 and ((tiles >= 200 and bits == 2) or f16):
        return "mb"
    return "none" if f16 else "round-1"


def w3_nw(m):
    """the STREAM3 layout: row tiles per workgroup -- cost = rounds of 256 workgroups x NW, ties to the larger NW"""
    ntile, best, pick = m // 16, None, None
    for c in (1, 2, 4, 7, 8):
        cost = -(-(-(-ntile // c)) // 256) * c
        if best is None or cost <= best:
            best, pick = cost, c
    return pick


def grouped_branch(bits, f16, groups, m, d, bs, qfn="b", accumulate=False, form=0):
    """2..4 problems of one shape in the STREAM layout: fp16 groups of up to three (grid b) run as ONE launch of the grouped h kernel
    ("hg rt<row tiles>") or, beyond two rounds of one-per-CU workgroups at 8 < chunks <= 16, of the grouped weight-stream kernel
    ("sg <row tiles>"); every other fp16 group as one launch per problem of `k2_branch`'s kernel ("each: ..."); bf16 groups run on the round-1
    kernels.  form: quipamd_dequant_gemm_grouped_config."""
    if not f16:
        return "round-1"
    tiles, nkc = m // 16, d // (512 // bits)
    if groups > 3 or qfn != "b" or bs > 16 or nkc > (16 if bits == 2 else 32) or accumulate or tiles > 768:
        return "each: " + k2_branch(bits, True, m, d, bs, accumulate)
    if bits == 4:
        return "hg rt1"
    if nkc > 8:
        sg = {74: 4, 72: 7, 81: 8}.get(form, 0 if form in (1, 2, 4) else 7 if tiles * groups > 512 else 0)
        if sg:
            return f"sg {sg}"
        rt = 4 if (tiles * groups > 512 and tiles % 4 == 0) else 2 if (tiles * groups > 256 and tiles % 2 == 0) else 1
        return f"hg rt{form if form in (1, 2, 4) and tiles % form == 0 else rt}"
    rt = 2 if (tiles * groups > 256 and tiles % 2 == 0) else 1
    return f"hg rt{form if form in (1, 2) and tiles % form == 0 else rt}"


def plan_branch(plan, bits):
    """a plan of ops.dequant_gemm_plan -- (kernel, parameters, k-slices, launches) -- in the words of the rules above"""
    kernel, p = plan[0], plan[1]
    if kernel == "h":
        return "h" if bits != 2 or p[0] == 1 else f"h rt{p[0]} {p[1]}x{p[2]}"
    return {"r1_tile": "round-1", "r1_wave": "round-1", "r1_batched": "round-1", "h_half": "h-half", "h_half_x2": "h-half x 2", "s": "s", "mb": "mb",
            "hg": f"hg rt{p[0]}", "sg": f"sg {p[0]}", "w3": f"w3 {p[0]}"}[kernel]
