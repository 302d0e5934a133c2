"""CPU test (needs hipcc, no GPU): the headline instantiation dq_h_kernel<2, bf16, RT 1, NW 4, NCH 4, full slabs, exact K> dequantises its
2-bit codes with the multi-exponent form (csrc/dq_common.h DeqME2, selected in csrc/dq_h_body.inc): three neighbouring fields share one
shift, 10 VALU per packed dword instead of 16, and both row sums (S_1, S_off) come from the one row-sum MFMA of a step.

dqgemm_v2.hip is compiled with the flags build() uses for it, as tests/test_k2_isa_preload.py does.  In the generated code of that
instantiation:

  * the vector-ALU instructions (v_*, other than v_mfma_* and v_accvgpr_*) between the first and the last MFMA, both included, number at
    most PARENT_VALU - 80: a wave has 16 packed dwords and saves 6 VALU on each (96); 16 are slack for address arithmetic the scheduler moves
    in or out of the stretch;
  * exactly 64 MFMAs remain (32 steps x {product, row sums}: the second row sum costs no MFMA);
  * the number of instructions in front of the first weight request (`global_load_dwordx4 ... nt`), counted behind the compatibility
    prologue of the kernel-argument preload, is at most PARENT_HEAD: the head of the wave did not grow.

The parent's figures, from this file's own counters on the build of the commit before the change (uniform-offset form; the same as a
-DK2_H_UNIFORM=1 build of this tree, whose code for every dq_h / dq_hg / dq_hr instantiation is instruction for instruction the
parent's): 253 VALU between the first and the last MFMA, 64 MFMAs, 27 instructions in front of the first weight request.  This build: 157 VALU,
64 MFMAs, 27 instructions."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRC = "dqgemm_v2.hip"
# Itanium mangling of dq_h_kernel<2, ActBF16, 1, 4, 4, false, true>
HEADLINE = "dq_h_kernelILi2ENS_7ActBF16ELi1ELi4ELi4ELb0ELb1EEE"
PARENT_VALU = 253
PARENT_HEAD = 27


def _functions(text):
    cur, body = None, []
    for ln in text.splitlines():
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            cur, body = m.group(1), []
            continue
        if cur is not None:
            body.append(ln)
            if ".end_amdhsa_kernel" in ln:
                yield cur, body
                cur = None


def _instructions(body):
    out = []
    for ln in body:
        s = ln.split(";")[0].strip()
        if s and not s.startswith(".") and not s.endswith(":"):
            out.append(s)
        if s.startswith("s_endpgm"):
            break
    return out


def _behind_compat_prologue(ins):
    """the loads of the preloaded arguments, a wait and an s_branch over padding to byte 256: the body proper starts behind that branch"""
    br = next((i for i, s in enumerate(ins[:16]) if s.startswith("s_branch")), None)
    if br is None:
        return ins
    rest = ins[br + 1:]
    while rest and rest[0].startswith(("s_nop", "s_code_end")):
        rest = rest[1:]
    return rest


def count(text):
    """(VALU between the first and the last MFMA, MFMAs, instructions in front of the first weight request) of the headline instantiation"""
    found = [(n, b) for n, b in _functions(text) if HEADLINE in n]
    assert len(found) == 1, f"{len(found)} kernels match {HEADLINE}"
    ins = _behind_compat_prologue(_instructions(found[0][1]))
    mf = [i for i, s in enumerate(ins) if s.startswith("v_mfma")]
    valu = [s for s in ins[mf[0]:mf[-1] + 1] if s.startswith("v_") and not s.startswith(("v_mfma", "v_accvgpr"))]
    head = next(i for i, s in enumerate(ins) if s.startswith("global_load_dwordx4") and s.endswith(" nt"))
    return len(valu), len(mf), head


@pytest.fixture(scope="module")
def counts(tmp_path_factory):
    if not shutil.which(HIPCC) and not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    sys.path.insert(0, ROOT) if ROOT not in sys.path else None
    import __graft_entry__ as entry
    out = tmp_path_factory.mktemp("isa_me") / "dqgemm_v2.s"
    subprocess.check_call([HIPCC] + entry.hip_flags(SRC) + ["--cuda-device-only", "-S", os.path.join(ROOT, "quip_amd", "csrc", SRC), "-o", str(out)])
    c = count(out.read_text())
    print(f"headline: {c[0]} VALU between the first and the last MFMA (parent {PARENT_VALU}), {c[1]} MFMAs, "
          f"{c[2]} instructions in front of the first weight request (parent {PARENT_HEAD})")
    return c


def test_the_mfma_stretch_lost_the_shifts(counts):
    assert counts[0] <= PARENT_VALU - 80, f"{counts[0]} VALU between the first and the last MFMA; the parent had {PARENT_VALU}"


def test_the_second_row_sum_costs_no_mfma(counts):
    assert counts[1] == 64


def test_the_head_of_the_wave_did_not_grow(counts):
    assert counts[2] <= PARENT_HEAD, f"{counts[2]} instructions in front of the first weight request; the parent had {PARENT_HEAD}"


if __name__ == "__main__":                                            # python tests/test_k2_isa_me.py file.s: the counters on an assembly file
    print(count(open(sys.argv[1]).read()))
