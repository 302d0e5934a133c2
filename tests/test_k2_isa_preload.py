"""CPU test (needs hipcc, no GPU): the head of dq_h_kernel / dq_hg_kernel in the code the BUILD generates (csrc/dq_h_body.inc, K2_HEAD;
csrc/dqgemm_v2.h, K2_FLAT_ARGS).

The cold critical path of the headline launch is wave start -> kernel arguments -> weight request -> HBM round trip -> ...: what sits in
front of the first weight request delays the whole launch.  dqgemm_v2.hip is compiled here with exactly the flags build() uses for it (the
common ones plus its entry in __graft_entry__.EXTRA_FLAGS: kernel-argument preload), and for every instantiation:

  dq_h_kernel   the kernel descriptor preloads at least x, qw and d (6 SGPRs), and in the body behind the compatibility prologue (the
                s_loads + s_branch + padding a non-preloading firmware enters through; a preloading one starts 256 bytes in) the first weight
                tile request (`global_load_dwordx4 ... nt`) precedes every `s_waitcnt` that names lgkmcnt and every other global_load /
                buffer_load: no scalar round trip and no other vector-memory request in front of it;
  dq_hg_kernel  (three structs: no preload) at most ONE s_waitcnt lgkmcnt precedes the first weight request, and no other vector-memory
                request does.

tests/test_k2_isa.py and tests/test_k2_isa_slabs.py keep auditing the same source compiled without the per-source flags."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRC = "dqgemm_v2.hip"


def _build_flags():
    """the flags of build() for SRC, from the entry point's own helper"""
    sys.path.insert(0, ROOT) if ROOT not in sys.path else None
    import __graft_entry__ as entry
    flags = entry.hip_flags(SRC)
    assert "-amdgpu-kernarg-preload-count=16" in flags, "build() no longer asks for kernel-argument preload in " + SRC
    return flags


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not shutil.which(HIPCC) and not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa_preload") / "dqgemm_v2.s"
    subprocess.check_call([HIPCC] + _build_flags() + ["--cuda-device-only", "-S", os.path.join(ROOT, "quip_amd", "csrc", SRC), "-o", str(out)])
    found, cur, body = [], None, []
    for ln in out.read_text().splitlines():
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            cur, body = m.group(1), []
            continue
        if cur is not None:
            body.append(ln)
            if ".end_amdhsa_kernel" in ln:
                found.append((cur, body))
                cur = None
    return found


def _instructions(body):
    out = []
    for ln in body:
        s = ln.split(";")[0].strip()
        if s and not s.startswith(".") and not s.endswith(":"):
            out.append(s)
        if s.startswith("s_endpgm"):
            break
    return out


def _behind_compat_prologue(name, ins, preload):
    """with a preload length the compiler emits, at the kernel's entry, the loads of the preloaded arguments, a wait, an s_branch over
    padding to byte 256: the body proper starts behind that branch"""
    if not preload:
        return ins
    br = next((i for i, s in enumerate(ins[:16]) if s.startswith("s_branch")), None)
    assert br is not None, f"{name}: preload length {preload} but no compatibility prologue"
    assert all(s.startswith(("s_load", "s_waitcnt")) for s in ins[:br]), f"{name}: unexpected instructions in the compatibility prologue: {ins[:br]}"
    rest = ins[br + 1:]
    while rest and rest[0].startswith(("s_nop", "s_code_end")):
        rest = rest[1:]
    return rest


def _head(name, body):
    """(preload length, number of s_waitcnt lgkmcnt in front of the first weight request, other vector-memory loads in front of it)"""
    meta = "\n".join(body)
    m = re.search(r"\.amdhsa_user_sgpr_kernarg_preload_length\s+(\d+)", meta)
    preload = int(m.group(1)) if m else 0
    ins = _behind_compat_prologue(name, _instructions(body), preload)
    first = next((i for i, s in enumerate(ins) if s.startswith("global_load_dwordx4") and s.endswith(" nt")), None)
    assert first is not None, f"{name}: no weight tile request"
    waits = [s for s in ins[:first] if s.startswith("s_waitcnt") and "lgkmcnt" in s]
    loads = [s for s in ins[:first] if s.startswith(("global_load", "buffer_load"))]
    return preload, waits, loads


def test_one_problem_kernel_preloads_its_pointers_and_requests_the_weights_first(kernels):
    n = 0
    for name, body in kernels:
        if "dq_h_kernel" not in name:
            continue
        n += 1
        preload, waits, loads = _head(name, body)
        assert preload >= 6, f"{name}: kernarg_preload_length {preload}: x, qw and d are not all preloaded"
        assert not waits, f"{name}: {waits} in front of the first weight request"
        assert not loads, f"{name}: {loads} in front of the first weight request"
    assert n >= 32, f"only {n} dq_h_kernel instantiations found"


def test_grouped_kernel_reads_its_arguments_in_one_round_trip(kernels):
    n = 0
    for name, body in kernels:
        if "dq_hg_kernel" not in name:
            continue
        n += 1
        _, waits, loads = _head(name, body)
        assert len(waits) <= 1, f"{name}: {len(waits)} scalar round trips in front of the first weight request: {waits}"
        assert not loads, f"{name}: {loads} in front of the first weight request"
    assert n >= 16, f"only {n} dq_hg_kernel instantiations found"
