"""CPU test (needs hipcc, no GPU): which x slab every LDS read of dq_h_kernel / dq_hg_kernel finds landed (csrc/dq_h_body.inc).

A wave's x arrives by LDS-DMA (`buffer_load_dwordx4 ... lds`), one slab of NDMA instructions per k-chunk, and is read back with
`ds_read_b128 ... offset:N` behind a counted `s_waitcnt vmcnt(N)`.  Since the issue-ahead schedule (K2_AHEAD) the slabs of later chunks are
requested BETWEEN the MFMA steps of earlier ones, so the wait counts are no longer one formula over a fixed prologue.  This audit replays the
vector-memory queue of every EXACT instantiation in program order, as tests/test_k2_isa.py does for the weight registers:
  * the n-th LDS-DMA instruction belongs to chunk n // NDMA (slabs are requested in chunk order, NDMA instructions each);
  * a ds_read_b128 with offset N in front of the block barrier reads chunk N // XB (slab i of a wave starts i * XB into its region, and a
    lane's base address stays inside the first column block);
  * memory returns in order: s_waitcnt vmcnt(N) leaves the N youngest operations in the queue.
No read may find an LDS-DMA of its own chunk still in the queue, and no instruction may touch the destination of a ds_read_b128 before an
`s_waitcnt lgkmcnt(0)` (the reads are inline asm: hipcc does not know their data is late).  NDMA and XB follow from BITS and HALF in the
mangled name.  The headline instantiations must also issue their first MFMA before their last LDS-DMA: the property the schedule exists for."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NAME = re.compile(r"dq_hg?_kernelILi(\d+)ENS_\d+(Act\w+?)ELi(\d+)ELi(\d+)ELi(\d+)ELb([01])ELb([01])EE")
VMEM = ("global_load", "buffer_load", "global_store", "buffer_store", "scratch_", "flat_")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not shutil.which(HIPCC) and not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa_slabs") / "dqgemm_v2.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "quip_amd", "csrc"),
                           os.path.join(ROOT, "quip_amd", "csrc", "dqgemm_v2.hip"), "-o", str(out)])
    return out.read_text().splitlines()


def _exact_kernels(lines):
    """(name, (bits, act, rt, nw, nch, half), instructions) of every EXACT dq_h_kernel / dq_hg_kernel instantiation"""
    cur, body = None, []
    for ln in lines:
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            cur, body = m.group(1), []
            continue
        if cur is None:
            continue
        s = ln.split(";")[0].strip()
        if s and not s.startswith("."):
            body.append(s)
        if ".end_amdhsa_kernel" in ln:
            k = NAME.search(cur)
            if k and k.group(7) == "1":
                yield cur, (int(k.group(1)), k.group(2), int(k.group(3)), int(k.group(4)), int(k.group(5)), k.group(6) == "1"), body
            cur = None


def _regs(tok):
    out = set()
    for a, b in re.findall(r"\bv\[(\d+):(\d+)\]", tok):
        out |= set(range(int(a), int(b) + 1))
    for a in re.findall(r"\bv(\d+)\b", tok):
        out.add(int(a))
    return out


def _replay(name, par, body):
    """returns (index of the first MFMA, index of the last LDS-DMA) after asserting the slab discipline"""
    bits, _, _, _, nch, half = par
    kc = 512 // bits
    ncb = kc * 2 // 128
    ndma = ncb if half else 2 * ncb
    xb = ncb * (1024 if half else 2048)
    queue = []                    # outstanding vector-memory operations, oldest first: chunk of an LDS-DMA | None
    late = set()                  # destination registers of ds_read_b128s that no lgkmcnt(0) has retired
    n_dma = n_read = 0
    first_mfma = last_dma = None
    for i, s in enumerate(body):
        op = s.split()[0]
        if op == "s_barrier":
            break
        if op == "ds_read_b128":
            m = re.search(r"offset:(\d+)", s)
            chunk = (int(m.group(1)) if m else 0) // xb
            assert chunk < nch, f"{name}: line {i}: `{s}` reads past the wave's {nch} slabs"
            assert chunk not in queue, (f"{name}: line {i}: `{s}` reads slab {chunk} with {queue.count(chunk)} of its LDS-DMA "
                                        f"instructions still in the queue")
            late |= _regs(s.split(",")[0])
            n_read += 1
            continue
        assert not (_regs(s) & late), f"{name}: line {i}: `{s}` touches a ds_read_b128 destination before s_waitcnt lgkmcnt(0)"
        if op.startswith(VMEM):
            if op == "buffer_load_dwordx4" and s.endswith(" lds"):
                queue.append(n_dma // ndma)
                n_dma += 1
                last_dma = i
            else:
                queue.append(None)
        if op.startswith("v_mfma") and first_mfma is None:
            first_mfma = i
        if op == "s_waitcnt":
            m = re.search(r"vmcnt\((\d+)\)", s)
            if m:
                keep = int(m.group(1))
                queue = queue[len(queue) - keep:] if keep else []
            if "lgkmcnt(0)" in s:
                late = set()
    assert n_dma == nch * ndma, f"{name}: {n_dma} LDS-DMA instructions, expected {nch} slabs x {ndma}"
    assert n_read == nch * (kc // 32), f"{name}: {n_read} fragment reads, expected {nch} chunks x {kc // 32} MFMA steps"
    assert not [c for c in queue if c is not None], f"{name}: LDS-DMA still in flight at the block barrier"
    return first_mfma, last_dma


def test_no_read_finds_its_slab_in_flight(asm):
    seen = set()
    for name, par, body in _exact_kernels(asm):
        _replay(name, par, body)
        seen.add(("hg" if "dq_hg_kernel" in name else "h",) + par)
    assert len(seen) >= 32, f"only {len(seen)} exact dq_h_kernel / dq_hg_kernel instantiations found"
    for act in ("ActBF16", "ActF16"):
        for half in (False, True):
            assert ("h", 2, act, 1, 4, 4, half) in seen, f"the headline instantiation <2, {act}, 1, 4, 4, HALF {half}> is missing"


def test_headline_starts_its_arithmetic_before_its_last_request(asm):
    """<2, bf16 | f16, RT 1, NW 4, NCH 4, HALF 0 | 1, EXACT> of dq_h_kernel: compute overlaps the ingest of x"""
    n = 0
    for name, par, body in _exact_kernels(asm):
        if "dq_hg_kernel" in name or par[0] != 2 or par[2:5] != (1, 4, 4):
            continue
        first_mfma, last_dma = _replay(name, par, body)
        assert first_mfma is not None and last_dma is not None and first_mfma < last_dma, \
            f"{name}: first MFMA at instruction {first_mfma}, last LDS-DMA at {last_dma}: request everything, then consume"
        n += 1
    assert n == 4
