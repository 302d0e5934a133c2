"""CPU tests (no device) of the STREAM3 layout -- 3-bit codes at 3 bits per weight: the NumPy specification round-trips, the C ABI
knows the layout and rejects bad arguments before touching a device, QuantLinear(native3=True) sizes and records itself, and the
generated code of csrc/dqgemm_w3.hip obeys the house rules (no scratch, no waterfall loop around the LDS-DMA, compiler-made bfi)."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream3_spec as S3  # noqa: E402
from oracle import quip_oracle as O  # noqa: E402
from quip_amd import _lib, ops  # noqa: E402
from quip_amd.quant import Quant3Linear, QuantLinear  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SHAPES = [(16, 256), (48, 768), (32, 11008)]


def _pattern(m, d):
    r, k = np.meshgrid(np.arange(m), np.arange(d), indexing="ij")
    return ((5 * r + 3 * k + k // 8) % 8).astype(np.uint8)


@pytest.mark.parametrize("m,d", SHAPES)
def test_spec_round_trips_and_is_three_bits_per_weight(m, d):
    rng = np.random.default_rng(m + d)
    for codes in (rng.integers(0, 8, (m, d), dtype=np.uint8), _pattern(m, d)):
        w = S3.pack_stream3(codes)
        assert w.dtype == np.int32 and w.size == m * d * 3 // 32 == S3.n_words(m, d)
        assert np.array_equal(S3.unpack_stream3(w, m, d), codes)
        # the low plane is the existing 2-bit STREAM tile of code & 3, byte for byte
        assert np.array_equal(S3.low_plane(w, m, d), O.pack_stream(codes & 3, 2))


def test_spec_is_a_permutation_of_the_code_bits():
    m, d = 16, 512
    seen = np.zeros(m * d * 3, dtype=np.int64)
    for bit in range(3):                                          # every single set bit lands on exactly one packed bit, all distinct
        for r, k in [(0, 0), (5, 37), (15, 255), (9, 256), (3, 511)]:
            codes = np.zeros((m, d), dtype=np.uint8)
            codes[r, k] = 1 << bit
            w = S3.pack_stream3(codes).view(np.uint32)
            bits = np.unpackbits(w.view(np.uint8), bitorder="little")
            assert bits.sum() == 1
            seen += bits
    assert seen.max() == 1
    assert np.unpackbits(S3.pack_stream3(np.full((m, d), 7, np.uint8)).view(np.uint8)).all()    # all ones fill every bit: no padding


def test_abi_knows_the_layout_and_checks_arguments_first():
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)           # `one`: non-null, never dereferenced
    assert ops.LAYOUT_STREAM3 == 2
    with pytest.raises(_lib.QuipAmdError, match="STREAM3 layout needs"):
        _lib.call("quipamd_pack", one, 3, 2, one, 16, 100, null)
    with pytest.raises(_lib.QuipAmdError, match="STREAM3 layout needs"):
        _lib.call("quipamd_unpack", one, 3, 2, one, 24, 256, null)
    with pytest.raises(_lib.QuipAmdError, match=r"code 4\)"):     # QUIPAMD_ERR_UNSUPPORTED
        _lib.call("quipamd_pack", one, 2, 2, one, 16, 256, null)
    with pytest.raises(_lib.QuipAmdError, match=r"code 4\)"):
        _lib.call("quipamd_unpack", one, 4, 2, one, 16, 256, null)
    with pytest.raises(_lib.QuipAmdError, match="null pointer"):
        _lib.call("quipamd_repack_canonical_to_stream3", null, one, 16, 256, null)
    with pytest.raises(_lib.QuipAmdError, match="STREAM3 layout needs"):
        _lib.call("quipamd_repack_canonical_to_stream3", one, one, 16, 384, null)
    # K2: shape, width and forced configurations are refused before anything is launched
    gemm = lambda bits, m, d: _lib.call("quipamd_dequant_gemm", one, 1, one, bits, 2, 1, one, null, null, one, 0, 0, 1, m, d, null)
    with pytest.raises(_lib.QuipAmdError, match="STREAM3 layout needs"):
        gemm(3, 16, 384)
    with pytest.raises(_lib.QuipAmdError, match=r"code 4\)"):
        gemm(4, 16, 256)
    cfg = (ctypes.c_int32 * 4)(3, 4, 2, 0)
    with pytest.raises(_lib.QuipAmdError, match=r"code 4\)"):
        _lib.call("quipamd_dequant_gemm_cfg", one, 1, one, 3, 2, 1, one, null, null, one, 0, 0, 1, 16, 256, ctypes.cast(cfg, ctypes.c_void_p), null)
    # empty problems return OK without a device
    _lib.call("quipamd_pack", null, 3, 2, null, 0, 256, null)
    _lib.call("quipamd_dequant_gemm", null, 1, null, 3, 2, 1, null, null, null, null, 0, 0, 0, 16, 256, null)
    # the existing layouts keep their messages
    with pytest.raises(_lib.QuipAmdError, match="STREAM layout"):
        _lib.call("quipamd_dequant_gemm", one, 2, one, 3, 0, 1, one, null, null, one, 2, 0, 1, 16, 256, null)


def test_native3_layer_host_logic():
    q = QuantLinear(512, 64, bits=3, qfn='b', native3=True)
    assert q.native3 and q.layout == ops.LAYOUT_STREAM3 and q.qweight.numel() == 512 * 64 * 3 // 32
    c = QuantLinear(512, 64, bits=3, qfn='b')
    assert not c.native3 and c.layout == ops.LAYOUT_STREAM and c.qweight.numel() == 512 * 64 * 4 // 32
    assert q.packed_bytes() * 4 == c.packed_bytes() * 3
    q3 = Quant3Linear(256, 32, native3=True)
    assert q3.native3 and q3.qfn == 'a' and q3.qweight.numel() == 256 * 32 * 3 // 32
    assert not Quant3Linear(256, 32).native3
    for bad in (dict(bits=2), dict(bits=4)):
        with pytest.raises(ValueError, match="native3"):
            QuantLinear(512, 64, native3=True, **bad)
    with pytest.raises(ValueError, match="native3"):
        QuantLinear(384, 64, bits=3, native3=True)
    with pytest.raises(ValueError, match="native3"):
        Quant3Linear(128, 64, native3=True)
    with pytest.raises(ValueError, match="STREAM3"):
        ops.packed_words(4, ops.LAYOUT_STREAM3, 16, 256)


def test_packed_state_carries_the_layout_and_old_records_stay_the_container():
    q = QuantLinear(256, 32, bits=3, qfn='b', native3=True)
    q.qweight = torch.arange(q.qweight.numel(), dtype=torch.int32)
    st = q.packed_state()
    assert st["layout"] == ops.LAYOUT_STREAM3
    back = QuantLinear.from_packed_state(st, "cpu")
    assert back.native3 and torch.equal(back.qweight, q.qweight)
    c = QuantLinear(256, 32, bits=3, qfn='b')
    c.qweight = torch.arange(c.qweight.numel(), dtype=torch.int32)
    old = c.packed_state()
    assert old.pop("layout") == ops.LAYOUT_STREAM                 # a record written before the layout existed has no such key
    back = QuantLinear.from_packed_state(old, "cpu")
    assert not back.native3 and back.layout == ops.LAYOUT_STREAM and torch.equal(back.qweight, c.qweight)
    assert back.qweight.numel() == 256 * 32 * 4 // 32


# ---- generated code ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not shutil.which(HIPCC) and not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa") / "dqgemm_w3.s"
    csrc = os.path.join(ROOT, "quip_amd", "csrc")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S",
                           "-I", os.path.join(ROOT, "include"), "-I", csrc, os.path.join(csrc, "dqgemm_w3.hip"), "-o", str(out)],
                          stderr=subprocess.DEVNULL)
    found, cur, body = {}, None, []
    for ln in out.read_text().splitlines():
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            cur, body = m.group(1), []
        elif cur is not None:
            body.append(ln)
            if ".end_amdhsa_kernel" in ln:
                if "dq_w3_kernel" in cur:
                    found[cur] = body
                cur = None
    return found


def test_w3_kernels_no_scratch_no_waterfall_and_compiler_made_field_inserts(kernels):
    assert len(kernels) >= 10, "bf16 and fp16 instantiations of every configuration"
    for name, body in kernels.items():
        text = "\n".join(body)
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", text), f"{name}: scratch"
        ndma = 0
        for i, ln in enumerate(body):
            if "buffer_load_dwordx4" in ln and " lds" in ln:
                ndma += 1
                window = "\n".join(body[max(0, i - 6):i])
                assert "v_readfirstlane_b32" not in window or "s_and_saveexec" not in window, f"{name}: waterfall loop at line {i}"
        assert ndma > 0, f"{name}: no LDS-DMA found"
        # the only inline asm of the kernel: empty statements (opaque constants) and s_waitcnt -- no hand-written loads or VALU
        in_asm = False
        for ln in body:
            s = ln.strip()
            if s.startswith(";;#ASMSTART"):
                in_asm = True
            elif s.startswith(";;#ASMEND"):
                in_asm = False
            elif in_asm and s and not s.startswith(";"):
                assert s.split()[0] == "s_waitcnt", f"{name}: inline asm `{s}`"
        # ONE instruction per field insert (v_bfi_b32, or v_and_or_b32 where the loop-invariant `base & ~mask` is hoisted): 8 to merge the
        # planes + 32 output dwords = 40 per 256-k stage, times the SPW stages a wave's loop body holds (the 58 / 66 VALU of DESIGN.md count
        # the shifts too).  An insert that degraded to v_and + v_or would show up as a missing one here and as extra v_or_b32.
        spw = int(re.search(r"ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E", name).group(3))
        nins = sum(1 for l in body if l.strip().startswith(("v_bfi_b32", "v_and_or_b32")))
        nor = sum(1 for l in body if l.strip().startswith("v_or_b32"))
        assert nins >= 40 * spw, f"{name}: {nins} single-instruction field inserts for {spw} stage(s)"
        assert nor <= 8, f"{name}: {nor} v_or_b32 (field inserts split into and + or?)"
