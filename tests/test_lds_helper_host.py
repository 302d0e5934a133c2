"""The launch convention of csrc/ (DESIGN.md section 3), checked on the sources: the dynamic-LDS limit of a kernel is raised through qa_lds<>
in common.h and nowhere else, and the two sizes it turns on have one name each.  What a new kernel family must not bring back: its own
hipFuncSetAttribute call, its own per-device cache, its own spelling of 64 KiB or 160 KiB."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "quip_amd", "csrc")


def _sources():
    paths = sorted(p for ext in ("*.hip", "*.h", "*.inc") for p in glob.glob(os.path.join(CSRC, ext)))
    assert len(paths) > 30 and any(p.endswith("common.h") for p in paths)
    return {os.path.basename(p): open(p).read() for p in paths}


def test_the_lds_attribute_is_raised_in_common_h_only():
    src = _sources()
    for name in ("hipFuncSetAttribute", "hipFuncAttributeMaxDynamicSharedMemorySize"):
        assert [f for f, text in src.items() if name in text] == ["common.h"], name
    assert "template <auto Kern> int qa_lds(size_t lds, const char *who)" in src["common.h"]
    for gone in ("QaPerDevice", "reserved[64]", "raised[64]", "attr_set[64]"):         # the per-site caches the helper replaced
        assert [f for f, text in src.items() if gone in text] == [], gone


def test_the_lds_sizes_are_named():
    """160 * 1024 is written once, where QA_LDS_MAX is defined; 64 * 1024 is compared with an LDS size nowhere (QA_LDS_DEFAULT is)"""
    big, dflt = re.compile(r"160\s*\*\s*1024"), re.compile(r"(?<!\d)64\s*\*\s*1024")
    for f, text in _sources().items():
        for ln in text.splitlines():
            if big.search(ln):
                assert f == "common.h" and ln.startswith("constexpr size_t QA_LDS_MAX = 160 * 1024;"), (f, ln)
            if dflt.search(ln) and "lds" in ln.lower() and re.search(r"[<>]", ln):
                assert False, (f, ln)
