"""CPU-side checks of the group-wise path: the sixth ABI table (include/quip_amd_groupwise.h <-> _lib.GROUPWISE_SIGNATURES <-> the
library's exports), quipamd_dequant_gemm_groupwise's refusals before any device is touched, and the group-wise QuantLinear's constructor,
pack and checkpoint record on CPU tensors."""
import ctypes
import os
import re

import pytest
import torch

from quip_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE, NULL = ctypes.c_void_p(16), ctypes.c_void_p(0)     # non-null dummy pointers are never dereferenced: the checks come first
NAME = "quipamd_dequant_gemm_groupwise"


def _declared():
    hdr = open(os.path.join(ROOT, "include", "quip_amd_groupwise.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(quipamd_[a-z0-9_]+)\s*\(", hdr)))


def test_every_groupwise_symbol_is_declared_exported_and_bound():
    names = _declared()
    assert names == [NAME]
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/quip_amd_groupwise.h but not exported"
    assert sorted(_lib.GROUPWISE_SIGNATURES) == names
    bound = _lib.load()
    for n in names:
        assert getattr(bound, n).argtypes == _lib.GROUPWISE_SIGNATURES[n]
        assert getattr(bound, n).restype is ctypes.c_int
    assert len(_lib.GROUPWISE_SIGNATURES[NAME]) == 14


def test_the_groupwise_table_is_disjoint_from_the_other_five():
    for other in (_lib.SIGNATURES, _lib.PREFILL_SIGNATURES, _lib.SAMPLE_SIGNATURES, _lib.GENERATE_SIGNATURES, _lib.SCORE_SIGNATURES):
        assert not set(_lib.GROUPWISE_SIGNATURES) & set(other)
    for hdr in ("quip_amd.h", "quip_amd_prefill.h", "quip_amd_sample.h", "quip_amd_generate.h", "quip_amd_score.h"):
        text = open(os.path.join(ROOT, "include", hdr)).read()
        assert not [n for n in _lib.GROUPWISE_SIGNATURES if n in text], hdr


def _call(x=ONE, qw=ONE, gs=ONE, gz=ONE, bias=NULL, y=ONE, x_dtype=1, y_dtype=0, bits=4, G=128, bs=4, m=64, d=256):
    _lib.call(NAME, x, x_dtype, qw, bits, G, gs, gz, bias, y, y_dtype, bs, m, d, NULL)


def test_groupwise_refuses_bad_arguments_without_a_device():
    for name in ("x", "qw", "gs", "gz", "y"):
        with pytest.raises(_lib.QuipAmdError, match="null pointer") as e:
            _call(**{name: NULL})
        assert "code 1" in str(e.value)                                         # QUIPAMD_ERR_ARG
    for bits in (0, 1, 5, 8, -2):
        with pytest.raises(_lib.QuipAmdError, match=r"bits -?\d+ \(2, 3 or 4\)") as e:
            _call(bits=bits)
        assert "code 1" in str(e.value)
    for G in (-1, 0, 16, 48, 96, 256):
        with pytest.raises(_lib.QuipAmdError, match=r"groupsize -?\d+ \(32, 64 or 128\)") as e:
            _call(G=G)
        assert "code 4" in str(e.value)                                         # QUIPAMD_ERR_UNSUPPORTED
    for m in (0, 8, 40, 65):
        with pytest.raises(_lib.QuipAmdError, match="not a multiple of 16") as e:
            _call(m=m)
        assert "code 2" in str(e.value)                                         # QUIPAMD_ERR_SHAPE
    for bits, d in ((2, 128), (2, 384), (4, 64), (4, 192), (3, 64), (3, 320), (4, 0)):
        with pytest.raises(_lib.QuipAmdError, match=r"not a multiple of (128|256) \(512 / bits\)") as e:
            _call(bits=bits, d=d, G=32)
        assert "code 2" in str(e.value)
    for x_dtype in (0, 3, -1):
        with pytest.raises(_lib.QuipAmdError, match="f16 / bf16 only") as e:
            _call(x_dtype=x_dtype)
        assert "code 4" in str(e.value)
    for bs in (0, -3):
        with pytest.raises(_lib.QuipAmdError, match="at least one row") as e:
            _call(bs=bs)
        assert "code 2" in str(e.value)
    for name in ("x", "qw", "gs", "gz", "bias", "y"):
        with pytest.raises(_lib.QuipAmdError, match="16-byte aligned"):
            _call(**{name: ctypes.c_void_p(24)})


def test_ops_dequant_gemm_groupwise_refuses_cpu_tensors():
    from quip_amd import ops
    x = torch.ones(4, 256, dtype=torch.float16)
    qw = torch.zeros(ops.packed_words(4, ops.LAYOUT_STREAM, 64, 256), dtype=torch.int32)
    t = torch.ones(2, 64)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.dequant_gemm_groupwise(x, qw, 4, 128, t, t)
    gs, gz = ops.group_tables(torch.arange(12.).reshape(3, 4), -torch.arange(12.).reshape(3, 4))      # [m, d/G] -> [d/G, m]
    assert gs.shape == (4, 3) and gs.is_contiguous() and gs.dtype == torch.float32 and gs[1, 2] == 9. and gz[3, 0] == -3.


def test_quantlinear_groupwise_refusals():
    from quip_amd import quant
    QL = quant.QuantLinear
    for G in (16, 48, 256, 1):
        with pytest.raises(ValueError, match="groupsize 32, 64 or 128"):
            QL(512, 64, 4, qfn='a', groupsize=G)
    with pytest.raises(ValueError, match="dividing infeatures"):
        QL(320, 64, 4, qfn='a', groupsize=128)                                  # d % G
    with pytest.raises(ValueError, match="qfn 'b'"):
        QL(512, 64, 4, qfn='b', groupsize=128)
    with pytest.raises(ValueError, match="native3"):
        QL(512, 64, 3, qfn='a', native3=True, groupsize=128)
    with pytest.raises(ValueError, match="outfeatures % 16"):
        QL(512, 40, 4, qfn='a', groupsize=128)
    ql = QL(512, 64, 3, qfn='a', groupsize=64)
    assert ql.groupsize == 64 and ql.groupwise and not ql.native3
    assert ql.gscales.shape == ql.gzeros.shape == (8, 64) and ql.gscales.dtype == torch.float32
    assert QL(512, 64, 4, qfn='a').groupsize == -1 and QL(512, 64, 4, qfn='a').gscales is None          # today's layer
    for call in (ql.to_native3, ql.decode_only, ql.decode_qweight):
        with pytest.raises(ValueError, match="group-wise grid"):
            call()
    codes = torch.zeros(64, 512, dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"\[m, d/G\]"):
        ql.pack(codes, torch.ones(64), torch.ones(64))                          # per-row parameters
    with pytest.raises(ValueError, match=r"\[m, d/G\]"):
        ql.pack(codes, torch.ones(64, 4), torch.ones(64, 4))                    # another group size's tables
    with pytest.raises(ValueError, match=r"\[m, d/G\]"):
        ql.pack(codes, torch.ones(64, 8), None)
    ql.half()                                                                   # model.half() must not narrow the tables
    assert ql.gscales.dtype == ql.gzeros.dtype == torch.float32


def test_packed_state_round_trip_on_cpu_keeps_every_buffer():
    from quip_amd import quant, ops
    g = torch.Generator().manual_seed(5)
    ql = quant.QuantLinear(256, 32, 4, qfn='a', groupsize=32)
    ql.qweight = torch.randint(-2 ** 31, 2 ** 31 - 1, ql.qweight.shape, generator=g, dtype=torch.int64).to(torch.int32)
    ql.gscales, ql.gzeros = torch.rand(8, 32, generator=g) + 0.1, torch.rand(8, 32, generator=g) * 15
    ql.scales, ql.zeros = torch.zeros(0), torch.zeros(0)
    ql.bias, ql.inv_scaleWH = torch.randn(32, generator=g), torch.rand(256, generator=g) + 0.5
    st = ql.packed_state()
    assert st["groupsize"] == 32 and st["layout"] == ops.LAYOUT_STREAM
    back = quant.QuantLinear.from_packed_state(st, "cpu")
    assert back.groupsize == 32 and back.groupwise and back.bits == 4 and back.qfn == 'a' and back.U is None and back.V is None
    for name in ("qweight", "gscales", "gzeros", "scales", "zeros", "bias", "inv_scaleWH"):
        a, b = getattr(ql, name), getattr(back, name)
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32) if a.is_floating_point() else a,
                                                                         b.view(torch.int32) if b.is_floating_point() else b), name
    st2 = back.packed_state()
    assert sorted(st2) == sorted(st)


def test_a_record_without_groupsize_is_todays_layer():
    from quip_amd import quant
    ql = quant.QuantLinear(256, 32, 4, qfn='a')
    st = ql.packed_state()
    assert "groupsize" not in st and "gscales" not in st and "gzeros" not in st
    back = quant.QuantLinear.from_packed_state(st, "cpu")
    assert back.groupsize == -1 and not back.groupwise and back.gscales is None and back.gzeros is None
    assert back.scales.shape == (32,) and back.zeros.shape == (32,)
    old = {k: v for k, v in st.items() if k != "layout"}                        # a record from before STREAM3, too
    assert not quant.QuantLinear.from_packed_state(old, "cpu").groupwise


def test_engine_names_groupwise_layers():
    from quip_amd import decode
    assert callable(decode.groupwise_layers)
