"""CPU-side checks of generation control: the fourth ABI table (include/quip_amd_generate.h <-> _lib.GENERATE_SIGNATURES <-> the library's
exports), the parameter struct's layout against the C compiler's, quipamd_generate_rows' refusals before any device is touched,
decode.Generation, and the reference helpers of the GPU tests (tests/generate_ref.py) on hand-made rows."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import generate_ref as GR
from quip_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE, NULL = ctypes.c_void_p(16), ctypes.c_void_p(0)     # non-null dummy pointers are never dereferenced: the checks come first
OTHER_HEADERS = ("quip_amd.h", "quip_amd_prefill.h", "quip_amd_sample.h")


# ---------------------------------------------------------------------------------------------------------------- ABI
def _declared():
    hdr = open(os.path.join(ROOT, "include", "quip_amd_generate.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(quipamd_[a-z0-9_]+)\s*\(", hdr)))


def test_every_generate_symbol_is_declared_exported_and_bound():
    names = _declared()
    assert names == ["quipamd_generate_rows"]
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/quip_amd_generate.h but not exported"
    assert sorted(_lib.GENERATE_SIGNATURES) == names
    bound = _lib.load()                                               # load() binds the fourth table as well
    for n in names:
        assert getattr(bound, n).argtypes == _lib.GENERATE_SIGNATURES[n] and getattr(bound, n).restype is ctypes.c_int


def test_the_four_tables_are_disjoint():
    others = set(_lib.SIGNATURES) | set(_lib.PREFILL_SIGNATURES) | set(_lib.SAMPLE_SIGNATURES)
    assert not set(_lib.GENERATE_SIGNATURES) & others
    for hdr in OTHER_HEADERS:
        text = open(os.path.join(ROOT, "include", hdr)).read()
        assert not [n for n in _lib.GENERATE_SIGNATURES if n in text], hdr   # the other headers do not know the new entry


def test_the_prototype_has_as_many_arguments_as_the_table():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "quip_amd_generate.h")).read(), flags=re.S)
    proto = re.search(r"int\s+quipamd_generate_rows\s*\((.*?)\)\s*;", hdr, flags=re.S).group(1)
    args = [a.strip() for a in proto.split(",")]
    table = _lib.GENERATE_SIGNATURES["quipamd_generate_rows"]
    assert len(args) == len(table) == 23
    for a, t in zip(args, table):                                     # pointers are void pointers, `int` is c_int, int64_t is c_int64
        want = ctypes.c_void_p if "*" in a else ctypes.c_int64 if a.startswith("int64_t") else ctypes.c_int
        assert t is want, (a, t)


def test_params_struct_layout_is_the_c_compilers(tmp_path):
    from quip_amd import ops
    P = ops.GenerateParams
    fields = ["temperature", "top_p", "top_k", "repetition_penalty", "seed"]
    assert [n for n, _ in P._fields_] == fields
    assert ctypes.sizeof(P) == ops.GENERATE_PARAMS_BYTES == 24 and ops.GENERATE_PARAMS_BYTES % 8 == 0
    assert [(n, getattr(P, n).offset) for n in fields] == [("temperature", 0), ("top_p", 4), ("top_k", 8), ("repetition_penalty", 12), ("seed", 16)]
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "the oracle's build needs a C compiler as well"
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "quip_amd_generate.h"\nint main(void) {\n'
                   '    printf("%zu", sizeof(quipamd_generate_params));\n'
                   + "".join(f'    printf(" %zu", offsetof(quipamd_generate_params, {n}));\n' for n in fields)
                   + '    printf(" %d", QUIPAMD_GENERATE_MAX_STOP);\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(P)] + [getattr(P, n).offset for n in fields] + [ops.GENERATE_MAX_STOP]
    raw = ops._generate_params_host(0.75, 50, 0.9, 0xfedcba9876543210, 1.3)
    assert np.frombuffer(raw[:8], np.float32).tolist() == [0.75, float(np.float32(0.9))]
    assert np.frombuffer(raw[8:12], np.int32).tolist() == [50] and np.frombuffer(raw[12:16], np.float32)[0] == np.float32(1.3)
    assert int(np.frombuffer(raw[16:], np.uint64)[0]) == 0xfedcba9876543210


def _call(logits=ONE, dtype=1, rows=2, n=100, ld=100, params=ONE, counter=ONE, hist=NULL, hist_cap=0, ld_hist=0, fed=NULL, stop_ids=NULL, n_stop=0,
          pad_id=0, done=NULL, stop_pos=NULL, out=ONE, clear=NULL, clear_n=0):
    _lib.call("quipamd_generate_rows", logits, dtype, rows, n, ld, params, counter, hist, hist_cap, ld_hist, fed, stop_ids, n_stop, pad_id, done,
              stop_pos, out, NULL, NULL, NULL, clear, clear_n, NULL)


def test_generate_rows_refuses_bad_arguments_without_a_device():
    for name in ("logits", "params", "counter", "out"):
        with pytest.raises(_lib.QuipAmdError, match="null pointer") as e:
            _call(**{name: NULL})
        assert "code 1" in str(e.value)                               # QUIPAMD_ERR_ARG
    for dt in (3, -1, 7):
        with pytest.raises(_lib.QuipAmdError, match="bad dtype") as e:
            _call(dtype=dt)
        assert "code 1" in str(e.value)
    for n in (0, 262145, -5):
        with pytest.raises(_lib.QuipAmdError, match="bad shape") as e:
            _call(n=n, ld=max(n, 1))
        assert "code 2" in str(e.value)                               # QUIPAMD_ERR_SHAPE
    with pytest.raises(_lib.QuipAmdError, match="bad shape"):
        _call(ld=99)
    for rows in (-1, 65536):
        with pytest.raises(_lib.QuipAmdError, match="bad shape"):
            _call(rows=rows)
    for cn in (0, -4):
        with pytest.raises(_lib.QuipAmdError, match="clear_n") as e:
            _call(clear=ONE, clear_n=cn)
        assert "code 1" in str(e.value)
    for ns in (17, -1, 1 << 40):
        with pytest.raises(_lib.QuipAmdError, match="n_stop") as e:
            _call(stop_ids=ONE, n_stop=ns)
        assert "code 1" in str(e.value)
    for cap, ldh in ((0, 8), (-3, 8), (8, 7), (1 << 31, 1 << 31)):
        with pytest.raises(_lib.QuipAmdError, match="hist_cap") as e:
            _call(hist=ONE, hist_cap=cap, ld_hist=ldh)
        assert "code 2" in str(e.value)
    for pad in (-1, 1 << 31):
        with pytest.raises(_lib.QuipAmdError, match="pad_id"):
            _call(pad_id=pad)
    _call(rows=0)                                                     # nothing to do: no launch, no error
    _call(rows=0, n=262144, ld=262144, dtype=0, hist=ONE, hist_cap=4, ld_hist=4, stop_ids=ONE, n_stop=16, done=ONE, stop_pos=ONE, fed=ONE)


def test_ops_refuse_cpu_tensors():
    from quip_amd import ops
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.generate_rows(torch.zeros(2, 8), torch.zeros(2, 24, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.write_generate_params(torch.zeros(2, 24, dtype=torch.uint8), 0, 1.0)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.generate_params(2, device="cpu")


# ---------------------------------------------------------------------------------------------------------------- decode.Generation
def test_generation_is_a_validated_value():
    from quip_amd import decode
    G, S = decode.Generation, decode.Sampling
    g = G()
    assert (g.sampling, g.repetition_penalty, g.stop_ids, g.pad_id) == (None, 1.0, (), 0)
    assert g.rows(3) == [(0.0, 0, 1.0, 0, 1.0)] * 3                   # no Sampling: greedy rows
    s = S(0.8, top_k=5, top_p=0.9, seed=7)
    g = G(s, 1.25, [2, 50], pad_id=1)
    assert g == G(sampling=S(0.8, 5, 0.9, 7), repetition_penalty=1.25, stop_ids=(2, 50), pad_id=1) and hash(g) == hash(G(s, 1.25, (2, 50), 1))
    assert g != G(s, 1.25, [2, 51], 1) and g != G(s, 1.3, [2, 50], 1) and g != G(None, 1.25, [2, 50], 1) and g != G(s, 1.25, [2, 50], 0) and g != "g"
    assert g.rows(2) == [(0.8, 5, 0.9, 7, 1.25)] * 2
    per = G([S(0.5, seed=1), S(0.0), S(1.5, top_k=3, seed=2)], [1.0, 1.1, 2], stop_ids=np.array([4]).tolist())
    assert per.rows(3) == [(0.5, 0, 1.0, 1, 1.0), (0.0, 0, 1.0, 0, 1.1), (1.5, 3, 1.0, 2, 2.0)]
    assert G(stop_ids=range(16)).stop_ids == tuple(range(16)) and G(repetition_penalty=np.float32(0.5)).repetition_penalty == 0.5
    for bad in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.2), dict(repetition_penalty=float("nan")),
                dict(repetition_penalty=float("inf")), dict(repetition_penalty="strong"), dict(repetition_penalty=None),
                dict(repetition_penalty=True), dict(repetition_penalty=[1.0, 0.0]), dict(repetition_penalty=[]),
                dict(stop_ids=range(17)), dict(stop_ids=[-1]), dict(stop_ids=[2.5]), dict(stop_ids=[1 << 31]), dict(stop_ids=7),
                dict(pad_id=-1), dict(pad_id=1.0), dict(pad_id=None), dict(pad_id=1 << 31),
                dict(sampling="greedy"), dict(sampling=0.7), dict(sampling=[]), dict(sampling=[S(), None]),
                dict(sampling=[S(), S()], repetition_penalty=[1.0, 1.1, 1.2])):
        with pytest.raises(ValueError, match="Generation"):
            G(**bad)
    for wrong in (per, G([S()] * 2), G(repetition_penalty=[1.0] * 5)):  # per-sequence settings of the wrong length for 4 sequences
        with pytest.raises(ValueError, match="Generation"):
            wrong.rows(4)
    with pytest.raises(AttributeError):
        g.pad_id = 3
    with pytest.raises(AttributeError):
        g.stop_ids = ()


def test_engine_generation_api_is_there():
    from quip_amd import decode
    E = decode.DecodeEngine
    assert callable(E.set_generation) and E.poll == 8
    params = inspect.signature(E.generate).parameters
    assert list(params) == ["self", "first", "n", "sampling", "generation"] and params["generation"].default is None
    assert list(inspect.signature(decode.Generation.__init__).parameters) == ["self", "sampling", "repetition_penalty", "stop_ids", "pad_id"]


# ---------------------------------------------------------------------------------------------------------------- the reference helpers
def test_penalise_on_hand_made_rows():
    inf, nan = float("inf"), float("nan")
    x = np.array([2.0, -2.0, 0.0, -0.0, -inf, inf, nan, 3.0, -3.0], dtype=np.float32)
    got = GR.penalise(x, [0, 1, 1, 1, 2, 3, 4, 5, 6, -1, 9, 100, 0], 2.0)        # duplicates count once; -1, 9 and 100 are outside
    assert got.dtype == np.float32 and got[:3].tolist() == [1.0, -4.0, 0.0] and np.signbit(got[3]) and got[3] == 0
    assert got[4] == -inf and got[5] == inf and np.isnan(got[6]) and got[7:].tolist() == [3.0, -3.0]
    assert x[0] == 2.0                                                           # a copy
    assert np.array_equal(GR.penalise(x, [], 1.7), x, equal_nan=True) and np.array_equal(GR.penalise(x, [7, 8], 1.0), x, equal_nan=True)
    assert GR.penalise(np.array([7.0], np.float32), [0], 1.3)[0] == np.float32(7.0) / np.float32(1.3)      # a division, in fp32
    rows = GR.penalise_rows(np.ones((2, 4), np.float32), np.array([[0, 1, 2], [3, 3, 3]]), [2, 0], [2.0, 2.0])
    assert rows.tolist() == [[0.5, 0.5, 1, 1], [1, 1, 1, 1]]


def test_stop_bookkeeping_on_hand_made_runs():
    out, done, pos = GR.stop_step([5, 9, 7], [0, 1, 0], [-1, 3, -1], {7, 9}, 4, 0)
    assert (out, done, pos) == ([5, 0, 7], [0, 1, 1], [-1, 3, 4])
    plain = [[1, 2], [3, 9], [9, 4], [5, 6]]
    toks, lengths, first = GR.trim(plain, {9}, 0)
    assert toks.tolist() == [[1, 2], [3, 9], [9, 0]] and lengths == [3, 2] and first == [2, 1]
    toks, lengths, first = GR.trim(plain, {6, 1}, 8)
    assert toks.tolist() == [[1, 2], [8, 9], [8, 4], [8, 6]] and lengths == [1, 4] and first == [0, 3]
    toks, lengths, first = GR.trim(plain, {3}, 0)                                # one sequence never stops: all n steps
    assert toks.tolist() == [[1, 2], [3, 9], [0, 4], [0, 6]] and lengths == [2, 4] and first == [1, None]
    toks, lengths, first = GR.trim(plain, set(), 0)
    assert toks.tolist() == plain and lengths == [4, 4]
