"""CPU-side checks of token sampling: Philox4x32-10's known answers, the third ABI table (include/quip_amd_sample.h <->
_lib.SAMPLE_SIGNATURES <-> the library's exports), quipamd_sample_rows' refusals before any device is touched, decode.Sampling, and the
conditions the GPU test relies on, asserted on the very inputs it uses (tests/sample_ref.py)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import sample_ref as R
from quip_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE, NULL = ctypes.c_void_p(16), ctypes.c_void_p(0)     # non-null dummy pointers are never dereferenced: the checks come first


# ---------------------------------------------------------------------------------------------------------------- Philox
KAT = [([0, 0, 0, 0], [0, 0], "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ([0xffffffff] * 4, [0xffffffff] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], "d16cfe09 94fdcceb 5001e420 24126ea1")]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox4x32_10_known_answers(ctr, key, want):
    assert " ".join("%08x" % w for w in R.philox4x32_10(ctr, key)) == want


def test_uniform_uses_seed_counter_and_row_as_the_contract_says():
    seed, ctr, row = 0x299f31d0a4093822, 0x85a308d3243f6a88, 0x13198a2e
    x0 = R.philox4x32_10([0x243f6a88, 0x85a308d3, 0x13198a2e, 0], [0xa4093822, 0x299f31d0])[0]
    assert R.uniform(seed, ctr, row) == (x0 >> 8) * 2.0 ** -24 < 1.0
    counters, rows = [0, 5, (1 << 32) + 7, (1 << 40) + 1], [0, 1, 15, 8191]
    for s in (7, R.SEED):
        got = R.uniforms(s, counters, rows)
        for i, c in enumerate(counters):
            for j, r in enumerate(rows):
                assert got[i, j] == R.uniform(s, c, r)


# ---------------------------------------------------------------------------------------------------------------- ABI
def _declared():
    hdr = open(os.path.join(ROOT, "include", "quip_amd_sample.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(quipamd_[a-z0-9_]+)\s*\(", hdr)))


def test_every_sample_symbol_is_declared_exported_and_bound():
    names = _declared()
    assert names == ["quipamd_sample_rows"]
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/quip_amd_sample.h but not exported"
    assert sorted(_lib.SAMPLE_SIGNATURES) == names
    bound = _lib.load()                                               # load() binds the third table as well
    for n in names:
        assert getattr(bound, n).argtypes == _lib.SAMPLE_SIGNATURES[n] and getattr(bound, n).restype is ctypes.c_int


def test_the_three_tables_are_disjoint():
    assert not set(_lib.SAMPLE_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.PREFILL_SIGNATURES))
    for hdr in ("quip_amd.h", "quip_amd_prefill.h"):
        text = open(os.path.join(ROOT, "include", hdr)).read()
        assert not [n for n in _lib.SAMPLE_SIGNATURES if n in text], hdr  # the other headers do not know the new entry


def test_params_struct_layout():
    from quip_amd import ops
    S = ops.SampleParams
    assert ctypes.sizeof(S) == ops.SAMPLE_PARAMS_BYTES == 24
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [("temperature", 0), ("top_p", 4), ("top_k", 8), ("reserved", 12), ("seed", 16)]
    raw = ops._sample_params_host(0.75, 50, 0.9, 0xfedcba9876543210).numpy().tobytes()
    assert np.frombuffer(raw[:8], np.float32).tolist() == [0.75, float(np.float32(0.9))]
    assert np.frombuffer(raw[8:16], np.int32).tolist() == [50, 0] and int(np.frombuffer(raw[16:], np.uint64)[0]) == 0xfedcba9876543210


def _call(logits=ONE, dtype=1, rows=2, n=100, ld=100, params=ONE, counter=ONE, out=ONE, clear=NULL, clear_n=0):
    _lib.call("quipamd_sample_rows", logits, dtype, rows, n, ld, params, counter, out, NULL, NULL, NULL, clear, clear_n, NULL)


def test_sample_rows_refuses_bad_arguments_without_a_device():
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
    with pytest.raises(_lib.QuipAmdError, match="bad shape") as e:
        _call(ld=99)
    assert "code 2" in str(e.value)
    for rows in (-1, 65536):
        with pytest.raises(_lib.QuipAmdError, match="bad shape"):
            _call(rows=rows)
    for cn in (0, -4):
        with pytest.raises(_lib.QuipAmdError, match="clear_n") as e:
            _call(clear=ONE, clear_n=cn)
        assert "code 1" in str(e.value)
    _call(rows=0)                                                     # nothing to do: no launch, no error
    _call(rows=0, n=262144, ld=262144, dtype=0)


def test_ops_sample_rows_refuses_cpu_tensors():
    from quip_amd import ops
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.sample_rows(torch.zeros(2, 8), torch.zeros(24, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.write_sample_params(torch.zeros(24, dtype=torch.uint8), 1.0)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.sample_params(0.7, device="cpu")


# ---------------------------------------------------------------------------------------------------------------- decode.Sampling
def test_sampling_is_a_validated_value():
    from quip_amd import decode
    S = decode.Sampling
    s = S(0.8, top_p=0.95)
    assert (s.temperature, s.top_k, s.top_p, s.seed) == (0.8, 0, 0.95, 0)
    assert S() == S(1.0, 0, 1.0, 0) and S(0.5, 3, 0.25, 9) == S(temperature=0.5, top_k=3, top_p=0.25, seed=9) and S(0.5) != S(0.6)
    assert hash(S(0.5, 3)) == hash(S(0.5, 3)) and S(seed=1) != S(seed=2) and S() != "Sampling"
    assert S(0).temperature == 0.0 and S(seed=(1 << 64) - 1).seed == (1 << 64) - 1 and S(top_k=np.int64(5)).top_k == 5
    for bad in (dict(temperature=-0.1), dict(temperature=float("nan")), dict(temperature=float("inf")), dict(temperature="hot"),
                dict(top_p=0.0), dict(top_p=-0.5), dict(top_p=1.0001), dict(top_p=float("nan")),
                dict(top_k=-1), dict(top_k=2.5), dict(top_k=True),
                dict(seed=1.0), dict(seed="7"), dict(seed=None), dict(seed=1 << 64), dict(seed=-1)):
        with pytest.raises(ValueError, match="Sampling"):
            S(**bad)
    with pytest.raises(AttributeError):
        s.temperature = 2.0


def test_engine_sampling_api_is_there():
    from quip_amd import decode
    assert callable(decode.DecodeEngine.set_sampling)
    assert "sampling" in inspect.signature(decode.DecodeEngine.generate).parameters
    assert inspect.signature(decode.DecodeEngine.generate).parameters["sampling"].default is None


# ---------------------------------------------------------------------------------------------------------------- the oracle on the GPU test's inputs
def _us():
    return R.uniforms(R.SEED, R.COUNTER0 + np.arange(R.COUNTERS), np.arange(R.ROWS)).ravel()


@pytest.mark.parametrize("case", R.SHARP, ids=lambda c: "-".join(str(v) for v in c))
def test_sharp_inputs_leave_few_draws_ambiguous(case):
    """on these inputs at most 2 % of the 2048 draws have more than one acceptable token at delta = 3e-5: the GPU test's "every token is
    acceptable" is then nearly "every token is THE token"; and the oracle accepts its own draws"""
    n, scale, T, k, p, dt = case
    o = R.Oracle(R.values(R.make_logits(n, scale, dt)), T, k, p)
    u = _us()
    lo, hi = o.bounds(u)
    share = float(np.mean(hi > lo))
    print(f"{case}: {100 * share:.2f} % ambiguous, kept_n {o.kept_n} in [{o.n_lo}, {o.n_hi}], kept_mass {o.kept_mass:.5f}")
    assert share <= 0.02
    assert o.accepts(u, o.draw(u)).all() and o.n_lo <= o.kept_n <= o.n_hi
    assert (o.bounds(u, 0.0)[0] == o.bounds(u, 0.0)[1]).all()         # delta 0: exactly one
    assert np.array_equal(o.survivors[o.bounds(u, 0.0)[0]], o.draw(u))


def test_flat_input_is_why_only_its_sandwich_is_checked():
    n, scale, T, k, p, dt = R.FLAT
    o = R.Oracle(R.values(R.make_logits(n, scale, dt)), T, k, p)
    lo, hi = o.bounds(_us())
    print(f"flat: kept_n {o.kept_n} in [{o.n_lo}, {o.n_hi}]; {100 * float(np.mean(hi > lo)):.1f} % of the draws have several acceptable tokens")
    assert o.n_lo < o.kept_n < o.n_hi and o.n_hi - o.n_lo < 40
    assert float(np.mean(hi > lo)) > 0.2


def test_oracle_on_hand_made_rows():
    inf = float("inf")
    o = R.Oracle([0.0] * 16, 1.0, 0, 0.5)                             # p = 1/16 each: the mass before entry j is j/16 < 0.5 for j < 8
    assert o.kept_n == 8 and o.survivors.tolist() == list(range(8)) and o.kept_mass == 0.5
    o = R.Oracle([1.0, 3.0, 3.0, -inf, 3.0, 1.0], 1.0, 2, 1.0)        # ties at the top-k cut go to the smaller indices
    assert o.survivors.tolist() == [1, 2] and o.kept_n == 2 and o.kept_mass == 1.0
    assert o.draw(0.49).item() == 1 and o.draw(0.5).item() == 2
    o = R.Oracle([-inf, 2.0, -inf], 0.5)
    assert o.survivors.tolist() == [1] and o.logprob(1) == 0.0 and o.draw(0.999).item() == 1
