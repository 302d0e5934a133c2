"""CPU-side checks of the prompt pass: the second ABI table (include/quip_amd_prefill.h <-> _lib.PREFILL_SIGNATURES <-> the library's
exports), quipamd_prefill_attention's refusals before any device is touched, and the kernel's arithmetic -- restated in torch
(tests/prefill_ref.py: fp32 scores, online softmax over 64-position tiles, P rounded to the 16-bit type) -- against fp64 causal
attention under the attention gate of the decode tests."""
import ctypes
import os
import re

import pytest
import torch

import prefill_ref as R
from quip_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE, NULL = ctypes.c_void_p(16), ctypes.c_void_p(0)     # non-null dummy pointers are never dereferenced: the checks come first


def _declared():
    hdr = open(os.path.join(ROOT, "include", "quip_amd_prefill.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(quipamd_[a-z0-9_]+)\s*\(", hdr)))


def test_every_prefill_symbol_is_declared_exported_and_bound():
    names = _declared()
    assert "quipamd_prefill_attention" in names
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/quip_amd_prefill.h but not exported"
        assert n in _lib.PREFILL_SIGNATURES, f"{n} has no ctypes signature in quip_amd/_lib.py"
    assert sorted(_lib.PREFILL_SIGNATURES) == names
    bound = _lib.load()                                               # load() binds the second table as well
    for n in names:
        assert getattr(bound, n).argtypes == _lib.PREFILL_SIGNATURES[n]


def test_the_two_tables_are_disjoint():
    assert not set(_lib.PREFILL_SIGNATURES) & set(_lib.SIGNATURES)
    main = open(os.path.join(ROOT, "include", "quip_amd.h")).read()
    assert not [n for n in _lib.PREFILL_SIGNATURES if n in main]     # the frozen header does not know the new entries


def _call(T=8, heads=32, kv_heads=8, hd=128, maxlen=512, q=ONE, start=ONE, out=ONE, dtype=1, ldq=None, ldk=None, ldv=None, tables=(NULL, NULL),
          bs=2):
    ldq = heads * hd if ldq is None else ldq
    ldk = kv_heads * hd if ldk is None else ldk
    ldv = kv_heads * hd if ldv is None else ldv
    _lib.call("quipamd_prefill_attention", q, ONE, ONE, ONE, ONE, start, T, out, tables[0], tables[1], 64, dtype, bs, heads, kv_heads, hd,
              maxlen, ctypes.c_float(0.1), ldq, ldk, ldv, NULL)


def test_prefill_attention_refuses_bad_arguments_without_a_device():
    with pytest.raises(_lib.QuipAmdError, match="null pointer") as e:
        _call(q=NULL)
    assert "code 1" in str(e.value)                                   # QUIPAMD_ERR_ARG
    with pytest.raises(_lib.QuipAmdError, match="null pointer"):
        _call(start=NULL)
    with pytest.raises(_lib.QuipAmdError, match="null pointer"):
        _call(out=NULL)
    for hd in (16, 96, 256):
        with pytest.raises(_lib.QuipAmdError, match="head_dim") as e:
            _call(hd=hd)
        assert "code 4" in str(e.value)                               # QUIPAMD_ERR_UNSUPPORTED
    with pytest.raises(_lib.QuipAmdError, match="not a multiple of kv_heads") as e:
        _call(heads=12, kv_heads=8)
    assert "code 2" in str(e.value)                                   # QUIPAMD_ERR_SHAPE
    with pytest.raises(_lib.QuipAmdError, match="group size 32"):
        _call(heads=64, kv_heads=2)
    for name in ("ldq", "ldk", "ldv"):
        with pytest.raises(_lib.QuipAmdError, match="row strides"):
            _call(**{name: 32 * 128 + 4})                             # not a multiple of 8
    with pytest.raises(_lib.QuipAmdError, match="row strides"):
        _call(ldk=8 * 128 - 8)                                        # shorter than a row
    for T in (0, -3):
        with pytest.raises(_lib.QuipAmdError, match="at least one new position"):
            _call(T=T)
    with pytest.raises(_lib.QuipAmdError, match="maxlen"):
        _call(maxlen=32769)
    with pytest.raises(_lib.QuipAmdError, match="f16 / bf16"):
        _call(dtype=0)
    with pytest.raises(_lib.QuipAmdError, match="16-byte aligned"):
        _call(q=ctypes.c_void_p(18))
    with pytest.raises(_lib.QuipAmdError, match="rotary tables"):
        _call(tables=(ONE, NULL))
    _call(bs=0)                                                       # nothing to do: no launch, no error
    _call(heads=8, kv_heads=8, bs=0)                                  # multi-head (g = 1) is served by the same entry


def test_ops_prefill_attention_refuses_cpu_tensors():
    from quip_amd import ops
    x = torch.ones(4, 256, dtype=torch.float16)
    c = torch.ones(1, 2, 8, 128, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.prefill_attention(x, x, x, c, c, torch.tensor([0]), 4)


def test_engine_prefill_api_is_there():
    from quip_amd import decode
    for cls in (decode.OPTBlock, decode.LlamaBlock, decode.OPTDecoder, decode.LlamaDecoder, decode.DecodeEngine):
        assert callable(getattr(cls, "prefill"))
    assert callable(decode.DecodeEngine.perplexity) and callable(decode.perplexity)


def test_rope_restatement_is_hf_rotate_half():
    """tests/prefill_ref.rope (rope_kernel's expression) against HF's apply_rotary_pos_emb form x * cos + rotate_half(x) * sin in fp64"""
    hd, T, start, nh = 64, 9, 5, 3
    cos, sin = R.tables(hd, 32)
    x = torch.randn(2 * T, nh * hd, generator=torch.Generator().manual_seed(0))
    got = R.rope(x, cos, sin, start, T, nh).double().view(2, T, nh, hd)
    xd = x.double().view(2, T, nh, hd)
    rot = torch.cat((-xd[..., hd // 2:], xd[..., :hd // 2]), -1)
    want = xd * cos[start:start + T].double().view(1, T, 1, hd) + rot * sin[start:start + T].double().view(1, T, 1, hd)
    assert (got - want).abs().max().item() < 1e-5


# (start, T): from the first token to a full second half of a 4096 context, aligned and unaligned starts, ragged ends
MODEL_CASES = ([(hd, s, T) for hd in (64, 128) for s, T in [(0, 1), (0, 17), (0, 64), (0, 65), (0, 300), (37, 100), (511, 1), (63, 2), (1000, 24)]]
               + [(128, 2048, 2048)])                                 # (one head at the long case: CPU time)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("hd,start,T", MODEL_CASES)
def test_kernel_arithmetic_model_against_fp64_under_the_attention_gate(dtype, hd, start, T):
    """what the kernel computes -- with the 16-bit P -- has room under the gate the decode attention tests use (its measured worst case
    here: under 0.3 of the gate for either type), so the GPU test of the op can keep that gate as it is"""
    big = T >= 2048
    bs, kv, g = (1, 1, 1) if big else (2, 2, 2)
    gen = torch.Generator().manual_seed(start + T + hd)
    mk = lambda *s: torch.randn(*s, generator=gen).to(dtype)
    n = start + T
    q, kc, vc = mk(bs * T, kv * g * hd), mk(bs, kv, n, hd), mk(bs, kv, n, hd)
    want = R.causal_fp64(q, kc, vc, start, T, g)
    got = R.kernel_model(q, kc, vc, start, T, g)
    ok, frac = R.within_gate(got, want, dtype)
    print(f"{dtype} hd {hd} start {start} T {T}: {frac:.3f} of the gate")
    assert ok, frac
