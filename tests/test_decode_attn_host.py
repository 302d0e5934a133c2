"""CPU-side checks of the fused decode attention's context limit: quipamd_decode_attention_fused_max_len is the LDS rule of
csrc/decode_attn.hip (restated below), the launch refuses a longer cache before touching a device, and the decode engine's mode choice
keeps a cache that no form of the launch holds off mode v3."""
import ctypes
import types

import pytest
import torch

from quip_amd import _lib

ONE, NULL = ctypes.c_void_p(16), ctypes.c_void_p(0)     # non-null dummy pointers are never dereferenced: the checks come first
LDS_MAX = 160 * 1024                                    # dynamic LDS a gfx950 workgroup may hold
SHAPES = [(64, 64, 32), (128, 64, 64), (128, 64, 32)]   # (head_dim, p, q) of the three instantiations


def fused_attention_lds(hd, p, q, maxlen, three_heads):
    """bytes of LDS of one workgroup of the fused attention launch: three operator images (PassDims<p, q, 4>) and the attention buffers
    (q / k / v slices, scores [maxlen], reductions, partial outputs) of one wave group, or of three when a workgroup serves three heads"""
    image = q * (p + 8) * 2 + p * (q + 8) * 2 + p * (q + 4) * 4
    group = (3 * hd * 2 + 32 + (maxlen + 8 + 4 * hd) * 4 + 15) & ~15
    return 3 * image + (3 if three_heads else 1) * group


def form_max_len(hd, p, q, three_heads):
    """the largest maxlen (at most the launch's 32768) whose LDS fits one workgroup, by the rule above"""
    lo, hi = 0, 32768
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if fused_attention_lds(hd, p, q, mid, three_heads) <= LDS_MAX:
            lo = mid
        else:
            hi = mid - 1
    return lo


def _fused_call(hd, p, q, maxlen, heads=None):
    from quip_amd import ops
    heads = heads or p * q // hd
    fops = (ops.Fop * 3)(*[ops.Fop(16, 16, 16, 16, p, q) for _ in range(3)])
    ptrs = (ctypes.c_void_p * 3)(16, 16, 16)
    _lib.call("quipamd_decode_attention_fused", ctypes.cast(fops, ctypes.c_void_p), ctypes.cast(ptrs, ctypes.c_void_p),
              ctypes.cast(ptrs, ctypes.c_void_p), ONE, ONE, ONE, ONE, NULL, NULL, 0, 2, heads, hd, maxlen, ctypes.c_float(0.1), heads * hd,
              NULL)


def test_max_len_is_positive_for_the_served_shapes_only():
    from quip_amd import ops
    for hd, p, q in SHAPES:
        assert ops.decode_attention_fused_max_len(hd, p, q) > 4096
    for hd, p, q in [(64, 64, 64), (128, 128, 64), (96, 64, 32), (64, 32, 32), (0, 64, 32), (-128, 64, 64)]:
        assert ops.decode_attention_fused_max_len(hd, p, q) == 0


def test_max_len_follows_the_lds_rule():
    """the query is the one-head form's limit (the three-heads form falls back to it past its own); the rule gives the limits DESIGN.md
    states, and one position more no longer fits"""
    from quip_amd import ops
    want = {(128, 64, 64): (3972, 13360), (64, 64, 32): (8548, 26384), (128, 64, 32): (8196, 26032)}
    for hd, p, q in SHAPES:
        one, three = form_max_len(hd, p, q, False), form_max_len(hd, p, q, True)
        assert (three, one) == want[(hd, p, q)]
        assert ops.decode_attention_fused_max_len(hd, p, q) == one
        for mh, lim in ((False, one), (True, three)):
            assert fused_attention_lds(hd, p, q, lim, mh) <= LDS_MAX < fused_attention_lds(hd, p, q, lim + 1, mh)


def test_launch_refuses_a_cache_past_the_limit_without_a_device():
    from quip_amd import ops
    for hd, p, q in SHAPES:
        cap = ops.decode_attention_fused_max_len(hd, p, q)
        with pytest.raises(_lib.QuipAmdError, match="LDS") as e:
            _fused_call(hd, p, q, cap + 1)
        assert "code 2" in str(e.value)                               # QUIPAMD_ERR_SHAPE
    with pytest.raises(_lib.QuipAmdError) as e:
        _fused_call(96, 64, 32, 64, heads=21)                         # 21 x 96 = 2016: not the operator's 2048
    assert "code 2" in str(e.value)
    with pytest.raises(_lib.QuipAmdError, match="head_dim 64 with a 64 x 64") as e:
        _fused_call(64, 64, 64, 64)                                   # a shape no instantiation serves: unsupported, whatever the maxlen
    assert "code 4" in str(e.value)


def _llama_v3_stub(h, heads, maxpos, monkeypatch):
    """a one-block LlamaDecoder whose seven projections stand for packed layers with the operator shape hidden size h gets, and every
    condition of mode v3 but the attention launch's granted"""
    from quip_amd import decode
    pq = {2048: (64, 32), 4096: (64, 64)}[h]
    lin = [types.SimpleNamespace(U=types.SimpleNamespace(p=pq[0], q=pq[1], fused_ok=True), outfeatures=h) for _ in range(7)]
    norm = lambda: decode.RMSNorm(h, 1e-5, torch.float16)
    blk = decode.LlamaBlock(norm(), *lin[:4], norm(), *lin[4:], heads)
    monkeypatch.setattr(decode, "fused_ok", lambda *a, **k: True)
    monkeypatch.setattr(decode, "bigp_tail_ok", lambda *a, **k: True)
    monkeypatch.setattr(decode.LlamaDecoder, "packed", lambda self: True)
    monkeypatch.setattr(decode.LlamaDecoder, "head_ok", lambda self, bs: False)
    dec = decode.LlamaDecoder(torch.nn.Embedding(8, h), [blk], norm(), torch.nn.Linear(h, 8, bias=False), heads, torch.ones(h // heads // 2), maxpos)
    return dec, lin[:3]


def test_mode_choice_checks_the_real_maxlen(monkeypatch):
    """fused_attention_ok bounds the cache's maxlen by the query; LlamaDecoder.v3_ok checks the maxlen it is given, its rotary tables' rows
    by default (it used to ask about a cache of ONE position: a 64 x 64 Llama at max_len 16384 got mode v3 and failed on its first step);
    best_mode passes the engine's max_len, so such a cache gets mode `fused`"""
    from quip_amd import decode, ops, quant
    dec, qkv = _llama_v3_stub(4096, 32, 16384, monkeypatch)
    cap = ops.decode_attention_fused_max_len(128, 64, 64)
    kc = lambda n: torch.empty((9, 32, n, 128), dtype=torch.float16, device='meta')
    assert quant.fused_attention_ok(qkv, kc(4096)) and quant.fused_attention_ok(qkv, kc(cap))
    assert not quant.fused_attention_ok(qkv, kc(cap + 1)) and not quant.fused_attention_ok(qkv, kc(16384))
    assert dec.v3_ok(9, cap) and dec.v3_ok(16, 4096) and not dec.v3_ok(9, cap + 1)
    assert not dec.v3_ok(1)                                           # default: the rotary tables' 16384 rows
    assert decode.best_mode(dec, 1, torch.float16, 16384) == "fused" and decode.best_mode(dec, 9, torch.float16, 4096) == "v3"
    assert decode.best_mode(dec, 9, torch.float16, cap) == "v3" and decode.best_mode(dec, 9, torch.float16, cap + 1) == "fused"
    assert decode.best_mode(dec, 1, torch.float16) == "fused"         # no max_len: the decoder's own context
    dec4k, _ = _llama_v3_stub(4096, 32, 4096, monkeypatch)
    assert dec4k.v3_ok(16) and decode.best_mode(dec4k, 16, torch.float16) == "v3"
    small, _ = _llama_v3_stub(2048, 16, 32768, monkeypatch)
    cap2 = ops.decode_attention_fused_max_len(128, 64, 32)
    assert small.v3_ok(17, cap2) and not small.v3_ok(17, cap2 + 1) and not small.v3_ok(17)
