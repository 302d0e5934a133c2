"""CPU-side checks of grouped-query attention: quipamd_decode_attention_grouped refuses what it cannot serve before touching a
device, and decoder_from_hf binds a grouped-query Llama over the model's own modules (or refuses it at construction)."""
import ctypes

import pytest
import torch

from quip_amd import _lib

ONE, NULL = ctypes.c_void_p(16), ctypes.c_void_p(0)     # non-null dummy pointers are never dereferenced: the checks come first


def _call(heads=32, kv_heads=8, hd=128, maxlen=512, q=ONE, dtype=1, ldq=None, ldk=None, ws_bytes=1 << 30, tables=(NULL, NULL)):
    ldq = heads * hd if ldq is None else ldq
    ldk = kv_heads * hd if ldk is None else ldk
    _lib.call("quipamd_decode_attention_grouped", q, ONE, ONE, ONE, ONE, ONE, ONE, tables[0], tables[1], 64, dtype, 2, heads, kv_heads, hd,
              maxlen, ctypes.c_float(0.1), ldq, ldk, ldk, ONE, ws_bytes, NULL)


def test_grouped_attention_refuses_bad_arguments_without_a_device():
    with pytest.raises(_lib.QuipAmdError, match="not a multiple of kv_heads") as e:
        _call(heads=12, kv_heads=8)
    assert "code 2" in str(e.value)                                   # QUIPAMD_ERR_SHAPE
    with pytest.raises(_lib.QuipAmdError, match="group size 32") as e:
        _call(heads=64, kv_heads=2)
    assert "code 4" in str(e.value)                                   # QUIPAMD_ERR_UNSUPPORTED
    with pytest.raises(_lib.QuipAmdError, match="group size 1"):
        _call(heads=8, kv_heads=8)                                    # multi-head: quipamd_decode_attention
    for hd in (16, 96, 256):
        with pytest.raises(_lib.QuipAmdError, match="head_dim"):
            _call(hd=hd)
    with pytest.raises(_lib.QuipAmdError, match="maxlen"):
        _call(maxlen=32769)
    with pytest.raises(_lib.QuipAmdError, match="f16 / bf16"):
        _call(dtype=0)
    with pytest.raises(_lib.QuipAmdError, match="null pointer") as e:
        _call(q=NULL)
    assert "code 1" in str(e.value)                                   # QUIPAMD_ERR_ARG
    with pytest.raises(_lib.QuipAmdError, match="16-byte aligned"):
        _call(q=ctypes.c_void_p(18))
    with pytest.raises(_lib.QuipAmdError, match="row strides"):
        _call(ldq=32 * 128 + 4)
    with pytest.raises(_lib.QuipAmdError, match="row strides"):
        _call(ldk=8 * 128 - 8)
    with pytest.raises(_lib.QuipAmdError, match="rotary tables"):
        _call(tables=(ONE, NULL))
    with pytest.raises(_lib.QuipAmdError, match="workspace"):
        _call(ws_bytes=64)


def test_workspace_size_follows_the_shape():
    f = _lib.load().quipamd_decode_attention_grouped_workspace_bytes
    assert f(1, 64, 8, 128, 256) == 0                                 # one chunk of positions: no partials, no counters
    small, big = f(1, 64, 8, 128, 4096), f(16, 64, 8, 128, 4096)
    assert small > 0 and big > 15 * small                             # counters + 16 chunks of (g x hd + 2 g) floats per (sequence, kv head)
    assert small >= 8 * 16 * (8 * 128 + 16) * 4
    assert f(1, 12, 8, 128, 4096) == 0                                # not a grouping: the launch itself refuses


def _tiny_llama(**kw):
    from transformers import LlamaConfig, LlamaForCausalLM
    cfg = dict(hidden_size=512, intermediate_size=256, num_hidden_layers=2, num_attention_heads=8, num_key_value_heads=2, vocab_size=96,
               max_position_embeddings=32, tie_word_embeddings=False)
    cfg.update(kw)
    return LlamaForCausalLM(LlamaConfig(**cfg))


def test_decoder_from_hf_binds_grouped_query_models():
    from quip_amd import decode
    m = _tiny_llama()                                                 # 8 heads of 64 over 2 key / value heads: g = 4
    d = decode.decoder_from_hf(m)
    assert d.arch == "llama" and d.heads == 8 and d.kv_heads == 2 and d.h == 512
    assert all(b.kv_heads == 2 and b.heads == 8 and b.hd == 64 for b in d.blocks)
    assert d.blocks[0].k_proj is m.model.layers[0].self_attn.k_proj and d.blocks[1].v_proj is m.model.layers[1].self_attn.v_proj
    assert d.blocks[0].k_proj.out_features == 2 * 64
    mha = decode.decoder_from_hf(_tiny_llama(num_key_value_heads=8))
    assert mha.kv_heads == mha.heads == 8 and all(b.kv_heads == b.heads for b in mha.blocks)


def test_decoder_from_hf_refuses_groupings_the_kernel_cannot_serve():
    from quip_amd import decode
    with pytest.raises(NotImplementedError, match="grouped-query"):
        decode.decoder_from_hf(_tiny_llama(hidden_size=2048, num_attention_heads=32, num_key_value_heads=1))     # g = 32
    with pytest.raises(NotImplementedError, match="grouped-query"):
        decode.decoder_from_hf(_tiny_llama(hidden_size=64, num_attention_heads=4, num_key_value_heads=2))         # head_dim 16
    with pytest.raises(NotImplementedError, match="grouped-query"):
        decode.decoder_from_hf(_tiny_llama(hidden_size=1536, num_attention_heads=16, num_key_value_heads=8))      # head_dim 96


def test_random_grouped_block_and_packed_paths_on_the_host():
    """LlamaBlock.random(kv_heads=...) sizes k / v; the v3 launch families stay multi-head only (fused_ok / fused_attention_ok refuse
    the grouped q / k / v, so a packed grouped-query model runs in mode `fused`)"""
    from quip_amd import decode, quant
    blk = decode.LlamaBlock.random(1024, 2048, 8, 1e-5, torch.float32, kv_heads=2)
    assert blk.kv_heads == 2 and blk.k_proj.out_features == blk.v_proj.out_features == 256 and blk.q_proj.out_features == 1024
    assert decode.LlamaBlock.random(1024, 2048, 8, 1e-5, torch.float32).kv_heads == 8
    qls = [quant.QuantLinear(1024, n, bits=2, qfn='b') for n in (1024, 256, 256)]
    assert not quant.fused_ok(qls, 1)
    kc = torch.empty((1, 2, 1, 128), dtype=torch.float16, device='meta')
    assert not quant.fused_attention_ok(qls, kc)
