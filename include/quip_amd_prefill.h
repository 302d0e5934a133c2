/* quip_amd_prefill.h -- the prompt-side entries of libquip_amd.so (C ABI, same conventions as quip_amd.h)
 *
 * Why a header of its own: quip_amd.h and the Python table _lib.SIGNATURES are tied together by the test suite.  tests/test_abi.py
 * asserts that the table lists exactly the names quip_amd.h declares, and tests/test_gpu_memory_contract.py asserts that every
 * launching name of that table ran under a guard arena IN THAT FILE.  A new launching entry declared there would need a new case in
 * an existing test file.  The entries of this header are bound through a second table, _lib.PREFILL_SIGNATURES, and meet the same
 * two obligations in tests of their own: tests/test_prefill_host.py (header == table == exported symbols, disjoint from SIGNATURES)
 * and tests/test_gpu_prefill_contract.py (every launching name of the table ran under a guard arena).
 *
 * Return codes, dtype codes and quipamd_last_error() are those of quip_amd.h.
 */
#ifndef QUIP_AMD_PREFILL_H
#define QUIP_AMD_PREFILL_H

#include <stdint.h>

#include "quip_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Causal attention over T >= 1 new positions per sequence with a static KV cache (csrc/prefill_attn.hip).
 *
 *   q   [bs*T, heads*hd]     row b*T + t is new position t of sequence b; row stride ldq (elements, a multiple of 8)
 *   k,v [bs*T, kv_heads*hd]  row strides ldk, ldv
 *   kcache, vcache [bs, kv_heads, maxlen, hd] contiguous
 *   start  int64 ON THE DEVICE: the cache position of new position 0 (read by the kernels: the call can be captured in a hipGraph)
 *   out [bs*T, heads*hd] contiguous
 *   cos_table, sin_table  fp32 [table_rows, hd], HF's duplicated-halves layout, or both NULL (no rotary)
 *
 * With g = heads / kv_heads (1..16, HF's repeat_kv order: query head j reads key / value head j / g):
 *   kcache / vcache[b, h, *start + t, :] = k / v[b*T + t, h*hd : (h+1)*hd]     (k rotated first when tables are given, bit-identical
 *                                                                               to quipamd_rope_inplace at position *start + t)
 *   out[b*T + t, j*hd : (j+1)*hd] = softmax(scale * q_j(t) . K_h[0 .. *start+t]^T) V_h[0 .. *start+t]    (q rotated the same way)
 * q, k, v are not written.  Two launches on `stream`: the append, then the attention, which reads K / V from the cache only.
 * K tiles are aligned to absolute cache positions, so a row's result depends on its absolute position alone: cutting a prompt into
 * calls in any way gives bit-identical out and caches.  No atomics, no workspace.
 * If *start < 0 or *start + T > maxlen nothing is written (and the call still returns QUIPAMD_OK: the host cannot see *start).
 * dtype QUIPAMD_F16 / QUIPAMD_BF16; hd 64 or 128; maxlen <= 32768; all pointers 16-byte aligned.
 */
int quipamd_prefill_attention(const void *q, const void *k, const void *v, void *kcache, void *vcache, const int64_t *start, int64_t T,
                              void *out, const float *cos_table, const float *sin_table, int64_t table_rows, int dtype, int64_t bs,
                              int heads, int kv_heads, int hd, int64_t maxlen, float scale, int64_t ldq, int64_t ldk, int64_t ldv,
                              void *stream);

#ifdef __cplusplus
}
#endif
#endif
