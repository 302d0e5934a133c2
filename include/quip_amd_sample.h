/* quip_amd_sample.h -- the token-sampling entry of libquip_amd.so (C ABI, same conventions as quip_amd.h)
 *
 * A header of its own for the reason quip_amd_prefill.h gives: quip_amd.h and _lib.SIGNATURES are tied together by tests/test_abi.py and
 * tests/test_gpu_memory_contract.py.  The entry of this header is bound through a third table, _lib.SAMPLE_SIGNATURES, and meets the same
 * two obligations in tests of its own: tests/test_sample_host.py (header == table == exported symbols, disjoint from the other two tables)
 * and tests/test_gpu_sample_contract.py (every launching name of the table ran under a guard arena).
 *
 * Return codes, dtype codes and quipamd_last_error() are those of quip_amd.h.
 */
#ifndef QUIP_AMD_SAMPLE_H
#define QUIP_AMD_SAMPLE_H

#include <stdint.h>

#include "quip_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* lives ON THE DEVICE and is read by the kernel at run time: a captured graph follows changes of it */
typedef struct quipamd_sample_params {
    float    temperature;   /* <= 0: greedy -- first index among the maxima, nothing is drawn */
    float    top_p;         /* >= 1: off */
    int32_t  top_k;         /* <= 0 or >= n: off */
    int32_t  reserved;
    uint64_t seed;
} quipamd_sample_params;

/* One token per row of `logits` by temperature / top-k / top-p sampling, one launch, one workgroup per row (csrc/decode_sample.hip).
 *
 *   logits  [rows, n] f32 / f16 / bf16, row stride ld >= n in elements; no alignment is asked of the rows.  1 <= n <= 262144,
 *           0 <= rows <= 65535 (rows == 0 launches nothing).
 *   params, counter   ON THE DEVICE (counter: one int64), read by the kernel
 *   out     int64 [rows];  logprob fp32 [rows], kept_n int32 [rows], kept_mass fp32 [rows]: each may be NULL
 *   clear   NULL, or int32 [rows, clear_n]: every word is set to -1 (the argmax partials of quipamd_decode_head: the next
 *           quipamd_decode_embed then reads `out` instead of them)
 *
 * Per row, with z_i = float(logits[i]) / temperature (entries that are -inf have probability 0 and are not candidates):
 *   order    z descending, ties by smaller index
 *   top-k    the first top_k entries of the order survive
 *   top-p    with p the softmax over the top-k survivors, entry i survives iff the summed p of the entries before it in the order is
 *            < top_p (Hugging Face's TopPLogitsWarper after TopKLogitsWarper); at least one entry survives
 *   kept_n   the number of survivors;  kept_mass  their summed p (1 when top-p is off)
 *   draw     u = (x0 >> 8) * 2^-24 with x0 the first word of Philox4x32-10, key (lo32(seed), hi32(seed)), counter words
 *            (lo32(*counter), hi32(*counter), row, 0).  With C_i the inclusive prefix sums of the survivors' weights exp(z_i - max z)
 *            in INDEX order and Z their total, the token is the first survivor with C_i > u * Z;  logprob = log(weight / Z)
 *   greedy   temperature <= 0 or top_k == 1: exactly quipamd_argmax_rows' answer, logprob 0, kept_n 1, kept_mass 1
 * The weights are fp32; every sum of them is carried in 2^-40 fixed point (integers), so no sum depends on the order in which it was
 * formed: the same inputs give the same outputs bit for bit.  A row holding NaN or +inf, or -inf only, still yields 0 <= out < n.
 */
int quipamd_sample_rows(const void *logits, int dtype, int64_t rows, int64_t n, int64_t ld,
                        const quipamd_sample_params *params, const int64_t *counter,
                        int64_t *out, float *logprob, int32_t *kept_n, float *kept_mass,
                        int32_t *clear, int64_t clear_n, void *stream);

#ifdef __cplusplus
}
#endif
#endif
