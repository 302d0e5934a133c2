/* quip_amd_generate.h -- the generation-control entry of libquip_amd.so (C ABI, same conventions as quip_amd.h)
 *
 * A header of its own for the reason quip_amd_sample.h gives: the earlier header / table pairs are tied together by their tests
 * (tests/test_sample_host.py holds _lib.SAMPLE_SIGNATURES to the names of quip_amd_sample.h, tests/test_gpu_sample_contract.py asks every name
 * of that table for a run under its arena).  The entry of this header is bound through a fourth table, _lib.GENERATE_SIGNATURES, and meets
 * the same two obligations in tests of its own: tests/test_generate_host.py (header == table == exported symbols, disjoint from the other
 * three tables) and tests/test_gpu_generate_contract.py (every launching name of the table ran under a guard arena).
 *
 * Return codes, dtype codes and quipamd_last_error() are those of quip_amd.h.
 */
#ifndef QUIP_AMD_GENERATE_H
#define QUIP_AMD_GENERATE_H

#include <stdint.h>

#include "quip_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QUIPAMD_GENERATE_MAX_STOP 16

/* one per row, ON THE DEVICE, read by the kernel at run time: a captured graph follows changes of it */
typedef struct quipamd_generate_params {
    float    temperature;          /* <= 0: greedy -- first index among the maxima, nothing is drawn */
    float    top_p;                /* >= 1: off */
    int32_t  top_k;                /* <= 0 or >= n: off */
    float    repetition_penalty;   /* > 0; 1: off */
    uint64_t seed;
} quipamd_generate_params;

/* quipamd_sample_rows with per-row parameters, a repetition penalty over the row's token history, and stop tokens: one launch, one
 * workgroup per row (csrc/decode_generate.hip; the sampling arithmetic is the one copy in csrc/sample_body.h).
 *
 *   logits, dtype, rows, n, ld, counter, out, logprob, kept_n, kept_mass, clear, clear_n     as in quipamd_sample_rows
 *   params    quipamd_generate_params[rows] ON THE DEVICE: row r uses params[r]; its draw is Philox4x32-10 with key params[r].seed and
 *             counter words (lo32(*counter), hi32(*counter), r, 0)
 *   hist      NULL, or int32 [rows, ld_hist] with hist_cap >= 1 usable columns (ld_hist >= hist_cap): the tokens of row r by position.
 *             With c = *counter the kernel stores hist[r, c] = out[r] at its end, and before anything else hist[r, c - 1] = fed[r] when
 *   fed       (int64 [rows], may be NULL, may be `out`: it is read before `out` is written) is given.  A position < 0 or >= hist_cap is
 *             neither written nor read.
 *   penalty   with p = params[r].repetition_penalty != 1: for every DISTINCT id in hist[r, 0 : min(c, hist_cap)] (after the store of
 *             fed) that lies in [0, n), the logit x = float(logits[r, id]) counts as x < 0 ? x * p : x / p (fp32, an IEEE division) in
 *             every step of the contract of quipamd_sample_rows, the greedy one included.  `logits` is not written.
 *   stop_ids  NULL, or int32 [n_stop] ON THE DEVICE, 0 <= n_stop <= 16;  pad_id  what a finished row yields (0 <= pad_id < 2^31)
 *   done      NULL, or int32 [rows], in / out;  stop_pos  NULL, or int64 [rows], in / out
 *             A row with done[r] != 0 on entry reads no logits: out = pad_id, logprob = 0, kept_n = 0, kept_mass = 1, hist[r, c] = pad_id.
 *             Any other row whose token is one of stop_ids gets done[r] = 1 and stop_pos[r] = c.
 * With hist, stop_ids and done NULL and equal parameters in every row, the outputs are those of quipamd_sample_rows bit for bit.
 */
int quipamd_generate_rows(const void *logits, int dtype, int64_t rows, int64_t n, int64_t ld,
                          const quipamd_generate_params *params, const int64_t *counter,
                          int32_t *hist, int64_t hist_cap, int64_t ld_hist, const int64_t *fed,
                          const int32_t *stop_ids, int64_t n_stop, int64_t pad_id, int32_t *done, int64_t *stop_pos,
                          int64_t *out, float *logprob, int32_t *kept_n, float *kept_mass,
                          int32_t *clear, int64_t clear_n, void *stream);

#ifdef __cplusplus
}
#endif
#endif
