/* quip_amd_score.h -- the scoring entries of libquip_amd.so (C ABI, same conventions as quip_amd.h)
 *
 * A header of its own for the reason quip_amd_prefill.h gives: quip_amd.h and _lib.SIGNATURES are tied to existing test files.  These
 * entries are bound through _lib.SCORE_SIGNATURES and meet the two obligations in tests of their own: tests/test_score_host.py (header
 * == table == exported symbols, disjoint from the other tables) and tests/test_gpu_score_contract.py (every launching name of the table
 * ran under a guard arena).
 *
 * Return codes, dtype codes and quipamd_last_error() are those of quip_amd.h.
 */
#ifndef QUIP_AMD_SCORE_H
#define QUIP_AMD_SCORE_H

#include <stdint.h>

#include "quip_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The lm_head GEMM with a log-probability epilogue (csrc/head_score.hip): the [rows, vocab] logits are never written.
 *
 *   x        [rows, h]       f16 / bf16, row stride ldx (elements)
 *   W        [>= vocab, h]   same type, row stride ldw; only rows 0 .. vocab - 1 are read
 *   targets  int64 [rows]    ON THE DEVICE
 *   logprob, lse fp32 [rows]; greedy int64 [rows]
 *
 * With z[r][j] = sum_i x[r, i] W[j, i], accumulated in fp32 and never rounded to 16 bits, j < vocab:
 *   lse[r]     = log sum_j exp(z[r][j])                    (max-subtracted)
 *   greedy[r]  = the smallest j that attains max_j z[r][j]  (quipamd_argmax_rows' convention)
 *   logprob[r] = z[r][t] - lse[r]   for t = targets[r] in [0, vocab)
 *              = 0                  for t < 0 (an ignored position)
 *              = -inf               for t >= vocab
 * lse and greedy are written for every row.
 *
 * h % 32 == 0; rows >= 1 and vocab >= 1, any value (vocab <= 65535 * 256); ldx, ldw multiples of 8 and at least h; every pointer 16-byte
 * aligned; workspace_bytes >= quipamd_head_score_workspace_bytes(rows, vocab) (0 for rows or vocab it does not serve).  Anything else is
 * refused before a launch.
 *
 * Two launches on `stream`: per-slice partials, then a merge.  The vocabulary is cut into slices of 256 entries -- a rule of vocab
 * alone --, a workgroup walks its slice with an online max / sum, and the merge adds the slices in index order: no atomics, runs are
 * bit-identical, and a row's three outputs depend on that row of x, on W and on its target only -- not on `rows`, the row's index or the
 * other rows.  The call writes inside logprob / lse / greedy [rows] and workspace[workspace_bytes] only; x, W and targets are read-only.
 * The workspace needs no initialisation and carries nothing between calls.
 */
int64_t quipamd_head_score_workspace_bytes(int64_t rows, int64_t vocab);
int quipamd_head_score(const void *x, int64_t ldx, const void *W, int64_t ldw, const int64_t *targets, int dtype, int64_t rows, int64_t h,
                       int64_t vocab, float *logprob, float *lse, int64_t *greedy, void *workspace, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
