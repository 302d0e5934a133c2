/* quip_amd_groupwise.h -- the group-wise dequant-GEMM entry of libquip_amd.so (C ABI, same conventions as quip_amd.h)
 *
 * A header of its own for the reason quip_amd_score.h gives: quip_amd.h and _lib.SIGNATURES are tied to existing test files.  This entry
 * is bound through _lib.GROUPWISE_SIGNATURES and meets the two obligations in tests of its own: tests/test_groupwise_host.py (header ==
 * table == exported symbols, disjoint from the other tables) and tests/test_gpu_groupwise_contract.py (every launching name of the table
 * ran under a guard arena).
 *
 * Return codes, dtype codes and quipamd_last_error() are those of quip_amd.h.
 */
#ifndef QUIP_AMD_GROUPWISE_H
#define QUIP_AMD_GROUPWISE_H

#include <stdint.h>

#include "quip_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The fused dequant-GEMM with one (scale, zero) per output row and per group of G = groupsize consecutive input columns
 * (csrc/dqgemm_gw.hip) -- the grid a quantiser run with --groupsize leaves behind:
 *
 *   y[b, r] = bias[r] + sum_g gscale[g, r] * sum_{k in [g G, (g + 1) G)} (code[r, k] - gzero[g, r]) * x[b, k]
 *
 *   x        [bs, d]      f16 / bf16, row-major, dense
 *   qweight  the STREAM layout of quip_amd.h, unchanged: 16-row x (512 / bits)-column tiles, m * d * cb / 32 words, cb = 2 for bits 2 and
 *            4 for bits 3 and 4 (3-bit codes sit in the 4-bit container)
 *   gscale, gzero   float [d / G, m], GROUP-MAJOR: the parameters of group g for all rows are contiguous (the four consecutive output rows
 *            a lane owns are one 16-byte load).  gzero need not be an integer.
 *   bias     float [m] or NULL
 *   y        [bs, m] in y_dtype: F32, F16 or BF16, whatever x is
 *
 * bits 2 / 3 / 4; groupsize 32 / 64 / 128 (a group is groupsize / 32 whole MFMA steps and a STREAM tile holds whole groups at every
 * width); m % 16 == 0; d % (512 / bits') == 0 with bits' = cb; bs >= 1, any value; every pointer 16-byte aligned.  Anything else is
 * refused before a launch.
 *
 * The products code * x and the group sums are accumulated in fp32 on the matrix pipe from the exact values OFF + code (OFF = 4 or 16);
 * each group is folded in fp32 as gscale * (acc - (OFF + gzero) * sum_{k in g} x[b, k]).  Within 1e-3 (relative l2, fp32 y) of the formula
 * evaluated in fp64 on the 16-bit x.
 *
 * One launch on `stream`.  Two regimes chosen from bs alone: bs <= 16 (one batch tile, K split over the waves of a workgroup, partials
 * met once in LDS and added in index order) and bs > 16 (64 batch rows per workgroup, gridDim.y over batch blocks).  No atomics: runs are
 * bit-identical.  A row of y depends on that row of x and on the weights only -- not on the other rows or on its index, and within a
 * regime not on bs.  The call reads inside x [bs, d], the code words, the two tables [d / G, m] and bias [m] only and writes inside
 * y [bs, m] only; it needs no workspace.
 */
int quipamd_dequant_gemm_groupwise(const void *x, int x_dtype, const int32_t *qweight, int bits, int groupsize, const float *gscale,
                                   const float *gzero, const float *bias, void *y, int y_dtype, int64_t bs, int64_t m, int64_t d,
                                   void *stream);

#ifdef __cplusplus
}
#endif
#endif
