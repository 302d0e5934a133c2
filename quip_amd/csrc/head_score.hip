// head_score.hip -- the lm_head GEMM with a log-probability epilogue (include/quip_amd_score.h)
//
// quipamd_head_score is two launches on one stream:
//
//   partial  grid (row tiles of 128, vocabulary slices of 256).  A workgroup of 4 waves computes z = x W^T for its 128 rows against its
//            slice, one tile of 128 vocabulary entries at a time, and reduces every finished tile -- still fp32 accumulators -- into five
//            numbers per row: the running maximum, the sum of exponentials under it, the best value with its index, and the target's logit
//            if the target lies in the slice.  They go to the workspace as [field][slice][row].
//   merge    one thread per row walks that row's slices in index order: lse, greedy and logprob.
//
// partial: the dense-weight sibling of the bs > 16 dequant-GEMM (both operands K-contiguous, staged global -> registers -> LDS, two LDS
// buffers, the loads of step i + 1 issued before the products of step i) in the orientation prefill_attn.hip uses for S^T = K Q^T:
//   A = 16 rows of W (vocabulary entries), B = 16 rows of x.  C: lane l holds entries 16 nb + 4 (l >> 4) + r of x row l & 15.
// Wave w owns x rows 32 w .. 32 w + 31 against all 128 entries of the tile (acc[8][2], 64 accumulator registers), so a row's statistics
// are in-lane over 32 values per tile; the four lanes that share a row (l, l ^ 16, l ^ 32, l ^ 48) keep their own online max / sum over
// the whole slice and are combined once, behind the last tile, with two shuffles.  a + b == b + a, so the four lanes end with the same bits.
// LDS rows are 64 elements (128 bytes); 16-byte chunk c of row r lies at chunk c ^ ((r >> 1) & 7): the sixteen rows of a ds_read_b128
// fragment fall on sixteen different 16-byte slots of the 256-byte bank row.
// Rows past `rows`, entries past `vocab` and k past h are staged as zeros (their loads go to a valid address and are masked on the way
// to LDS); entries past `vocab` are set to -inf before the statistics.  Nothing of a row mixes with another row: the outputs of a row are
// the same bits wherever it stands and whatever the call's `rows`.
// No atomics, no scratch; runs are bit-identical.
#include <math.h>

#include "common.h"
#include "quip_amd_score.h"

namespace {

constexpr int HS_BR = 128;                              // x rows per workgroup (32 per wave)
constexpr int HS_BV = 128;                              // vocabulary entries per tile
constexpr int HS_BK = 64;                               // k per staged step
constexpr int HS_SLICE_TILES = 2;
constexpr int HS_SLICE = HS_BV * HS_SLICE_TILES;        // vocabulary entries per slice: a constant, so the cut depends on vocab alone
constexpr int HS_FIELDS = 5;                            // max, sum, best value, target logit (fp32), best index (int32)
constexpr int HS_NLD = HS_BV * (HS_BK / 8) / 256;       // 16-byte chunks per thread, operand and step
constexpr int HS_TILE = HS_BV * HS_BK;                  // elements of one operand's LDS image

typedef _Float16 hs_f16x8 __attribute__((ext_vector_type(8)));

template <class TI> struct HsMma;
template <> struct HsMma<F16> {
    static __device__ __forceinline__ f32x4_t mma(uint4 a, uint4 b, f32x4_t c)
    {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(hs_f16x8, a), __builtin_bit_cast(hs_f16x8, b), c, 0, 0, 0);
    }
};
template <> struct HsMma<BF16> {
    static __device__ __forceinline__ f32x4_t mma(uint4 a, uint4 b, f32x4_t c)
    {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
    }
};

struct HsArgs {
    const uint16_t *x, *W;
    const int64_t *targets;
    int64_t ldx, ldw, rows, h, vocab;
    float *pm, *ps, *pbv, *pzt;           // partials [nslices][rows]
    int *pbi;
    float *logprob, *lse;
    int64_t *greedy;
    int nslices;
};

static inline int64_t hs_slices(int64_t vocab) { return (vocab + HS_SLICE - 1) / HS_SLICE; }

// element offset of 16-byte chunk `ch` of row `row` in an operand's LDS image
__device__ __forceinline__ int hs_off(int row, int ch) { return row * HS_BK + ((ch ^ ((row >> 1) & 7)) << 3); }

// exp(a - base) with exp(-inf - base) = 0; base is finite (a lane that has seen only -inf uses 0)
__device__ __forceinline__ float hs_exp(float a, float base) { return __expf(a - base); }

template <class TI>
__global__ __launch_bounds__(256, 2) void hs_partial_kernel(HsArgs A)
{
    __shared__ __attribute__((aligned(16))) uint16_t lds[2 * 2 * HS_TILE];      // [buffer][W, x][128][64]: 64 KB

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, hq = lane >> 4;
    const int64_t r0 = (int64_t)blockIdx.x * HS_BR;
    const int slice = blockIdx.y;
    const int64_t vs = (int64_t)slice * HS_SLICE;
    const int64_t left = A.vocab - vs;                                          // >= 1: the grid has no empty slice
    const int ntile = left >= HS_SLICE ? HS_SLICE_TILES : (int)((left + HS_BV - 1) / HS_BV);
    const int nk = (int)((A.h + HS_BK - 1) / HS_BK);
    const int total = ntile * nk;

    // this lane's two rows (column blocks cb = 0, 1 of the wave) and their targets
    int64_t tgt[2];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
        const int64_t row = r0 + 32 * wave + 16 * cb + li;
        tgt[cb] = row < A.rows ? A.targets[row] : -1;
    }
    float m[2], s[2], bv[2], zt[2];
    int bi[2];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
        m[cb] = -INFINITY; s[cb] = 0.f; bv[cb] = -INFINITY; zt[cb] = -INFINITY; bi[cb] = 0x7fffffff;
    }

    // staging: chunk i = tid + 256 u is row i >> 3, 16-byte chunk i & 7 of both operands.  Every load is issued, at an address clamped into
    // the operand (no branch, no select between a register and a load); what was clamped is zeroed by an AND on the way to LDS.
    uint4 wreg[HS_NLD], xreg[HS_NLD];
    uint32_t wmask = 0, xmask = 0;
    auto load_step = [&](int tile, int kt) {
        const int64_t v0 = vs + (int64_t)tile * HS_BV, k0 = (int64_t)kt * HS_BK;
        wmask = 0; xmask = 0;
#pragma unroll
        for (int u = 0; u < HS_NLD; ++u) {
            const int i = tid + 256 * u, row = i >> 3, ch = i & 7;
            const int64_t k = k0 + 8 * ch, vr = v0 + row, xr = r0 + row;
            const bool kok = k < A.h, wok = vr < A.vocab && kok, xok = xr < A.rows && kok;
            const int64_t kc = kok ? k : A.h - 8;
            wreg[u] = *reinterpret_cast<const uint4 *>(A.W + (vr < A.vocab ? vr : A.vocab - 1) * A.ldw + kc);
            xreg[u] = *reinterpret_cast<const uint4 *>(A.x + (xr < A.rows ? xr : A.rows - 1) * A.ldx + kc);
            wmask |= (uint32_t)wok << u;
            xmask |= (uint32_t)xok << u;
        }
    };
    auto masked = [](uint4 v, uint32_t bit) {
        const uint32_t k = 0u - (bit & 1u);
        return make_uint4(v.x & k, v.y & k, v.z & k, v.w & k);
    };

    load_step(0, 0);
    int it = 0;
    for (int tile = 0; tile < ntile; ++tile) {
        f32x4_t acc[8][2];
#pragma unroll
        for (int nb = 0; nb < 8; ++nb)
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) acc[nb][cb] = f32x4_t{0.f, 0.f, 0.f, 0.f};

        for (int kt = 0; kt < nk; ++kt, ++it) {
            uint16_t *Ws = lds + (it & 1) * (2 * HS_TILE), *Xs = Ws + HS_TILE;
            // the buffer was last read in step it - 2; every wave passed the barrier of step it - 1 after those reads
#pragma unroll
            for (int u = 0; u < HS_NLD; ++u) {
                const int i = tid + 256 * u, row = i >> 3, ch = i & 7;
                *reinterpret_cast<uint4 *>(Ws + hs_off(row, ch)) = masked(wreg[u], wmask >> u);
                *reinterpret_cast<uint4 *>(Xs + hs_off(row, ch)) = masked(xreg[u], xmask >> u);
            }
            __syncthreads();
            if (it + 1 < total) {
                if (kt + 1 < nk) load_step(tile, kt + 1);
                else load_step(tile + 1, 0);
            }
#pragma unroll
            for (int ks = 0; ks < HS_BK / 32; ++ks) {
                uint4 b[2];
#pragma unroll
                for (int cb = 0; cb < 2; ++cb) b[cb] = *reinterpret_cast<const uint4 *>(Xs + hs_off(32 * wave + 16 * cb + li, 4 * ks + hq));
#pragma unroll
                for (int nb = 0; nb < 8; ++nb) {
                    const uint4 a = *reinterpret_cast<const uint4 *>(Ws + hs_off(16 * nb + li, 4 * ks + hq));
#pragma unroll
                    for (int cb = 0; cb < 2; ++cb) acc[nb][cb] = HsMma<TI>::mma(a, b[cb], acc[nb][cb]);
                }
            }
        }

        // the tile is complete: acc[nb][cb][r] is entry v0 + 16 nb + 4 hq + r of row 32 wave + 16 cb + li
        const int64_t v0 = vs + (int64_t)tile * HS_BV;
        if (v0 + HS_BV > A.vocab) {                                             // uniform: the tile that holds the end of the vocabulary
#pragma unroll
            for (int nb = 0; nb < 8; ++nb)
#pragma unroll
                for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (v0 + 16 * nb + 4 * hq + r >= A.vocab) acc[nb][cb][r] = -INFINITY;
        }
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
            float mt = -INFINITY;
#pragma unroll
            for (int nb = 0; nb < 8; ++nb)
#pragma unroll
                for (int r = 0; r < 4; ++r) mt = fmaxf(mt, acc[nb][cb][r]);
            if (mt > bv[cb]) {                                                  // strictly: an earlier (smaller) index keeps a tie
                int idx = 0;
#pragma unroll
                for (int nb = 7; nb >= 0; --nb)
#pragma unroll
                    for (int r = 3; r >= 0; --r)
                        if (acc[nb][cb][r] == mt) idx = 16 * nb + r;            // walked downwards: the smallest index stays
                bv[cb] = mt;
                bi[cb] = (int)v0 + idx + 4 * hq;
            }
            const float mn = fmaxf(m[cb], mt);
            const float base = mn == -INFINITY ? 0.f : mn;
            float sum = 0.f;
#pragma unroll
            for (int nb = 0; nb < 8; ++nb)
#pragma unroll
                for (int r = 0; r < 4; ++r) sum += hs_exp(acc[nb][cb][r], base);
            s[cb] = s[cb] * hs_exp(m[cb], base) + sum;
            m[cb] = mn;
            const int64_t tl = tgt[cb] - v0;
            if (tl >= 0 && tl < HS_BV && (((int)tl >> 2) & 3) == hq) {
                const int want = (int)tl - 4 * hq;                              // 16 nb + r
#pragma unroll
                for (int nb = 0; nb < 8; ++nb)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (16 * nb + r == want) zt[cb] = acc[nb][cb][r];
            }
        }
    }

    // the four lanes of a row: two exchanges, each symmetric, so all four end with the same bits
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
#pragma unroll
        for (int off = 16; off <= 32; off <<= 1) {
            const float om = __shfl_xor(m[cb], off), os = __shfl_xor(s[cb], off), ov = __shfl_xor(bv[cb], off), oz = __shfl_xor(zt[cb], off);
            const int oi = __shfl_xor(bi[cb], off);
            const float mn = fmaxf(m[cb], om);
            const float base = mn == -INFINITY ? 0.f : mn;
            s[cb] = s[cb] * hs_exp(m[cb], base) + os * hs_exp(om, base);
            m[cb] = mn;
            if (ov > bv[cb] || (ov == bv[cb] && oi < bi[cb])) { bv[cb] = ov; bi[cb] = oi; }
            zt[cb] = fmaxf(zt[cb], oz);
        }
        const int64_t row = r0 + 32 * wave + 16 * cb + li;
        if (hq == 0 && row < A.rows) {
            const int64_t p = (int64_t)slice * A.rows + row;
            A.pm[p] = m[cb]; A.ps[p] = s[cb]; A.pbv[p] = bv[cb]; A.pzt[p] = zt[cb]; A.pbi[p] = bi[cb];
        }
    }
}

// ---- merge: one thread per row, slices in index order -----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hs_merge_kernel(HsArgs A)
{
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= A.rows) return;
    float M = -INFINITY;
    for (int sl = 0; sl < A.nslices; ++sl) M = fmaxf(M, A.pm[(int64_t)sl * A.rows + row]);
    const float base = M == -INFINITY ? 0.f : M;
    float S = 0.f, best = -INFINITY, z = -INFINITY;
    int idx = 0;
    for (int sl = 0; sl < A.nslices; ++sl) {
        const int64_t p = (int64_t)sl * A.rows + row;
        S += A.ps[p] * expf(A.pm[p] - base);
        const float v = A.pbv[p];
        if (sl == 0 || v > best) { best = v; idx = A.pbi[p]; }                  // strictly: the earlier slice keeps a tie
        z = fmaxf(z, A.pzt[p]);
    }
    const float lse = M + logf(S);
    const int64_t t = A.targets[row];
    A.lse[row] = lse;
    A.greedy[row] = idx;
    A.logprob[row] = t < 0 ? 0.f : t >= A.vocab ? -INFINITY : z - lse;
}

template <class TI> int hs_launch(const HsArgs &A, hipStream_t s)
{
    const dim3 grid((unsigned)((A.rows + HS_BR - 1) / HS_BR), (unsigned)A.nslices);
    hs_partial_kernel<TI><<<grid, 256, 0, s>>>(A);
    QA_LAUNCH_CHECK("head_score (partials)");
    hs_merge_kernel<<<(unsigned)((A.rows + 255) / 256), 256, 0, s>>>(A);
    QA_LAUNCH_CHECK("head_score (merge)");
    return QUIPAMD_OK;
}

}   // namespace

extern "C" int64_t quipamd_head_score_workspace_bytes(int64_t rows, int64_t vocab)
{
    if (rows < 1 || vocab < 1 || hs_slices(vocab) > 65535 || rows > ((int64_t)1 << 31) - HS_BR) return 0;
    return hs_slices(vocab) * rows * HS_FIELDS * 4;
}

extern "C" int quipamd_head_score(const void *x, int64_t ldx, const void *W, int64_t ldw, const int64_t *targets, int dtype, int64_t rows,
                                  int64_t h, int64_t vocab, float *logprob, float *lse, int64_t *greedy, void *workspace,
                                  int64_t workspace_bytes, void *stream)
{
    QA_REQUIRE(x && W && targets && logprob && lse && greedy && workspace, QUIPAMD_ERR_ARG, "head_score: null pointer");
    QA_REQUIRE(dtype == QUIPAMD_F16 || dtype == QUIPAMD_BF16, QUIPAMD_ERR_UNSUPPORTED, "head_score: f16 / bf16 only (dtype %d)", dtype);
    QA_REQUIRE(rows >= 1 && rows <= ((int64_t)1 << 31) - HS_BR, QUIPAMD_ERR_SHAPE, "head_score: rows %lld (at least one row)", (long long)rows);
    QA_REQUIRE(vocab >= 1 && hs_slices(vocab) <= 65535, QUIPAMD_ERR_SHAPE, "head_score: vocab %lld (1 .. %d)", (long long)vocab,
               65535 * HS_SLICE);
    QA_REQUIRE(h >= 32 && h % 32 == 0, QUIPAMD_ERR_SHAPE, "head_score: h %lld is not a multiple of 32", (long long)h);
    QA_REQUIRE(ldx >= h && ldw >= h && ldx % 8 == 0 && ldw % 8 == 0, QUIPAMD_ERR_SHAPE,
               "head_score: row strides %lld / %lld (multiples of 8, at least a row)", (long long)ldx, (long long)ldw);
    QA_REQUIRE((((uintptr_t)x | (uintptr_t)W | (uintptr_t)targets | (uintptr_t)logprob | (uintptr_t)lse | (uintptr_t)greedy |
                 (uintptr_t)workspace) & 15) == 0, QUIPAMD_ERR_ARG, "head_score: pointers must be 16-byte aligned");
    const int64_t need = quipamd_head_score_workspace_bytes(rows, vocab);
    QA_REQUIRE(workspace_bytes >= need, QUIPAMD_ERR_ARG, "head_score: workspace of %lld bytes is too small (%lld needed)",
               (long long)workspace_bytes, (long long)need);
    HsArgs A;
    A.x = (const uint16_t *)x; A.W = (const uint16_t *)W; A.targets = targets;
    A.ldx = ldx; A.ldw = ldw; A.rows = rows; A.h = h; A.vocab = vocab;
    A.nslices = (int)hs_slices(vocab);
    const int64_t n = (int64_t)A.nslices * rows;
    A.pm = (float *)workspace; A.ps = A.pm + n; A.pbv = A.ps + n; A.pzt = A.pbv + n; A.pbi = (int *)(A.pzt + n);
    A.logprob = logprob; A.lse = lse; A.greedy = greedy;
    hipStream_t s = (hipStream_t)stream;
    return dtype == QUIPAMD_F16 ? hs_launch<F16>(A, s) : hs_launch<BF16>(A, s);
}
