// prefill_attn.hip -- causal attention over T >= 1 new positions per sequence (the prompt pass of the decode engine)
//
// quipamd_prefill_attention (include/quip_amd_prefill.h) is two launches on one stream:
//
//   append  kcache / vcache[b, h, *start + t, :] = k / v[b T + t, h hd ..]; k rotated with rope_kernel's fp32 expression (bit-identical
//           to quipamd_rope_inplace at position *start + t followed by a copy).  One thread per (row, kv head, element pair).
//   attend  out[b T + t, j] = softmax(scale q_j(t) . K_h[0 .. *start + t]^T) V_h[0 .. *start + t], h = j / g, reading K / V from the
//           cache only (the rows of this call were appended by the launch before it).
//
// attend: a workgroup of 4 waves serves 64 new positions of one (sequence, query head); wave w owns 16 of them.  It walks the cache in
// tiles of 64 positions ALIGNED TO ABSOLUTE POSITIONS ([64 c, 64 c + 64)), so the reduction order of a query row depends on its absolute
// position only -- not on *start, T or its place in the query tile: a prompt cut into calls in any way gives the same bits.  Tiles
// wholly above the workgroup's (the wave's) last row are not visited; inside a visited tile a position past the row is a select to
// -inf before the max, which leaves max, sum and accumulator of that row exactly as they were (exp(-inf) = 0, x * 1 = x, x + 0 = x).
//
// Both products run on v_mfma_f32_16x16x32_{f16,bf16} in the swapped orientation, so that no lane movement lies between them:
//   S^T = K Q^T   A = K rows of the tile (ds_read_b128 from the row-major LDS image), B = the wave's q rows (registers, loaded and
//                 rotated once).  C: lane l holds key 16 nb + 4 (l >> 4) + r of query row l & 15 -- a query row's statistics are
//                 in-lane plus two shuffles (xor 16, 32), and max / sum / rescale factor are ONE scalar per lane.
//   O^T = V^T P^T B = P, the S^T accumulator rounded to the 16-bit type, registers r of tiles nb = 2 ks, 2 ks + 1 as the 8 elements of
//                 k-step ks: element j of lane group h is key 32 ks + 16 (j >> 2) + 4 h + (j & 3).  A = V^T in the SAME key order:
//                 two ds_read_b64_tr_b16 (rows 32 ks + 4 h .., + 16) of the row-major V image, the hardware transposes.
// Scores, max, sum and O are fp32; P is rounded only as the MFMA operand; the sum adds the unrounded fp32 P.
// K / V tiles go global -> registers -> LDS; the loads of tile c + 1 are issued before the products of tile c.
// LDS rows are padded by 16 elements (stride = 8 dwords mod 64): the transposed reads are conflict-free, the row reads 2-way.
// No atomics, no workspace, no scratch; runs are bit-identical.
#include "common.h"
#include "quip_amd_prefill.h"

namespace {

constexpr int PF_BM = 64;                                // new positions per workgroup (16 per wave)
constexpr int PF_BN = 64;                                // cached positions per tile
constexpr int PF_PAD = 16;                               // elements of padding per LDS row

typedef _Float16 pf_f16x8 __attribute__((ext_vector_type(8)));
typedef short pf_s16x4 __attribute__((ext_vector_type(4)));

template <class TI> struct PfMma;
template <> struct PfMma<F16> {
    static __device__ __forceinline__ f32x4_t mma(uint4 a, uint4 b, f32x4_t c)
    {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(pf_f16x8, a), __builtin_bit_cast(pf_f16x8, b), c, 0, 0, 0);
    }
    static __device__ __forceinline__ uint32_t bits(float f) { return f32_to_f16_bits(f); }
};
template <> struct PfMma<BF16> {
    static __device__ __forceinline__ f32x4_t mma(uint4 a, uint4 b, f32x4_t c)
    {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
    }
    static __device__ __forceinline__ uint32_t bits(float f) { return f32_to_bf16_bits(f); }
};

// ds_read_b64_tr_b16: per group of 16 lanes a block of 4 rows x 16 columns; lane 4 q + p gives the address of row q, columns 4 p ..
// 4 p + 3, lane i receives column i of the four rows.  EXEC must be full: every call site is wave-uniform.
__device__ __forceinline__ uint2 pf_tr_read(const uint16_t *p)
{
    typedef __attribute__((address_space(3))) pf_s16x4 lds_s16x4;
    return __builtin_bit_cast(uint2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)p));
}

struct PfArgs {
    const uint16_t *q, *k, *v;            // [bs T, heads hd] (ldq), [bs T, kv hd] (ldk, ldv)
    uint16_t *kc, *vc, *out;              // [bs, kv, maxlen, hd]; out [bs T, heads hd] contiguous
    const int64_t *start;
    const float *cos_t, *sin_t;           // rotary tables [table_rows, hd] or null
    int64_t table_rows, maxlen, ldq, ldk, ldv, T;
    int heads, kv, g;
    float scale;
};

// ---- append: one thread per (row b T + t, kv head, i < hd / 2) -------------------------------------------------------------------------
template <class TI>
__global__ __launch_bounds__(256) void pf_append_kernel(PfArgs A, int hd, int64_t total)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int64_t start = *A.start;
    if (start < 0 || start + A.T > A.maxlen) return;                      // uniform: nothing is written
    const int half = hd / 2, i = (int)(idx % half);
    const int64_t rh = idx / half;
    const int h = (int)(rh % A.kv);
    const int64_t row = rh / A.kv;                                        // b T + t
    const int64_t b = row / A.T, t = row % A.T, pos = start + t;
    const uint16_t *kn = A.k + row * A.ldk + (int64_t)h * hd, *vn = A.v + row * A.ldv + (int64_t)h * hd;
    const int64_t crow = ((b * A.kv + h) * A.maxlen + pos) * hd;
    uint16_t *kd = A.kc + crow, *vd = A.vc + crow;
    if (A.cos_t != nullptr && pos < A.table_rows) {                       // past the tables: no rotation (like quipamd_rope_inplace)
        const float c = A.cos_t[pos * hd + i], s = A.sin_t[pos * hd + i];
        const float a = DT<TI>::load(kn, i), bb = DT<TI>::load(kn, i + half);
        DT<TI>::store(kd, i, a * c - bb * s);
        DT<TI>::store(kd, i + half, bb * c + a * s);
    } else {
        kd[i] = kn[i];
        kd[i + half] = kn[i + half];
    }
    vd[i] = vn[i];
    vd[i + half] = vn[i + half];
}

// ---- attend ------------------------------------------------------------------------------------------------------------------------------
template <class TI, int HD>
__global__ __launch_bounds__(256) void pf_attn_kernel(PfArgs A)
{
    constexpr int LDW = HD + PF_PAD;                    // LDS row stride in elements
    constexpr int KS = HD / 32;                         // k-steps of S^T = K Q^T
    constexpr int DB = HD / 16;                         // 16-row blocks of O^T
    constexpr int CPR = HD / 8;                         // 16-byte chunks per cache row
    constexpr int NLD = PF_BN * CPR / 256;              // chunks per thread and tile, for K and for V
    __shared__ __attribute__((aligned(16))) uint16_t lds[2 * PF_BN * LDW];
    uint16_t *Ks = lds, *Vs = lds + PF_BN * LDW;

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, hq = lane >> 4;
    const int64_t start = *A.start, T = A.T;
    if (start < 0 || start + T > A.maxlen) return;                        // uniform: nothing is written
    const int64_t nqt = (T + PF_BM - 1) / PF_BM;
    const int64_t qt = nqt - 1 - (int64_t)blockIdx.x;                     // the longest rows first
    const int j = blockIdx.y, kvh = j / A.g;
    const int64_t b = blockIdx.z;
    const int64_t last = start + T - 1;                                   // the last cached position this call may read
    const int64_t t_wg_last = (qt * PF_BM + PF_BM - 1 < T - 1) ? qt * PF_BM + PF_BM - 1 : T - 1;
    const int nt = (int)((start + t_wg_last) / PF_BN) + 1;                // tiles 0 .. nt - 1 hold positions 0 .. the workgroup's last row
    const int64_t t_w0 = qt * PF_BM + 16 * wave;
    const bool wave_on = t_w0 < T;                                        // uniform per wave
    const int64_t t_w_last = (t_w0 + 15 < T - 1) ? t_w0 + 15 : T - 1;
    const int64_t p_w_last = start + t_w_last;
    const int64_t t = t_w0 + li;                                          // this lane's query row
    const int64_t prow = start + t;

    const uint16_t *kcb = A.kc + (b * A.kv + kvh) * A.maxlen * HD, *vcb = A.vc + (b * A.kv + kvh) * A.maxlen * HD;

    // q rows of the wave: lane (row li, group hq) holds elements 32 ks + 8 hq .. + 7, rotated with rope_kernel's fp32 expression
    uint4 qf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = make_uint4(0, 0, 0, 0);
    if (t < T) {
        const uint16_t *qr = A.q + (b * T + t) * A.ldq + (int64_t)j * HD;
        const bool rot = A.cos_t != nullptr && prow < A.table_rows;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int e0 = 32 * ks + 8 * hq;
            uint4 x = *reinterpret_cast<const uint4 *>(qr + e0);
            if (rot) {
                const bool lo = e0 < HD / 2;
                const int i0 = lo ? e0 : e0 - HD / 2;                     // the pair index: tables are read at i < hd / 2, like rope_kernel
                const uint4 y = *reinterpret_cast<const uint4 *>(qr + (lo ? e0 + HD / 2 : e0 - HD / 2));
                const uint16_t *xs = reinterpret_cast<const uint16_t *>(&x), *ys = reinterpret_cast<const uint16_t *>(&y);
                uint32_t o[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float c = A.cos_t[prow * HD + i0 + e], s = A.sin_t[prow * HD + i0 + e];
                    const float xe = DT<TI>::load(xs, e), ye = DT<TI>::load(ys, e);
                    // low half: a c - bb s with a = x, bb = y; high half: bb c + a s with bb = x, a = y
                    o[e] = PfMma<TI>::bits(lo ? xe * c - ye * s : xe * c + ye * s);
                }
                x = make_uint4(o[0] | o[1] << 16, o[2] | o[3] << 16, o[4] | o[5] << 16, o[6] | o[7] << 16);
            }
            qf[ks] = x;
        }
    }

    f32x4_t acc[DB];
#pragma unroll
    for (int db = 0; db < DB; ++db) acc[db] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;

    uint4 kreg[NLD], vreg[NLD];
    auto load_tile = [&](int c) {
#pragma unroll
        for (int u = 0; u < NLD; ++u) {
            const int i = tid + 256 * u, row = i / CPR, ch = i % CPR;
            const int64_t p = (int64_t)c * PF_BN + row;
            if (p <= last) {                                              // rows past this call's last position may hold anything: zeros
                kreg[u] = *reinterpret_cast<const uint4 *>(kcb + p * HD + 8 * ch);
                vreg[u] = *reinterpret_cast<const uint4 *>(vcb + p * HD + 8 * ch);
            } else {
                kreg[u] = make_uint4(0, 0, 0, 0);
                vreg[u] = make_uint4(0, 0, 0, 0);
            }
        }
    };

    load_tile(0);
    for (int c = 0; c < nt; ++c) {
        __syncthreads();                                                  // the reads of tile c - 1 are done
#pragma unroll
        for (int u = 0; u < NLD; ++u) {
            const int i = tid + 256 * u, row = i / CPR, ch = i % CPR;
            *reinterpret_cast<uint4 *>(Ks + row * LDW + 8 * ch) = kreg[u];
            *reinterpret_cast<uint4 *>(Vs + row * LDW + 8 * ch) = vreg[u];
        }
        __syncthreads();
        if (c + 1 < nt) load_tile(c + 1);
        if (!wave_on || (int64_t)c * PF_BN > p_w_last) continue;         // uniform per wave: the tile lies above all its rows

        // S^T = K Q^T: s[nb][r] is key 64 c + 16 nb + 4 hq + r against query row li
        f32x4_t s[4];
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            s[nb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const uint4 a = *reinterpret_cast<const uint4 *>(Ks + (16 * nb + li) * LDW + 32 * ks + 8 * hq);
                s[nb] = PfMma<TI>::mma(a, qf[ks], s[nb]);
            }
        }
        float mt = -INFINITY;
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t kp = (int64_t)c * PF_BN + 16 * nb + 4 * hq + r;
                const float x = kp <= prow ? s[nb][r] * A.scale : -INFINITY;
                s[nb][r] = x;
                mt = fmaxf(mt, x);
            }
        mt = fmaxf(mt, __shfl_xor(mt, 16));
        mt = fmaxf(mt, __shfl_xor(mt, 32));
        const float mn = fmaxf(m, mt);                                    // finite: tile 0 holds position 0 <= every row
        const float alpha = __expf(m - mn);
        float lt = 0.f;
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = __expf(s[nb][r] - mn);
                s[nb][r] = p;
                lt += p;
            }
        lt += __shfl_xor(lt, 16);
        lt += __shfl_xor(lt, 32);
        l = l * alpha + lt;
        m = mn;
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[db][r] *= alpha;

        // O^T += V^T P^T: k-step ks takes S^T tiles nb = 2 ks, 2 ks + 1; element j of lane group hq is key 32 ks + 16 (j >> 2) + 4 hq + (j & 3)
        uint4 pb[2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            uint32_t o[8];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                o[r] = PfMma<TI>::bits(s[2 * ks][r]);
                o[4 + r] = PfMma<TI>::bits(s[2 * ks + 1][r]);
            }
            pb[ks] = make_uint4(o[0] | o[1] << 16, o[2] | o[3] << 16, o[4] | o[5] << 16, o[6] | o[7] << 16);
        }
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const uint16_t *vp = Vs + (32 * ks + 4 * hq + (li >> 2)) * LDW + 16 * db + 4 * (li & 3);
                const uint2 a0 = pf_tr_read(vp), a1 = pf_tr_read(vp + 16 * LDW);
                acc[db] = PfMma<TI>::mma(make_uint4(a0.x, a0.y, a1.x, a1.y), pb[ks], acc[db]);
            }
    }

    // O^T: lane holds elements 16 db + 4 hq + r of query row li
    if (t < T) {
        uint16_t *orow = A.out + ((b * T + t) * A.heads + j) * HD;
#pragma unroll
        for (int db = 0; db < DB; ++db) {
            uint32_t o[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] = PfMma<TI>::bits(acc[db][r] / l);
            *reinterpret_cast<uint2 *>(orow + 16 * db + 4 * hq) = make_uint2(o[0] | o[1] << 16, o[2] | o[3] << 16);
        }
    }
}

template <class TI> int pf_launch(const PfArgs &A, int64_t bs, int hd, hipStream_t s)
{
    const int64_t total = bs * A.T * A.kv * (hd / 2);
    pf_append_kernel<TI><<<(unsigned)((total + 255) / 256), 256, 0, s>>>(A, hd, total);
    QA_LAUNCH_CHECK("prefill_attention (append)");
    const dim3 grid((unsigned)((A.T + PF_BM - 1) / PF_BM), (unsigned)A.heads, (unsigned)bs);
    if (hd == 64) pf_attn_kernel<TI, 64><<<grid, 256, 0, s>>>(A);
    else pf_attn_kernel<TI, 128><<<grid, 256, 0, s>>>(A);
    QA_LAUNCH_CHECK("prefill_attention");
    return QUIPAMD_OK;
}

}   // namespace

extern "C" int quipamd_prefill_attention(const void *q, const void *k, const void *v, void *kcache, void *vcache, const int64_t *start,
                                         int64_t T, void *out, const float *cos_table, const float *sin_table, int64_t table_rows,
                                         int dtype, int64_t bs, int heads, int kv_heads, int hd, int64_t maxlen, float scale, int64_t ldq,
                                         int64_t ldk, int64_t ldv, void *stream)
{
    QA_REQUIRE(bs >= 0 && heads > 0 && kv_heads > 0 && maxlen > 0, QUIPAMD_ERR_SHAPE, "prefill_attention: bad shape");
    QA_REQUIRE(T >= 1, QUIPAMD_ERR_SHAPE, "prefill_attention: T %lld (at least one new position)", (long long)T);
    QA_REQUIRE(heads % kv_heads == 0, QUIPAMD_ERR_SHAPE, "prefill_attention: heads %d is not a multiple of kv_heads %d", heads, kv_heads);
    const int g = heads / kv_heads;
    QA_REQUIRE(g <= 16, QUIPAMD_ERR_UNSUPPORTED, "prefill_attention: group size %d (1..16)", g);
    QA_REQUIRE(hd == 64 || hd == 128, QUIPAMD_ERR_UNSUPPORTED, "prefill_attention: head_dim %d (64 or 128)", hd);
    QA_REQUIRE(maxlen <= 32768, QUIPAMD_ERR_SHAPE, "prefill_attention: maxlen %lld > 32768", (long long)maxlen);
    QA_REQUIRE(dtype == QUIPAMD_F16 || dtype == QUIPAMD_BF16, QUIPAMD_ERR_UNSUPPORTED, "prefill_attention: f16 / bf16 only");
    if (bs == 0) return QUIPAMD_OK;
    QA_REQUIRE(q && k && v && kcache && vcache && start && out, QUIPAMD_ERR_ARG, "prefill_attention: null pointer");
    QA_REQUIRE((cos_table == nullptr) == (sin_table == nullptr) && (!cos_table || table_rows > 0), QUIPAMD_ERR_ARG,
               "prefill_attention: rotary tables (both or neither, table_rows > 0)");
    QA_REQUIRE(ldq >= (int64_t)heads * hd && ldk >= (int64_t)kv_heads * hd && ldv >= (int64_t)kv_heads * hd && ldq % 8 == 0 && ldk % 8 == 0 &&
               ldv % 8 == 0, QUIPAMD_ERR_SHAPE, "prefill_attention: row strides %lld / %lld / %lld (multiples of 8, at least a row)",
               (long long)ldq, (long long)ldk, (long long)ldv);
    QA_REQUIRE((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)kcache | (uintptr_t)vcache | (uintptr_t)out) & 15) == 0, QUIPAMD_ERR_ARG,
               "prefill_attention: pointers must be 16-byte aligned");
    QA_REQUIRE(heads <= 65535 && bs <= 65535 && bs * T * kv_heads * (hd / 2) < ((int64_t)1 << 39), QUIPAMD_ERR_SHAPE,
               "prefill_attention: grid too large");
    PfArgs A;
    A.q = (const uint16_t *)q; A.k = (const uint16_t *)k; A.v = (const uint16_t *)v;
    A.kc = (uint16_t *)kcache; A.vc = (uint16_t *)vcache; A.out = (uint16_t *)out; A.start = start;
    A.cos_t = cos_table; A.sin_t = sin_table;
    A.table_rows = cos_table ? table_rows : 0; A.maxlen = maxlen; A.ldq = ldq; A.ldk = ldk; A.ldv = ldv; A.T = T;
    A.heads = heads; A.kv = kv_heads; A.g = g; A.scale = scale;
    hipStream_t s = (hipStream_t)stream;
    return dtype == QUIPAMD_F16 ? pf_launch<F16>(A, bs, hd, s) : pf_launch<BF16>(A, bs, hd, s);
}
