// decode_gqa.hip -- single-token attention for grouped-query models (Llama-2-70B: 64 query heads share 8 key / value heads)
//
// One generated token per sequence: append this step's k, v (k rotated when rotary tables are given) to the static KV cache at
// position *pos, then for query head j of key / value head h = j / g (HF's repeat_kv order, g = heads / kv_heads):
//   o[b, j] = softmax(scale * q_j . K_h[0..pos]^T) V_h[0..pos].
// The point of the launch is the cache traffic: a workgroup serves the g query heads of ONE key / value head, so every cached K / V
// row is read once per (sequence, key / value head) and step -- repeating the cache out to `heads` (what the multi-head launch would
// need) reads it g times.
//
//   grid   bs * kv_heads * ceil(maxlen / 256) workgroups of 256 threads, sized from maxlen (never from pos: the launch is captured
//          once in a hipGraph and replayed while the position advances on the device).  Workgroup (sequence, kv head, chunk c)
//          serves positions [256 c, 256 c + 256); a chunk past pos leaves at once.
//   scores thread t owns position 256 c + t: its K row (16-byte loads) against the g rotated q rows held in LDS in the activation
//          dtype, fp32 accumulation on v_dot2_f32_{f16,bf16} (exact products); scale applied to the finished score.
//   softmax 16 threads per query head: chunk max, exp, chunk sum -- fp32, fixed order.
//   p V    lane = (row slot, E-element column chunk): one 16-byte (8-byte at g > 8) load covers several rows per instruction, eight
//          loads in flight; every lane accumulates all g heads for its elements, so a V row is read once for the group.
//   combine a single active chunk (pos < 256) writes o directly.  Otherwise every active chunk writes its partial (unnormalised o,
//          max, sum; fp32) to the caller's workspace, releases it at agent scope and adds to the (sequence, kv head) counter; the
//          workgroup whose add comes last acquires, merges the partials in chunk order 0, 1, ... (never in arrival order: two runs
//          are bit-identical) and re-arms the counter for the next launch.  Plain vector loads / stores and one vector atomic.
// LDS is static and independent of maxlen: (g <= 16, hd 128) 52 KB, (g <= 8, hd 128) 26 KB.
#include "common.h"

namespace {

constexpr int GQ_C = 256;                               // cached positions per workgroup: one per thread in the scores phase
constexpr int GQ_MAXCH = 32768 / GQ_C;                  // chunks at the largest supported maxlen

typedef _Float16 gq_f16x2 __attribute__((ext_vector_type(2)));

template <class TI> struct GqDot;
template <> struct GqDot<F16> {
    static __device__ __forceinline__ float dot2(uint32_t a, uint32_t b, float c)
    {
        return __builtin_amdgcn_fdot2(__builtin_bit_cast(gq_f16x2, a), __builtin_bit_cast(gq_f16x2, b), c, false);
    }
};
template <> struct GqDot<BF16> {
    static __device__ __forceinline__ float dot2(uint32_t a, uint32_t b, float c)
    {
        return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, a), __builtin_bit_cast(bf16x2_t, b), c, false);
    }
};

template <int E> struct GqVec;                          // the p V load of one lane: E 16-bit elements
template <> struct GqVec<8> { typedef uint4 T; };
template <> struct GqVec<4> { typedef uint2 T; };

struct GqaArgs {
    const uint16_t *q, *k, *v;            // [bs, heads * hd] (ldq), [bs, kv_heads * hd] (ldk, ldv)
    uint16_t *kc, *vc, *out;              // [bs, kv_heads, maxlen, hd]; out [bs, heads * hd] contiguous
    const int64_t *pos;
    const float *cos_t, *sin_t;           // rotary tables [table_rows, hd] or null
    int *cnt;                             // workspace: arrival counters [bs * kv_heads] (zero between launches)
    float *part;                          // workspace: partials [bs * kv_heads][nch][slot]
    int64_t table_rows, maxlen, ldq, ldk, ldv, slot;
    int kv, g, nch;
    float scale;
};

template <class TI, int HD, int GM>
__global__ __launch_bounds__(256) void gqa_kernel(GqaArgs A)
{
    typedef uint16_t S;
    constexpr int E = GM <= 8 ? 8 : 4;                  // V elements per lane in p V (g > 8: 4, so that g x E accumulators fit)
    constexpr int CH = HD / E, RS = 64 / CH;            // lanes per V row, rows per wave instruction
    constexpr int NV = GQ_C / (4 * RS);                 // V loads per lane over the chunk
    constexpr int NO = (GM * HD + 255) / 256;           // output elements of the group per thread
    static_assert(NV % 8 == 0 && GM % 4 == 0 && GM <= 16, "tiling");
    typedef typename GqVec<E>::T VT;
    __shared__ __attribute__((aligned(16))) S qs[GM * HD];                // q of the group, rotated, in the activation dtype
    __shared__ __attribute__((aligned(16))) float sc[GQ_C * GM];          // scores -> probabilities [row][head]; later the merge weights
    __shared__ __attribute__((aligned(16))) float pw[4 * GM * HD];        // the four waves' p V
    __shared__ float ml[2 * GM];                                          // max, sum per head
    __shared__ int last;
    static_assert(GQ_MAXCH * GM <= GQ_C * GM, "merge weights reuse the score buffer");

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = (int)(blockIdx.x % (unsigned)A.nch);
    const int64_t bk = blockIdx.x / (unsigned)A.nch;                     // sequence * kv_heads + kv head
    const int64_t b = bk / A.kv;
    const int kvh = (int)(bk % A.kv), g = A.g;
    const int64_t pos = *A.pos;
    if (pos < 0 || pos >= A.maxlen) return;                               // uniform: no append, no write
    const int nact = (int)(pos / GQ_C) + 1;                               // chunks that hold positions 0..pos
    if (c >= nact) return;
    const int64_t t0 = (int64_t)c * GQ_C;
    S *kcb = A.kc + bk * A.maxlen * HD, *vcb = A.vc + bk * A.maxlen * HD;
    const bool rot = A.cos_t != nullptr && pos < A.table_rows;            // past the tables: no rotation (like quipamd_rope_inplace)

    // q rows of the group (heads kvh g .. kvh g + g - 1, adjacent in q's row), rotated with rope_kernel's fp32 expression
    const S *qg = A.q + b * A.ldq + (int64_t)kvh * g * HD;
    for (int i = tid; i < g * (HD / 2); i += 256) {
        const int j = i / (HD / 2), e = i % (HD / 2);
        const float a = DT<TI>::load(qg, j * HD + e), bb = DT<TI>::load(qg, j * HD + e + HD / 2);
        if (rot) {
            const float cc = A.cos_t[pos * HD + e], ss = A.sin_t[pos * HD + e];
            DT<TI>::store(qs, j * HD + e, a * cc - bb * ss);
            DT<TI>::store(qs, j * HD + e + HD / 2, bb * cc + a * ss);
        } else {
            qs[j * HD + e] = qg[j * HD + e];
            qs[j * HD + e + HD / 2] = qg[j * HD + e + HD / 2];
        }
    }
    // the chunk that holds pos appends this token (k rotated: bit-identical to quipamd_rope_inplace followed by a copy); the barrier
    // makes the row visible to this workgroup's reads below, and no other workgroup reads it
    if (c == nact - 1) {
        if (tid < HD / 2) {
            const S *kn = A.k + b * A.ldk + (int64_t)kvh * HD;
            const float a = DT<TI>::load(kn, tid), bb = DT<TI>::load(kn, tid + HD / 2);
            S *dst = kcb + pos * HD;
            if (rot) {
                const float cc = A.cos_t[pos * HD + tid], ss = A.sin_t[pos * HD + tid];
                DT<TI>::store(dst, tid, a * cc - bb * ss);
                DT<TI>::store(dst, tid + HD / 2, bb * cc + a * ss);
            } else {
                dst[tid] = kn[tid];
                dst[tid + HD / 2] = kn[tid + HD / 2];
            }
        } else if (tid >= 128 && tid < 128 + HD) {
            vcb[pos * HD + tid - 128] = A.v[b * A.ldv + (int64_t)kvh * HD + tid - 128];
        }
    }
    __syncthreads();

    // ---- scores: thread tid owns position t0 + tid --------------------------------------------------------------------------------
    {
        const int64_t t = t0 + tid;
        const bool valid = t <= pos;
        float acc[GM];
#pragma unroll
        for (int j = 0; j < GM; ++j) acc[j] = 0.f;
        if (valid) {
            const S *row = kcb + t * HD;
            uint4 kr[HD / 8];
#pragma unroll
            for (int e8 = 0; e8 < HD / 8; ++e8) kr[e8] = *reinterpret_cast<const uint4 *>(row + 8 * e8);
#pragma unroll
            for (int e8 = 0; e8 < HD / 8; ++e8) {
#pragma unroll
                for (int j = 0; j < GM; ++j) {
                    if (j < g) {                                          // uniform
                        const uint4 q4 = *reinterpret_cast<const uint4 *>(qs + j * HD + 8 * e8);
                        acc[j] = GqDot<TI>::dot2(q4.x, kr[e8].x, acc[j]);
                        acc[j] = GqDot<TI>::dot2(q4.y, kr[e8].y, acc[j]);
                        acc[j] = GqDot<TI>::dot2(q4.z, kr[e8].z, acc[j]);
                        acc[j] = GqDot<TI>::dot2(q4.w, kr[e8].w, acc[j]);
                    }
                }
            }
        }
#pragma unroll
        for (int j4 = 0; j4 < GM; j4 += 4)
            *reinterpret_cast<float4 *>(sc + tid * GM + j4) =
                valid ? make_float4(acc[j4] * A.scale, acc[j4 + 1] * A.scale, acc[j4 + 2] * A.scale, acc[j4 + 3] * A.scale)
                      : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    }
    __syncthreads();

    // ---- softmax of the chunk: 16 threads per query head, fixed order ---------------------------------------------------------------
    {
        const int j = tid >> 4, s16 = tid & 15;
        float m = -INFINITY, l = 0.f;
        if (j < g)
            for (int r = s16; r < GQ_C; r += 16) m = fmaxf(m, sc[r * GM + j]);
#pragma unroll
        for (int off = 8; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
        if (j < g)
            for (int r = s16; r < GQ_C; r += 16) {                       // (row 0 of an active chunk is <= pos: m is finite)
                const float p = __expf(sc[r * GM + j] - m);
                sc[r * GM + j] = p;
                l += p;
            }
#pragma unroll
        for (int off = 8; off >= 1; off >>= 1) l += __shfl_xor(l, off);
        if (s16 == 0 && j < g) {
            ml[j] = m;
            ml[GM + j] = l;
        }
    }
    __syncthreads();

    // ---- p V: wave w takes rows w RS + 4 RS u + rsub; each lane E columns of every head of the group ----------------------------------
    const int ch = lane % CH, rsub = lane / CH;
    const int64_t nrow = pos - t0 + 1 < GQ_C ? pos - t0 + 1 : GQ_C;        // rows of the chunk at or before pos
    float o[GM][E];
#pragma unroll
    for (int j = 0; j < GM; ++j)
#pragma unroll
        for (int e = 0; e < E; ++e) o[j][e] = 0.f;
#pragma unroll
    for (int u0 = 0; u0 < NV; u0 += 8) {
        VT raw[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int r = wave * RS + (u0 + u) * 4 * RS + rsub;
            if (r < nrow) raw[u] = *reinterpret_cast<const VT *>(vcb + (t0 + r) * HD + E * ch);
            else raw[u] = VT{};
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int r = wave * RS + (u0 + u) * 4 * RS + rsub;          // (< GQ_C; a row past pos has p = 0 and V = 0)
            const S *rv = reinterpret_cast<const S *>(&raw[u]);
            float vf[E];
#pragma unroll
            for (int e = 0; e < E; ++e) vf[e] = DT<TI>::load(rv, e);
#pragma unroll
            for (int j4 = 0; j4 < GM; j4 += 4) {
                if (j4 < g) {
                    const float4 p4 = *reinterpret_cast<const float4 *>(sc + r * GM + j4);
                    const float pj[4] = {p4.x, p4.y, p4.z, p4.w};
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                        for (int e = 0; e < E; ++e) o[j4 + jj][e] = fmaf(pj[jj], vf[e], o[j4 + jj][e]);
                }
            }
        }
    }
    // rows of one column chunk sit CH lanes apart: fold the row slots, then the four waves through LDS
#pragma unroll
    for (int off = CH; off < 64; off <<= 1)
#pragma unroll
        for (int j = 0; j < GM; ++j)
#pragma unroll
            for (int e = 0; e < E; ++e) o[j][e] += __shfl_xor(o[j][e], off);
    if (rsub == 0) {
#pragma unroll
        for (int j = 0; j < GM; ++j)
            if (j < g)
#pragma unroll
                for (int e = 0; e < E; ++e) pw[(wave * GM + j) * HD + E * ch + e] = o[j][e];
    }
    __syncthreads();
    float oc[NO];
#pragma unroll
    for (int i = 0; i < NO; ++i) {
        const int idx = tid + 256 * i;                                    // (head j = idx / HD, element idx % HD)
        oc[i] = idx < g * HD ? (pw[idx] + pw[GM * HD + idx]) + (pw[2 * GM * HD + idx] + pw[3 * GM * HD + idx]) : 0.f;
    }
    S *ob = A.out + b * (int64_t)A.kv * g * HD + (int64_t)kvh * g * HD;  // out rows are contiguous: [bs, heads * hd]
    if (nact == 1) {                                                      // the whole context is this chunk
#pragma unroll
        for (int i = 0; i < NO; ++i) {
            const int idx = tid + 256 * i;
            if (idx < g * HD) DT<TI>::store(ob, idx, oc[i] / ml[GM + idx / HD]);
        }
        return;
    }

    // ---- partial of this chunk -> workspace; the last of the (sequence, kv head)'s chunks to arrive merges them ---------------------
    float *slots = A.part + bk * A.nch * A.slot;
    float *mine = slots + (int64_t)c * A.slot;
#pragma unroll
    for (int i = 0; i < NO; ++i) {
        const int idx = tid + 256 * i;
        if (idx < g * HD) mine[idx] = oc[i];
    }
    if (tid < 2 * g) mine[g * HD + tid] = ml[tid < g ? tid : GM + tid - g];  // max [g], then sum [g]
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                      // every storing wave: its stores are done ...
    __syncthreads();                                                      // ... before the one lane that signals for all of them
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");                // the partials leave this XCD's L2
        const int prev = __hip_atomic_fetch_add(A.cnt + bk, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int is_last = prev == nact - 1;
        if (is_last) {
            __hip_atomic_store(A.cnt + bk, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // re-armed for the next launch / replay
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");            // this CU's L1 holds no stale partial
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        last = is_last;
    }
    __syncthreads();
    if (!last) return;
    float *wgt = sc;                                                      // merge weights [chunk][head]
    if (tid < g) {
        float M = -INFINITY, L = 0.f;
        for (int cc = 0; cc < nact; ++cc) M = fmaxf(M, slots[(int64_t)cc * A.slot + g * HD + tid]);
        for (int cc = 0; cc < nact; ++cc) {
            const float w = __expf(slots[(int64_t)cc * A.slot + g * HD + tid] - M);
            wgt[cc * GM + tid] = w;
            L = fmaf(w, slots[(int64_t)cc * A.slot + g * HD + g + tid], L);
        }
        ml[GM + tid] = L;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NO; ++i) {
        const int idx = tid + 256 * i;
        if (idx < g * HD) {
            const int j = idx / HD;
            float acc = 0.f;
            for (int cc = 0; cc < nact; ++cc) acc = fmaf(wgt[cc * GM + j], slots[(int64_t)cc * A.slot + idx], acc);
            DT<TI>::store(ob, idx, acc / ml[GM + j]);
        }
    }
}

int64_t gqa_chunks(int64_t maxlen) { return (maxlen + GQ_C - 1) / GQ_C; }
int64_t gqa_slot(int g, int hd) { return ((int64_t)g * hd + 2 * g + 31) / 32 * 32; }       // floats, 128-byte slots
int64_t gqa_counter_bytes(int64_t pairs) { return (pairs * 4 + 255) / 256 * 256; }

template <class TI, int HD> int launch_gqa_hd(const GqaArgs &A, int64_t bs, hipStream_t s)
{
    const unsigned grid = (unsigned)(bs * A.kv * A.nch);
    if (A.g <= 4) gqa_kernel<TI, HD, 4><<<grid, 256, 0, s>>>(A);
    else if (A.g <= 8) gqa_kernel<TI, HD, 8><<<grid, 256, 0, s>>>(A);
    else gqa_kernel<TI, HD, 16><<<grid, 256, 0, s>>>(A);
    QA_LAUNCH_CHECK("decode_attention_grouped");
    return QUIPAMD_OK;
}

}   // namespace

extern "C" int64_t quipamd_decode_attention_grouped_workspace_bytes(int64_t bs, int heads, int kv_heads, int hd, int64_t maxlen)
{
    if (bs <= 0 || heads <= 0 || kv_heads <= 0 || heads % kv_heads != 0 || hd <= 0 || maxlen <= 0) return 0;
    const int64_t nch = gqa_chunks(maxlen);
    if (nch <= 1) return 0;                                               // one chunk: o is written directly
    return gqa_counter_bytes(bs * kv_heads) + bs * kv_heads * nch * gqa_slot(heads / kv_heads, hd) * (int64_t)sizeof(float);
}

extern "C" int quipamd_decode_attention_grouped(const void *q, const void *k, const void *v, void *kcache, void *vcache, const int64_t *pos,
                                                void *out, const float *cos_table, const float *sin_table, int64_t table_rows, int dtype,
                                                int64_t bs, int heads, int kv_heads, int hd, int64_t maxlen, float scale, int64_t ldq,
                                                int64_t ldk, int64_t ldv, void *workspace, int64_t workspace_bytes, void *stream)
{
    QA_REQUIRE(bs >= 0 && heads > 0 && kv_heads > 0 && maxlen > 0, QUIPAMD_ERR_SHAPE, "decode_attention_grouped: bad shape");
    QA_REQUIRE(heads % kv_heads == 0, QUIPAMD_ERR_SHAPE, "decode_attention_grouped: heads %d is not a multiple of kv_heads %d", heads, kv_heads);
    const int g = heads / kv_heads;
    QA_REQUIRE(g >= 2 && g <= 16, QUIPAMD_ERR_UNSUPPORTED, "decode_attention_grouped: group size %d (2..16; g = 1 is quipamd_decode_attention)", g);
    QA_REQUIRE(hd == 64 || hd == 128, QUIPAMD_ERR_UNSUPPORTED, "decode_attention_grouped: head_dim %d (64 or 128)", hd);
    QA_REQUIRE(maxlen <= 32768, QUIPAMD_ERR_SHAPE, "decode_attention_grouped: maxlen %lld > 32768", (long long)maxlen);
    QA_REQUIRE(dtype == QUIPAMD_F16 || dtype == QUIPAMD_BF16, QUIPAMD_ERR_UNSUPPORTED, "decode_attention_grouped: f16 / bf16 only");
    if (bs == 0) return QUIPAMD_OK;
    QA_REQUIRE(q && k && v && kcache && vcache && pos && out, QUIPAMD_ERR_ARG, "decode_attention_grouped: null pointer");
    QA_REQUIRE((cos_table == nullptr) == (sin_table == nullptr) && (!cos_table || table_rows > 0), QUIPAMD_ERR_ARG,
               "decode_attention_grouped: rotary tables (both or neither, table_rows > 0)");
    QA_REQUIRE(ldq >= (int64_t)heads * hd && ldk >= (int64_t)kv_heads * hd && ldv >= (int64_t)kv_heads * hd && ldq % 8 == 0 && ldk % 8 == 0 &&
               ldv % 8 == 0, QUIPAMD_ERR_SHAPE, "decode_attention_grouped: row strides %lld / %lld / %lld", (long long)ldq, (long long)ldk,
               (long long)ldv);
    QA_REQUIRE((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)kcache | (uintptr_t)vcache | (uintptr_t)out) & 15) == 0, QUIPAMD_ERR_ARG,
               "decode_attention_grouped: pointers must be 16-byte aligned");
    const int64_t nch = gqa_chunks(maxlen);
    QA_REQUIRE(bs * kv_heads * nch < (int64_t)1 << 31, QUIPAMD_ERR_SHAPE, "decode_attention_grouped: grid too large");
    const int64_t need = quipamd_decode_attention_grouped_workspace_bytes(bs, heads, kv_heads, hd, maxlen);
    QA_REQUIRE(need == 0 || (workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= need), QUIPAMD_ERR_ARG,
               "decode_attention_grouped: workspace of %lld bytes (16-byte aligned, zero-filled before the first launch) needed", (long long)need);
    GqaArgs A;
    A.q = (const uint16_t *)q; A.k = (const uint16_t *)k; A.v = (const uint16_t *)v;
    A.kc = (uint16_t *)kcache; A.vc = (uint16_t *)vcache; A.out = (uint16_t *)out; A.pos = pos;
    A.cos_t = cos_table; A.sin_t = sin_table;
    A.cnt = need ? (int *)workspace : nullptr;
    A.part = need ? (float *)((char *)workspace + gqa_counter_bytes(bs * kv_heads)) : nullptr;
    A.table_rows = cos_table ? table_rows : 0; A.maxlen = maxlen; A.ldq = ldq; A.ldk = ldk; A.ldv = ldv; A.slot = gqa_slot(g, hd);
    A.kv = kv_heads; A.g = g; A.nch = (int)nch; A.scale = scale;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == QUIPAMD_F16) return hd == 64 ? launch_gqa_hd<F16, 64>(A, bs, s) : launch_gqa_hd<F16, 128>(A, bs, s);
    return hd == 64 ? launch_gqa_hd<BF16, 64>(A, bs, s) : launch_gqa_hd<BF16, 128>(A, bs, s);
}
