// sample_body.h -- the device code of token sampling, shared by decode_sample.hip (quipamd_sample_rows) and decode_generate.hip
// (quipamd_generate_rows): ONE copy of the arithmetic.  decode_sample.hip's header comment describes the passes; sample_row() below is
// those passes for one row, run by the 1024 threads of its workgroup.
//
// PEN (a template flag of everything that reads the row): the entry of index i is penalised as it is loaded when bit i of `pen.seen` is
// set -- x < 0 ? x * p : x / p in fp32 (Hugging Face's RepetitionPenaltyLogitsProcessor) -- so every pass sees the same penalised row and the
// logits themselves are never written.  PEN false is the code as it was before the flag existed: `pen` is not looked at.
#pragma once
#include "common.h"

namespace {

typedef unsigned long long u64;

constexpr int SEG = 512;                 // entries per segment
constexpr int SAMPLE_MAX_N = 262144;     // 512 segments: the per-segment arrays of the draw
constexpr int L1_BINS = 4096, LX_BINS = 1024;
constexpr uint32_t NONE = 0xffffffffu;

// first output word of Philox4x32-10 (Salmon et al., SC'11): key (lo, hi of seed), counter (lo, hi of ctr, row, 0)
__device__ __forceinline__ uint32_t philox_x0(u64 seed, u64 ctr, uint32_t row)
{
    uint32_t c0 = (uint32_t)ctr, c1 = (uint32_t)(ctr >> 32), c2 = row, c3 = 0;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c0;
}

__device__ __forceinline__ float z_of(float x, float T)
{
    const float z = x / T;
    return z == 0.f ? 0.f : z;           // -0 and +0 are one value in the order
}
// ascending key = descending z
__device__ __forceinline__ uint32_t key_of(float z)
{
    const uint32_t b = __float_as_uint(z);
    return ~(b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u));
}
// the weight exp(z - m) <= 1 in 2^-40 fixed point (NaN -> 0)
__device__ __forceinline__ u64 q_of(float z, float m)
{
    const float w = __expf(z - m);
    return w > 0.f ? (u64)(w * 0x1p40f) : 0ull;
}

// the repetition penalty: one bit per vocabulary entry (LDS), and p
struct Pen {
    const uint32_t *seen;
    float p;
};
__device__ __forceinline__ float pen_of(float x, int i, const Pen &pen)
{
    if ((pen.seen[i >> 5] >> (i & 31)) & 1u) return x < 0.f ? x * pen.p : x / pen.p;
    return x;
}
// entry i of the row as every pass sees it (i < n)
template <class TI, bool PEN> __device__ __forceinline__ float load_one(const typename DT<TI>::storage *row, int n, int i, const Pen &pen)
{
    const float x = DT<TI>::load(row, i < n ? i : n - 1);
    if constexpr (PEN) return i < n ? pen_of(x, i, pen) : x;
    return x;
}

// one segment of the row: x[e] and its index.  16-bit rows on 16-byte boundaries: lane l holds entries base + 8 l .. + 7 of a full
// segment; otherwise entry base + 64 e + l, the address clamped to the row (idx >= n marks what is not there)
template <class TI, bool PEN>
__device__ __forceinline__ void load_seg(const typename DT<TI>::storage *row, int n, int vec, int seg, int lane, const Pen &pen, float (&x)[8], int (&idx)[8])
{
    const int base = seg * SEG;
    if constexpr (sizeof(typename DT<TI>::storage) == 2) {
        if (vec && base + SEG <= n) {
            const uint4 v = *reinterpret_cast<const uint4 *>(row + base + 8 * lane);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const typename DT<TI>::storage h = (typename DT<TI>::storage)(w[e >> 1] >> (16 * (e & 1)));
                x[e] = DT<TI>::load(&h, 0);
                idx[e] = base + 8 * lane + e;
                if constexpr (PEN) x[e] = pen_of(x[e], idx[e], pen);
            }
            return;
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int i = base + 64 * e + lane;
        x[e] = load_one<TI, PEN>(row, n, i, pen);
        idx[e] = i;
    }
}

// wave sum of a uint32 on the DPP network (wavered.h's pattern on integers); every lane active, every lane gets the sum
template <int CTRL> __device__ __forceinline__ uint32_t dpp_u(uint32_t x) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xf, 0xf, true); }
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v)
{
    v += dpp_u<0xB1>(v);
    v += dpp_u<0x4E>(v);
    v += dpp_u<0x141>(v);
    v += dpp_u<0x140>(v);
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 0) + (uint32_t)__builtin_amdgcn_readlane((int)v, 16) + (uint32_t)__builtin_amdgcn_readlane((int)v, 32) +
           (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
}
// a lane's mass is below 2^44: 64 of its 22-bit halves sum inside 32 bits
__device__ __forceinline__ u64 wave_sum_mass(u64 v)
{
    const uint32_t lo = wave_sum_u32((uint32_t)v & 0x3fffffu), hi = wave_sum_u32((uint32_t)(v >> 22));
    return ((u64)hi << 22) + lo;
}

__device__ __forceinline__ u64 shfl_up64(u64 v, int off)
{
    const uint32_t lo = __shfl_up((uint32_t)v, off), hi = __shfl_up((uint32_t)(v >> 32), off);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 shfl64(u64 v, int src)
{
    const uint32_t lo = __shfl((uint32_t)v, src), hi = __shfl((uint32_t)(v >> 32), src);
    return ((u64)hi << 32) | lo;
}

struct CM { uint32_t c; u64 m; };        // a count and a mass

struct Shared {
    u64 h1m[L1_BINS];                    // 12-bit digit: mass and count per bin, whole row
    uint32_t h1c[L1_BINS];
    u64 hxm[LX_BINS];                    // a 10-bit digit inside the threshold bin; the draw: mass per segment
    uint32_t hxc[LX_BINS];               //                                           the draw: ties per segment
    u64 s_m[16];
    uint32_t s_c[16];
    float bv[16];
    int bi[16];
    uint32_t r_bin, r_cb, r_c, r_cnt;    // what a search found: bin, count before it, its count
    u64 r_mb, r_m;                       //                      mass before it, its mass
    int r_tok;
};

// exclusive scan over the 1024 threads (threads in order) and the total; two barriers
__device__ __forceinline__ void block_scan(Shared &S, CM v, CM &excl, CM &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    CM inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t oc = __shfl_up(inc.c, off);
        const u64 om = shfl_up64(inc.m, off);
        if (lane >= off) { inc.c += oc; inc.m += om; }
    }
    if (lane == 63) { S.s_c[wave] = inc.c; S.s_m[wave] = inc.m; }
    __syncthreads();
    CM base = {0, 0};
    total = {0, 0};
#pragma unroll
    for (int w = 0; w < 16; ++w) {
        const uint32_t c = S.s_c[w];
        const u64 m = S.s_m[w];
        if (w < wave) { base.c += c; base.m += m; }
        total.c += c; total.m += m;
    }
    __syncthreads();
    excl.c = base.c + inc.c - v.c;
    excl.m = base.m + inc.m - v.m;
}

// the bin the cut lies in, bins ascending, with `before` in front of bin 0.  by count: the bin that holds the entry of rank `target`
// (1-based); by mass: the first bin whose inclusive mass reaches `target`.  Leaves S.r_* (r_bin == NONE: no such bin); returns the total.
template <int NB> __device__ __forceinline__ CM find_bin(Shared &S, const uint32_t *hc, const u64 *hm, bool by_mass, u64 target, CM before)
{
    constexpr int BPT = NB / 1024;
    const int tid = threadIdx.x;
    uint32_t c[BPT];
    u64 m[BPT];
    CM mine = {0, 0};
#pragma unroll
    for (int j = 0; j < BPT; ++j) {
        c[j] = hc[tid * BPT + j];
        m[j] = hm[tid * BPT + j];
        mine.c += c[j];
        mine.m += m[j];
    }
    if (tid == 0) S.r_bin = NONE;
    CM run, total;
    block_scan(S, mine, run, total);
    run.c += before.c;
    run.m += before.m;
#pragma unroll
    for (int j = 0; j < BPT; ++j) {
        if (c[j]) {
            const bool hit = by_mass ? (run.m < target && run.m + m[j] >= target) : ((u64)run.c < target && target <= (u64)run.c + c[j]);
            if (hit) { S.r_bin = tid * BPT + j; S.r_cb = run.c; S.r_mb = run.m; S.r_c = c[j]; S.r_m = m[j]; }
        }
        run.c += c[j];
        run.m += m[j];
    }
    __syncthreads();
    return total;
}

// histogram of the digit (key >> dshift) & (nb - 1) over the candidates (ALL: every one; else those with key >> pshift == prefix)
template <class TI, bool ALL, bool PEN>
__device__ __forceinline__ void hist_pass(Shared &S, const typename DT<TI>::storage *row, int n, int vec, const Pen &pen, float T, float m, uint32_t pshift,
                                          uint32_t prefix, uint32_t dshift, int nb, uint32_t *hc, u64 *hm)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < nb; i += 1024) { hc[i] = 0; hm[i] = 0; }
    __syncthreads();
    const int nseg = (n + SEG - 1) / SEG;
    for (int seg = wave; seg < nseg; seg += 16) {
        float x[8];
        int idx[8];
        load_seg<TI, PEN>(row, n, vec, seg, lane, pen, x, idx);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float z = z_of(x[e], T);
            const uint32_t key = key_of(z);
            if (idx[e] < n && z > -INFINITY && (ALL || (key >> pshift) == prefix)) {
                const uint32_t d = (key >> dshift) & (uint32_t)(nb - 1);
                atomicAdd(&hc[d], 1u);
                const u64 q = q_of(z, m);
                if (q) atomicAdd(&hm[d], q);
            }
        }
    }
    __syncthreads();
}

struct Cut {                             // survivors: key < cut.key, and the first `ties` entries (by index) with key == cut.key
    uint32_t key, ties, cnt;             // cnt, mass: of the survivors
    u64 mass, qt;                        // qt: the weight of an entry at cut.key
};

// the cut by rank (by_mass false: the first `target` entries) or by mass (the smallest prefix whose mass reaches `target`), from the
// 12-bit histogram of the whole row in S.h1*; false when there is none (fewer candidates / less mass than asked for)
template <class TI, bool PEN>
__device__ __forceinline__ bool select_cut(Shared &S, const typename DT<TI>::storage *row, int n, int vec, const Pen &pen, float T, float m, bool by_mass,
                                           u64 target, Cut &cut)
{
    find_bin<L1_BINS>(S, S.h1c, S.h1m, by_mass, target, CM{0, 0});
    if (S.r_bin == NONE) return false;
    const uint32_t b1 = S.r_bin;
    CM before = {S.r_cb, S.r_mb};
    __syncthreads();                                                             // S.r_* are read: the next search may write them
    hist_pass<TI, false, PEN>(S, row, n, vec, pen, T, m, 20, b1, 10, LX_BINS, S.hxc, S.hxm);
    find_bin<LX_BINS>(S, S.hxc, S.hxm, by_mass, target, before);
    if (S.r_bin == NONE) return false;
    const uint32_t b2 = S.r_bin;
    before = {S.r_cb, S.r_mb};
    __syncthreads();
    hist_pass<TI, false, PEN>(S, row, n, vec, pen, T, m, 10, (b1 << 10) | b2, 0, LX_BINS, S.hxc, S.hxm);
    find_bin<LX_BINS>(S, S.hxc, S.hxm, by_mass, target, before);
    if (S.r_bin == NONE) return false;
    const uint32_t b3 = S.r_bin, c3 = S.r_c;
    const u64 m3 = S.r_m;
    before = {S.r_cb, S.r_mb};
    __syncthreads();
    cut.key = (b1 << 20) | (b2 << 10) | b3;
    cut.qt = m3 / c3;                                                            // equal keys are equal weights
    if (by_mass) {
        const u64 need = target - before.m;                                      // > 0; entry j of the ties survives iff before + j qt < target
        const u64 t = cut.qt ? (need + cut.qt - 1) / cut.qt : (u64)c3;
        cut.ties = (uint32_t)(t < c3 ? t : c3);
    } else {
        cut.ties = (uint32_t)(target - before.c);
    }
    cut.cnt = before.c + cut.ties;
    cut.mass = before.m + (u64)cut.ties * cut.qt;
    return true;
}

// One row, by the 1024 threads of its workgroup: temperature T, top-k K, top-p P; the draw is Philox(*seed; *counter, r), both read only
// when something is drawn.  Every thread returns the same tok / lp / kn / kmass.
template <class TI, bool PEN>
__device__ __forceinline__ void sample_row(Shared &S, const typename DT<TI>::storage *row, int n, int vec, const Pen &pen, float T, float P, int K,
                                           const uint64_t *seed, const int64_t *counter, uint32_t r, int &tok, float &lp, int &kn, float &kmass)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nseg = (n + SEG - 1) / SEG;

    // ---- pass 0: the maximum and its first index, argmax_rows' comparison on the logits as they are ---------------------------------
    float best = -INFINITY;
    int gidx = 0x7fffffff;
    for (int seg = wave; seg < nseg; seg += 16) {
        float x[8];
        int idx[8];
        load_seg<TI, PEN>(row, n, vec, seg, lane, pen, x, idx);
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (idx[e] < n && (x[e] > best || (x[e] == best && idx[e] < gidx))) { best = x[e]; gidx = idx[e]; }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float ov = __shfl_xor(best, off);
        const int oi = __shfl_xor(gidx, off);
        if (ov > best || (ov == best && oi < gidx)) { best = ov; gidx = oi; }
    }
    if (lane == 0) { S.bv[wave] = best; S.bi[wave] = gidx; }
    if (tid == 0) S.r_cnt = 0;
    __syncthreads();
    best = S.bv[0];
    gidx = S.bi[0];
#pragma unroll
    for (int w = 1; w < 16; ++w)
        if (S.bv[w] > best || (S.bv[w] == best && S.bi[w] < gidx)) { best = S.bv[w]; gidx = S.bi[w]; }
    if (gidx < 0 || gidx >= n) gidx = 0;

    tok = gidx;
    lp = 0.f;
    kmass = 1.f;
    kn = 1;
    if (T > 0.f && K != 1) {
        const float m = z_of(best, T);
        const bool k_on = K > 0 && K < n, p_on = P < 1.f;
        Cut cut = {NONE, 0, 0, 0, 0};                                            // no truncation: every candidate survives
        if (k_on || p_on) {
            hist_pass<TI, true, PEN>(S, row, n, vec, pen, T, m, 0, 0, 20, L1_BINS, S.h1c, S.h1m);
            u64 zk = 0;
            bool have = false;
            if (k_on) {
                have = select_cut<TI, PEN>(S, row, n, vec, pen, T, m, false, (u64)K, cut);
                zk = cut.mass;
            }
            if (!have) {                                                         // top-k off, or no more than top_k candidates: the whole row
                u64 part = 0;
                for (int i = tid; i < L1_BINS; i += 1024) part += S.h1m[i];
                CM ex, tot;
                block_scan(S, CM{0, part}, ex, tot);
                zk = tot.m;
                cut = {NONE, 0, 0, 0, 0};
            }
            if (p_on && zk > 0) {
                const double want = ceil((double)P * (double)zk);                // entry survives iff mass before it < top_p * zk
                u64 tp = want >= 1.0 ? (u64)want : 1ull;
                tp = tp < zk ? tp : zk;
                Cut pc;
                if (select_cut<TI, PEN>(S, row, n, vec, pen, T, m, true, tp, pc)) {   // never longer than the top-k prefix: that one's mass is zk >= tp
                    cut = pc;
                    kmass = (float)((double)pc.mass / (double)zk);
                }
            }
        }

        // ---- the draw: survivors' mass per segment, in index order ---------------------------------------------------------------------
        u64 *segm = S.hxm;
        uint32_t *segt = S.hxc;
        for (int seg = wave; seg < nseg; seg += 16) {
            float x[8];
            int idx[8];
            load_seg<TI, PEN>(row, n, vec, seg, lane, pen, x, idx);
            u64 sm = 0;
            uint32_t st = 0, sc = 0;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float z = z_of(x[e], T);
                const uint32_t key = key_of(z);
                if (idx[e] < n && z > -INFINITY) {
                    if (key < cut.key) { sm += q_of(z, m); ++sc; }
                    st += key == cut.key;
                }
            }
            sm = wave_sum_mass(sm);
            st = wave_sum_u32(st);
            sc = wave_sum_u32(sc);
            if (lane == 0) {
                segm[seg] = sm;
                segt[seg] = st;
                if (sc) atomicAdd(&S.r_cnt, sc);
            }
        }
        if (tid == 0) S.r_bin = NONE;
        __syncthreads();
        const CM mine = tid < nseg ? CM{segt[tid], segm[tid]} : CM{0, 0};
        CM ex, tot;
        block_scan(S, mine, ex, tot);
        auto ties_in = [&](uint32_t t) { return t < cut.ties ? t : cut.ties; };  // of the first t ties (by index), how many survive
        const u64 zf = tot.m + (u64)ties_in(tot.c) * cut.qt;
        kn = (int)(S.r_cnt + ties_in(tot.c));
        if (zf > 0) {
            const u64 ctr = (u64)*counter;
            const u64 U = philox_x0(*seed, ctr, r) >> 8;
            const u64 tg = (__umul64hi(U, zf) << 40) | ((U * zf) >> 24);         // floor(u Z): C_i > u Z  <=>  C_i > tg, and tg < Z
            const u64 e0 = ex.m + (u64)ties_in(ex.c) * cut.qt, e1 = ex.m + mine.m + (u64)ties_in(ex.c + mine.c) * cut.qt;
            if (tid < nseg && e0 <= tg && tg < e1) { S.r_bin = tid; S.r_mb = e0; S.r_cb = ex.c; }
            if (tid == 0) S.r_tok = -1;
            __syncthreads();
            const uint32_t sseg = S.r_bin;
            if (sseg != NONE && wave == 0) {                                     // one wave walks the segment, 64 consecutive entries at a time
                u64 run = S.r_mb, qtok = 0;
                uint32_t tb = S.r_cb;
                int found = -1;
                for (int e = 0; e < 8 && found < 0; ++e) {
                    const int i = (int)sseg * SEG + 64 * e + lane;
                    const float z = z_of(load_one<TI, PEN>(row, n, i, pen), T);
                    const uint32_t key = key_of(z);
                    const bool cand = i < n && z > -INFINITY, tie = cand && key == cut.key;
                    const u64 tmask = __ballot(tie);
                    const uint32_t rank = tb + (uint32_t)__popcll(tmask & ((1ull << lane) - 1ull));
                    const bool in = cand && (key < cut.key || (tie && rank < cut.ties));
                    const u64 q = in ? q_of(z, m) : 0ull;
                    u64 c = q;
#pragma unroll
                    for (int off = 1; off < 64; off <<= 1) {
                        const u64 o = shfl_up64(c, off);
                        if (lane >= off) c += o;
                    }
                    const u64 hit = __ballot(in && run + c > tg);
                    if (hit) {
                        const int src = __ffsll((long long)hit) - 1;
                        found = __shfl(i, src);
                        qtok = shfl64(q, src);
                    }
                    run += shfl64(c, 63);
                    tb += (uint32_t)__popcll(tmask);
                }
                if (lane == 0 && found >= 0) {
                    S.r_tok = found;
                    S.r_m = qtok;
                }
            }
            __syncthreads();
            if (S.r_tok >= 0) {
                tok = S.r_tok;
                lp = logf((float)S.r_m / (float)zf);
            }
        }
    }
}

}   // namespace
