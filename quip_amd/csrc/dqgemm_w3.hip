// dqgemm_w3.hip -- K2 on the STREAM3 layout: the fused dequant-GEMM for 3-bit codes stored at 3 bits per weight
// (include/quip_amd.h; tests/stream3_spec.py is the layout's specification).
//
// The kernel is dq_s_kernel's engine (dqgemm_v2.h) with a second weight plane: loader waves own the DMA queue and fill a D-deep LDS ring
// behind counted vmcnt waits, compute waves touch nothing but LDS, one barrier per ring step.  A ring step is SPS = KSP * SPW stages of
// 256 k; per stage and row tile the weight loader brings the 1 KiB low tile (the 2-bit STREAM tile of code & 3) and, per PAIR of stages,
// one 1 KiB transfer of high bits (64 lanes x 16 B = two consecutive chunks), so SPS is even in every configuration and a ring step of two
// stages reads ONE contiguous 3 KiB block per row tile.  An odd chunk count (11008 = 43 x 256) ends in an unpaired chunk whose 512 bytes of
// high bits are read twice (lanes 32..63 repeat lanes 0..31).  No transfer leaves its row tile.
//
// Dequantisation, per lane and chunk (4 low dwords L[u], 2 high dwords H[w]; 32 output dwords of 2 halves each):
//     E[u] = bfi(0x33333333, L[u],      H[u/2] shifted by {0, <<2}[u&1])      fields of even i as nibbles: code bits 0..2, one stray bit on top
//     O[u] = bfi(0x33333333, L[u] >> 2, H[u/2] shifted by {>>1, <<1}[u&1])    fields of odd i
// i.e. ONE bit-field insert rebuilds four 4-bit-container nibbles per half.  Step t = 2u + tp then takes nibbles 2 tp, 2 tp + 1 of E and O
// with a shared shift and one bfi per output dword onto two mantissa positions (multi-exponent form of dq_common.h: value = OFF + code,
// exact):       bf16: positions 0 / 4, OFF 128 / 8 (tp = 0: no shift; tp = 1: >> 8)      fp16: positions 3 / 7, OFF 128 / 8 (<< 3; >> 5)
// Output dword v of a step: v = 0 E low position, 1 O low, 2 E high, 3 O high -- the same offsets in every step, so S_off needs one constant
// fragment.  VALU per 256 k and lane: 18 to merge + 40 (bf16) / 48 (fp16) to place, against 64 for the nibbles of the 4-bit container.
// The epilogue is dq_common.h's (S_1, S_off on the matrix pipe, maxq = 7).
//
// bs > 16: blockIdx.y walks 16-row batch tiles, each streaming the weights again -- correct, not an MFMA-bound prefill kernel.
#include "dqgemm_v2.h"
#include "k2_dispatch.h"

namespace {

template <class ACT> struct W3Field;
template <> struct W3Field<ActBF16> { static constexpr int M = 7, BIAS = 127, P_LO = 0, P_HI = 4, SH0 = 0, SH1 = -8; };   // SH: left shift of the nibble word for tp = 0 / 1
template <> struct W3Field<ActF16> { static constexpr int M = 10, BIAS = 15, P_LO = 3, P_HI = 7, SH0 = 3, SH1 = -5; };

template <class ACT> struct DeqW3 {
    typedef W3Field<ACT> F;
    static constexpr uint32_t base_at(int p) { return (uint32_t)((F::BIAS + F::M - p) << F::M) * 0x10001u; }   // the encoding of OFF = 2^(M - p), both halves
    static constexpr uint32_t mask_at(int p) { return (7u << p) * 0x10001u; }
    struct Consts { uint32_t b[2]; };
    static __device__ __forceinline__ Consts make_consts()
    {
        Consts c;
        c.b[0] = opaque(base_at(F::P_LO));
        c.b[1] = opaque(base_at(F::P_HI));
        return c;
    }
    static __device__ __forceinline__ uint32_t shl(uint32_t v, int s) { return s > 0 ? (v << s) : s < 0 ? (v >> (-s)) : v; }
    // the two nibble words of low dword u
    static __device__ __forceinline__ void merge(uint32_t l, uint32_t h, int u, uint32_t &E, uint32_t &O)
    {
        E = bfi(0x33333333u, l, shl(h, (u & 1) ? 2 : 0));
        O = bfi(0x33333333u, l >> 2, shl(h, (u & 1) ? 1 : -1));
    }
    static __device__ __forceinline__ u32x4 frag(uint32_t E, uint32_t O, int tp, const Consts &c)
    {
        const uint32_t X = shl(E, tp ? F::SH1 : F::SH0), Y = shl(O, tp ? F::SH1 : F::SH0);
        u32x4 o;
        o[0] = bfi(mask_at(F::P_LO), X, c.b[0]);
        o[1] = bfi(mask_at(F::P_LO), Y, c.b[0]);
        o[2] = bfi(mask_at(F::P_HI), X, c.b[1]);
        o[3] = bfi(mask_at(F::P_HI), Y, c.b[1]);
        return o;
    }
    static __device__ __forceinline__ u32x4 off_frag(const Consts &c) { return u32x4{c.b[0], c.b[0], c.b[1], c.b[1]}; }
};

template <int NW, int KSP, int SPW, int D> struct W3Cfg {
    static constexpr int KS = 256, XB = 16 * KS * 2, NI = 8;           // k per stage, x slab bytes, DMA instructions per slab
    static constexpr int SB1 = XB + NW * 1024;                         // stage: x slab + NW low tiles
    static constexpr int SPS = KSP * SPW, NHP = SPS / 2;               // stages per ring step; high transfers per row tile and ring step
    static constexpr int HOFF = SPS * SB1, SB = HOFF + NW * NHP * 1024;   // ring slot: SPS stages, then [NW][NHP] high units of 1 KiB
    static constexpr int NCW = NW * KSP;                               // compute waves
    static constexpr int NWOPS = SPS * NW + NHP * NW;                  // weight DMA instructions per ring step
    static constexpr size_t LDS = (size_t)D * SB;
    static_assert(SPS % 2 == 0, "a high transfer covers two stages");
    static_assert(SPS * NI * (D - 2) < 64 && NWOPS * (D - 2) < 64 && D >= 2, "vmcnt range");
    static_assert(NCW * 1024 + NCW * 128 <= D * SB && NW <= 8, "exchange area");
    static_assert(LDS <= QA_LDS_MAX, "LDS budget");
};

template <class ACT, int NW, int KSP, int SPW, int D>
__global__ __launch_bounds__(64 * (NW * KSP + 2)) void dq_w3_kernel(K2Args A, uint32_t ntile)
{
    typedef DeqW3<ACT> Q;
    typedef W3Cfg<NW, KSP, SPW, D> C;
    constexpr int KS = C::KS, XB = C::XB, NI = C::NI, SB1 = C::SB1, SPS = C::SPS, NHP = C::NHP, HOFF = C::HOFF, SB = C::SB, NCW = C::NCW;
    extern __shared__ __attribute__((aligned(16))) char smem[];       // [D] slots of {SPS stages {x slab, NW low tiles}, NW x NHP high units}

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t ns = (uint32_t)(A.d / KS), nss = (ns + SPS - 1) / SPS;   // stages (= chunks), ring steps
    const uint32_t rowbytes = (uint32_t)A.d * 2u;
    const uint32_t tile0 = blockIdx.x * NW;                            // first row tile of the workgroup
    const uint32_t hlast = (ns - 1) & ~1u;                             // the last chunk a high transfer starts at (the unpaired one when ns is odd)
    const int64_t b0 = (int64_t)blockIdx.y * 16;                       // first batch row of the workgroup
    const int64_t bsl = A.e.bs - b0 < 16 ? A.e.bs - b0 : 16;

    if (wave == NCW) {
        // ---- weight loader: row tile r is ns * 1536 bytes, chunk PAIR p at 3072 p: two low tiles, then 2 x 512 B of high bits; an unpaired
        // last chunk is its low tile followed by its 512 B of high bits -----------------------------------------------------------------
        const uint32_t rtb = ns * 1536u;
        __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc((void *)A.qw, 0, (int)((uint64_t)ntile * rtb), 0x00020000);
        const uint32_t vl = (uint32_t)lane * 16u;
        const uint32_t vh32 = (uint32_t)(lane & 31) * 16u;              // an unpaired chunk: one 512-byte unit, read twice -- no transfer leaves its row tile
        auto issue_w = [&](uint32_t ss) {
            const uint32_t slot = ss % D;
#pragma unroll
            for (int h = 0; h < SPS; ++h) {
                const uint32_t st = ss * SPS + h, sc = st < ns ? st : ns - 1;
#pragma unroll
                for (int i = 0; i < NW; ++i) {
                    const uint32_t r = tile0 + i, rc = r < ntile ? r : ntile - 1;
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(wrs, (lds_void2_t *)(smem + slot * SB + h * SB1 + XB + i * 1024), 16, vl,
                                                             rc * rtb + (sc >> 1) * 3072u + (sc & 1) * 1024u, 0, 2 /* nt */);
                }
            }
#pragma unroll
            for (int p = 0; p < NHP; ++p) {
                const uint32_t c0 = ss * SPS + 2 * p, cc = c0 < hlast ? c0 : hlast;
                const bool single = cc + 1 >= ns;                      // wave-uniform
                const uint32_t ho = (cc >> 1) * 3072u + (single ? 1024u : 2048u), vh = single ? vh32 : vl;
#pragma unroll
                for (int i = 0; i < NW; ++i) {
                    const uint32_t r = tile0 + i, rc = r < ntile ? r : ntile - 1;
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(wrs, (lds_void2_t *)(smem + slot * SB + HOFF + (i * NHP + p) * 1024), 16, vh,
                                                             rc * rtb + ho, 0, 2 /* nt */);
                }
            }
        };
#pragma unroll
        for (int c = 0; c < D - 1; ++c) issue_w(c);
#pragma unroll 1
        for (uint32_t ss = 0; ss < nss; ++ss) {
            wait_vm<C::NWOPS * (D - 2)>();                             // ring step ss has landed
            __builtin_amdgcn_s_barrier();
            issue_w(ss + D - 1);
        }
        wait_vm<0>();
        __builtin_amdgcn_s_barrier();                                  // "LDS is free"
        __builtin_amdgcn_s_barrier();                                  // the exchange below
        return;
    }
    if (wave == NCW + 1) {
        // ---- x loader: the slab image of dq_s_kernel; rows past the batch tile read zeros (buffer bounds) ------------------------------
        __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc((void *)(A.x + b0 * A.d), 0, (int)(bsl * (int64_t)rowbytes), 0x00020000);
        const uint32_t voff_lo = (lane >> 3) * rowbytes + ((uint32_t)((lane & 7) ^ (lane >> 3)) << 4);
        const uint32_t voff_hi = voff_lo + 8u * rowbytes;
        auto issue_x = [&](uint32_t ss) {
            const uint32_t slot = ss % D;
#pragma unroll
            for (int h = 0; h < SPS; ++h) {
                const uint32_t st = ss * SPS + h, sc = st < ns ? st : ns - 1;
#pragma unroll
                for (int i = 0; i < NI; ++i)                           // DMA instruction i = 2 * column block + row half
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(xrs, (lds_void2_t *)(smem + slot * SB + h * SB1 + i * 1024), 16,
                                                             (i & 1) ? voff_hi : voff_lo, sc * (KS * 2) + (i >> 1) * 128, 0, 0);
            }
        };
#pragma unroll
        for (int c = 0; c < D - 1; ++c) issue_x(c);
#pragma unroll 1
        for (uint32_t ss = 0; ss < nss; ++ss) {
            wait_vm<SPS * NI * (D - 2)>();
            __builtin_amdgcn_s_barrier();
            issue_x(ss + D - 1);
        }
        wait_vm<0>();
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_s_barrier();
        return;
    }

    // ---- compute waves: wave = hh * NW + (row tile in the workgroup); k-part hh takes stages hh * SPW .. of every ring step ----------
    EpiArgs e = A.e;
    e.bs = bsl;
    e.y = (char *)A.e.y + (size_t)b0 * (size_t)e.m * (e.y_f32 ? 4 : 2);
    const int j = lane & 15, g = lane >> 4;
    const int hh = wave / NW, wt = wave - hh * NW;
    const uint32_t rt = tile0 + wt;
    const bool live = rt < ntile;                                      // wave-uniform; a dead wave still meets the barriers
    const uint32_t rd_base = (j >> 3) * 1024 + (j & 7) * 128;
    const uint32_t rd0 = rd_base + (((0 + g) ^ (j & 7)) << 4);
    const uint32_t rd1 = rd_base + (((4 + g) ^ (j & 7)) << 4);
    const uint32_t wof = XB + (uint32_t)wt * 1024 + (uint32_t)lane * 16;
    const uint32_t hof = HOFF + (uint32_t)wt * NHP * 1024 + (uint32_t)lane * 8;

    f32x4_t acc[4], accx[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}, acco[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const u32x4 ones = {opaque(ACT::ONES), opaque(ACT::ONES), opaque(ACT::ONES), opaque(ACT::ONES)};
    const typename Q::Consts qc = Q::make_consts();
    const u32x4 offs = Q::off_frag(qc);
#pragma unroll 1
    for (uint32_t ss = 0; ss < nss; ++ss) {
        __builtin_amdgcn_s_barrier();
#pragma unroll
        for (int u = 0; u < SPW; ++u) {
            const int hs = hh * SPW + u;                               // stage inside the ring step
            const uint32_t st = ss * SPS + hs;
            if (st >= ns) continue;                                    // ragged tail of the ring step (wave-uniform)
            const char *sb = smem + (ss % D) * SB;
            const char *sl = sb + hs * SB1;
            const uint2 hv = *reinterpret_cast<const uint2 *>(sb + hof + (hs >> 1) * 1024 + (hs & 1) * 512);   // our half of the pair's 1 KiB
            const u32x4 ws = *reinterpret_cast<const u32x4 *>(sl + wof);
            u32x4 xf[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) xf[t] = *reinterpret_cast<const u32x4 *>(sl + (t >> 1) * 2048 + ((t & 1) ? rd1 : rd0));
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                uint32_t E, O;
                Q::merge(ws[q], q < 2 ? hv.x : hv.y, q, E, O);
                acc[(2 * q) & 3] = ACT::mfma(Q::frag(E, O, 0, qc), xf[2 * q], acc[(2 * q) & 3]);
                acc[(2 * q + 1) & 3] = ACT::mfma(Q::frag(E, O, 1, qc), xf[2 * q + 1], acc[(2 * q + 1) & 3]);
            }
            // one wave per stage keeps S_1 = sum x and S_off = sum OFF_k x (as dq_s_kernel)
            if (((ss * SPW + u) % NW) == (uint32_t)wt) {
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    accx[t & 1] = ACT::mfma(ones, xf[t], accx[t & 1]);
                    acco[t & 1] = ACT::mfma(offs, xf[t], acco[t & 1]);
                }
            }
        }
    }
    __builtin_amdgcn_s_barrier();                                      // every ring read retired: LDS is free
    const f32x4_t asum = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    float *xch = reinterpret_cast<float *>(smem);                      // [NCW][4][64] k-part partials, then [NCW][16] S_1, [NCW][16] S_off
    float *xsh = xch + NCW * 256, *xso = xsh + NCW * 16;
    if (KSP > 1 && hh > 0) {
        float *p = xch + wave * 256 + lane;
        p[0] = asum[0]; p[64] = asum[1]; p[128] = asum[2]; p[192] = asum[3];
    }
    if (lane < 16) {
        xsh[wave * 16 + lane] = accx[0][0] + accx[1][0];
        xso[wave * 16 + lane] = acco[0][0] + acco[1][0];
    }
    const uint32_t rtc = live ? rt : ntile - 1;
    EpiRow epi = load_epi(e, (int64_t)rtc * 16 + 4 * g);
    __syncthreads();
    if (hh == 0) {
        f32x4_t a = asum;
#pragma unroll
        for (int h = 1; h < KSP; ++h) {
            const float *p = xch + (h * NW + wt) * 256 + lane;
            a[0] += p[0]; a[1] += p[64]; a[2] += p[128]; a[3] += p[192];
        }
        float xsum = 0.f, xoff = 0.f;
#pragma unroll
        for (int v = 0; v < NCW; ++v) {
            xsum += xsh[v * 16 + j];
            xoff += xso[v * 16 + j];
        }
        a[0] -= xoff; a[1] -= xoff; a[2] -= xoff; a[3] -= xoff;
        if (live) epilogue_store(e, epi, 0.f, a, xsum, (int64_t)j, (int64_t)rt * 16 + 4 * g);
    }
}

template <class ACT, int NW, int KSP, int SPW, int D>
int launch_w3(const K2Args &A, hipStream_t s)
{
    constexpr size_t lds = W3Cfg<NW, KSP, SPW, D>::LDS;
    constexpr auto kern = dq_w3_kernel<ACT, NW, KSP, SPW, D>;
    static_assert(lds > QA_LDS_DEFAULT, "every configuration raises the dynamic LDS limit");
    if (int rc = qa_lds<kern>(lds, "dequant_gemm(STREAM3)")) return rc;
    const uint32_t ntile = (uint32_t)(A.e.m / 16);
    kern<<<dim3((ntile + NW - 1) / NW, (unsigned)((A.e.bs + 15) / 16)), 64 * (NW * KSP + 2), lds, s>>>(A, ntile);
    QA_LAUNCH_CHECK("quipamd_dequant_gemm(STREAM3)");
    return QUIPAMD_OK;
}

}   // namespace

// the plan (k2_plan_w3 in k2_plan.h: the cost rule and its measurements) names <NW, KSP, SPW, D>; a group is one launch per problem
int k2w3_run(const K2Plan &p, const K2Shape &c, const K2Problem *pr, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    const bool f16 = c.x_dtype == QUIPAMD_F16;
    for (int gi = 0; gi < p.launches; ++gi) {
        K2Args A;
        k2_fill_args(A, c, pr[gi]);
        int rc;
#define K2_W3_FORM(NW_, KSP_, SPW_, D_)                                                \
        if (p.p[0] == NW_ && p.p[1] == KSP_ && p.p[2] == SPW_ && p.p[3] == D_)         \
            rc = f16 ? launch_w3<ActF16, NW_, KSP_, SPW_, D_>(A, s) : launch_w3<ActBF16, NW_, KSP_, SPW_, D_>(A, s)
        K2_W3_FORM(1, 8, 1, 2);
        else K2_W3_FORM(2, 4, 1, 3);
        else K2_W3_FORM(4, 2, 1, 4);
        else K2_W3_FORM(8, 1, 2, 3);
        else K2_W3_FORM(7, 2, 1, 3);
        else rc = qa_fail(QUIPAMD_ERR_UNSUPPORTED, "dequant_gemm(STREAM3): the plan names no instantiation (%d %d %d %d)", p.p[0], p.p[1], p.p[2], p.p[3]);
#undef K2_W3_FORM
        if (rc != QUIPAMD_OK) return rc;
    }
    return QUIPAMD_OK;
}
