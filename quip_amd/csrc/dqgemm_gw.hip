// dqgemm_gw.hip -- the fused dequant-GEMM on group-wise grids (include/quip_amd_groupwise.h):
//     y[b, r] = bias[r] + sum_g gscale[g, r] * sum_{k in group g} (code[r, k] - gzero[g, r]) * x[b, k]
// STREAM codes (16 rows x KC = 512 / bits columns per 1 KiB tile; 3-bit codes in the 4-bit container), fp32 tables group-major [d / G, m].
//
// One kernel, dq_gw_kernel<CB, ACT, G, BT, NW, KSP, SPW, D>, in the shape of dq_w3_kernel (dqgemm_w3.hip): loader waves own the DMA queue
// and fill a D-deep LDS ring behind counted vmcnt waits, compute waves touch nothing but LDS, one barrier per ring step.  A ring step is
// SPS = KSP * SPW stages of one STREAM chunk (KC columns).  Per stage the ring holds
//     BT x slabs of 16 rows x KC columns (the swizzled image of dqgemm_v2.h, staged by one x-loader wave; rows >= bs read as zeros
//         through the descriptor's bounds check), then per row tile of the workgroup
//     the 1 KiB weight tile, 1 KiB of gscale and 1 KiB of gzero.
// The two tables travel WITH the weights, by the same loader wave, one DMA instruction each: lane L fetches the float4 of rows 4 (L & 3) ..
// of group (L >> 2) % GPS of the stage (GPS = KC / G groups per stage), so the first GPS * 64 bytes of each 1 KiB unit hold the stage's
// groups, 16 rows each, and compute lane (j, g) reads its four rows of group gi as ONE float4 at gi * 64 + g * 16.  The lanes past GPS
// repeat addresses of the first ones (every unit is a full 64-lane transfer; no transfer leaves the tables).
//
// Compute wave (row tile wt of the workgroup, k-part hh): per group, G / 32 MFMA steps into a FRESH accumulator per batch tile with the
// dequantised weights as A (DeqT: value = OFF + code, exact), the same steps against the ONES fragment for S_g[b] = sum_{k in g} x[b, k],
// then the fp32 fold   tot[i] += gscale[i] * (acc[i] - (OFF + gzero[i]) * S_g).   With BT > 1 every dequantised A fragment feeds BT MFMAs.
// K-parts meet once in LDS and are added in index order: no atomics, runs are bit-identical.  MFMA column b is computed from row b of x
// alone and with the same instruction sequence in every column, batch tile and workgroup row, so a row of y does not depend on the
// other rows, on its index or -- within a regime -- on bs.
//
// Two regimes, from bs alone:   bs <= 16: BT = 1, NW = 1, KSP = 4 (the decode stream: K split over four waves)
//                               bs >  16: BT = 4, NW = 4, KSP = 1 (64 batch rows per workgroup, blockIdx.y over batch blocks)
#include "dqgemm_v2.h"
#include "quip_amd_groupwise.h"

namespace {

struct GwArgs {
    const uint16_t *x;
    const u32x4 *qw;
    const float *gscale, *gzero, *bias;
    void *y;
    int y_f32, y_f16;
    int64_t bs, m, d;
};

template <int CB, int G, int BT, int NW, int KSP, int SPW, int D> struct GwCfg {
    static constexpr int KC = 512 / CB, NT = KC / 32, GPS = KC / G, SPG = G / 32;      // columns, MFMA steps, groups per stage; steps per group
    static constexpr int XB1 = 16 * KC * 2, XB = BT * XB1, NI = XB1 / 1024;            // one batch tile's slab, all of them, DMA instructions per slab
    static constexpr int TB = 3 * 1024;                                                 // per row tile: weight tile, gscale unit, gzero unit
    static constexpr int SB1 = XB + NW * TB;                                            // stage
    static constexpr int SPS = KSP * SPW, SB = SPS * SB1, NCW = NW * KSP;               // stages per ring step, ring slot, compute waves
    static constexpr int NWOPS = SPS * NW * 3, NXOPS = SPS * NI * BT;                   // DMA instructions per ring step: weight loader, x loader
    static constexpr int THREADS = 64 * (NCW + 2);
    static constexpr size_t LDS = (size_t)D * SB;
    static_assert(GPS >= 1 && GPS <= 16 && GPS * G == KC, "a stage holds whole groups, at most 16");
    static_assert(D >= 2 && NWOPS * (D - 2) < 64 && NXOPS * (D - 2) < 64, "vmcnt range");
    static_assert((size_t)NCW * BT * 1024 <= LDS, "exchange area");
    static_assert(LDS <= QA_LDS_MAX && THREADS <= 1024, "LDS / workgroup budget");
};

template <int CB, class ACT, int G, int BT, int NW, int KSP, int SPW, int D>
__global__ __launch_bounds__(64 * (NW * KSP + 2)) void dq_gw_kernel(GwArgs A, uint32_t ntile)
{
    typedef DeqT<CB, ACT> Q;
    typedef GwCfg<CB, G, BT, NW, KSP, SPW, D> C;
    constexpr int KC = C::KC, NT = C::NT, GPS = C::GPS, SPG = C::SPG, XB1 = C::XB1, XB = C::XB, NI = C::NI, TB = C::TB, SB1 = C::SB1, SPS = C::SPS,
                  SB = C::SB, NCW = C::NCW;
    constexpr int SPD = CB == 2 ? 2 : 1, US = SPG > 2 ? SPG : 2, NU = NT / US, DPU = US / SPD, GPU = US / SPG;   // steps per dword; per unit: steps, dwords, groups
    static_assert(NU * US == NT && DPU >= 1 && DPU <= 4 && GPU * SPG == US && NU * GPU == GPS, "the units cover the stage");
    extern __shared__ __attribute__((aligned(16))) char smem[];       // [D] slots of SPS stages {BT x slabs, NW x {weights, gscale, gzero}}

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t ns = (uint32_t)(A.d / KC), nss = (ns + SPS - 1) / SPS;   // stages (= chunks), ring steps
    const uint32_t rowbytes = (uint32_t)A.d * 2u;
    const uint32_t tile0 = blockIdx.x * NW;                            // first row tile of the workgroup
    const int64_t b0 = (int64_t)blockIdx.y * (16 * BT);                // first batch row of the workgroup

    if (wave == NCW) {
        // ---- weight loader: tile (rt, chunk) at (rt * ns + chunk) KiB; the groups of a chunk are rows chunk * GPS .. of the two tables ------
        const uint32_t tabbytes = (uint32_t)((A.d / G) * A.m * 4);
        __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc((void *)A.qw, 0, (int)((uint64_t)ntile * ns * 1024u), 0x00020000);
        __amdgpu_buffer_rsrc_t srs = __builtin_amdgcn_make_buffer_rsrc((void *)A.gscale, 0, (int)tabbytes, 0x00020000);
        __amdgpu_buffer_rsrc_t zrs = __builtin_amdgcn_make_buffer_rsrc((void *)A.gzero, 0, (int)tabbytes, 0x00020000);
        const uint32_t vl = (uint32_t)lane * 16u;
        const uint32_t vp = (uint32_t)((lane >> 2) % GPS) * (uint32_t)A.m * 4u + (uint32_t)(lane & 3) * 16u;
        auto issue_w = [&](uint32_t ss) {
            const uint32_t slot = ss % D;
#pragma unroll
            for (int h = 0; h < SPS; ++h) {
                const uint32_t st = ss * SPS + h, sc = st < ns ? st : ns - 1;
#pragma unroll
                for (int i = 0; i < NW; ++i) {
                    const uint32_t r = tile0 + i, rc = r < ntile ? r : ntile - 1;
                    char *dst = smem + slot * SB + h * SB1 + XB + i * TB;
                    const uint32_t po = (sc * GPS * (uint32_t)A.m + rc * 16u) * 4u;
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(wrs, (lds_void2_t *)dst, 16, vl, (rc * ns + sc) * 1024u, 0, 2 /* nt */);
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(srs, (lds_void2_t *)(dst + 1024), 16, vp, po, 0, 0);
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(zrs, (lds_void2_t *)(dst + 2048), 16, vp, po, 0, 0);
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
        // ---- x loader: per batch tile the slab image of dq_s_kernel; rows past bs read zeros (buffer bounds; an empty tile has 0 records) ---
        auto tile_rsrc = [&](int bt) {
            const int64_t left = A.bs - (b0 + 16 * bt);
            const int64_t bsl = left < 0 ? 0 : left < 16 ? left : 16;
            const uint16_t *xb = bsl > 0 ? A.x + (b0 + 16 * bt) * A.d : A.x;
            return __builtin_amdgcn_make_buffer_rsrc((void *)xb, 0, (int)(bsl * (int64_t)rowbytes), 0x00020000);
        };
        const uint32_t voff_lo = (lane >> 3) * rowbytes + ((uint32_t)((lane & 7) ^ (lane >> 3)) << 4);
        const uint32_t voff_hi = voff_lo + 8u * rowbytes;
        auto issue_x = [&](uint32_t ss) {
            const uint32_t slot = ss % D;
#pragma unroll
            for (int h = 0; h < SPS; ++h) {
                const uint32_t st = ss * SPS + h, sc = st < ns ? st : ns - 1;
#pragma unroll
                for (int bt = 0; bt < BT; ++bt) {
                    __amdgpu_buffer_rsrc_t xrs = tile_rsrc(bt);
#pragma unroll
                    for (int i = 0; i < NI; ++i)                       // DMA instruction i = 2 * column block + row half
                        __builtin_amdgcn_raw_ptr_buffer_load_lds(xrs, (lds_void2_t *)(smem + slot * SB + h * SB1 + bt * XB1 + i * 1024), 16,
                                                                 (i & 1) ? voff_hi : voff_lo, sc * (KC * 2) + (i >> 1) * 128, 0, 0);
                }
            }
        };
#pragma unroll
        for (int c = 0; c < D - 1; ++c) issue_x(c);
#pragma unroll 1
        for (uint32_t ss = 0; ss < nss; ++ss) {
            wait_vm<C::NXOPS * (D - 2)>();
            __builtin_amdgcn_s_barrier();
            issue_x(ss + D - 1);
        }
        wait_vm<0>();
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_s_barrier();
        return;
    }

    // ---- compute waves: wave = hh * NW + (row tile in the workgroup); k-part hh takes stages hh * SPW .. of every ring step ----------
    const int j = lane & 15, g = lane >> 4;
    const int hh = wave / NW, wt = wave - hh * NW;
    const uint32_t rt = tile0 + wt;
    const bool live = rt < ntile;                                      // wave-uniform; a dead wave still meets the barriers
    // lane parts of the LDS addresses, hidden from the optimiser: it would otherwise merge them into the constant parts with v_or (the bits are
    // disjoint) and keep one address register per read instead of one base and immediate offsets
    const uint32_t rd_base = (j >> 3) * 1024 + (j & 7) * 128;
    const uint32_t rd0 = opaque(rd_base + (((0 + g) ^ (j & 7)) << 4));
    const uint32_t rd1 = opaque(rd_base + (((4 + g) ^ (j & 7)) << 4));
    const uint32_t wl = opaque((uint32_t)lane * 16), pl = opaque((uint32_t)g * 16);
    constexpr uint32_t wof = XB, pof = XB + 1024;
    const uint32_t tof = (uint32_t)wt * TB;

    f32x4_t tot[BT];
#pragma unroll
    for (int b = 0; b < BT; ++b) tot[b] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const u32x4 ones = {opaque(ACT::ONES), opaque(ACT::ONES), opaque(ACT::ONES), opaque(ACT::ONES)};
#pragma unroll 1
    for (uint32_t ss = 0; ss < nss; ++ss) {
        __builtin_amdgcn_s_barrier();
#pragma unroll
        for (int u = 0; u < SPW; ++u) {
            const int hs = hh * SPW + u;                               // stage inside the ring step
            const uint32_t st = ss * SPS + hs;
            if (st >= ns) continue;                                    // ragged tail of the ring step (wave-uniform)
            const char *sl = smem + (ss % D) * SB + hs * SB1;
            const u32x4 ws = *reinterpret_cast<const u32x4 *>(sl + tof + wl + wof);
            // a unit = US steps = whole dwords of the lane's four and whole groups.  BT > 1 walks the units in a ROLLED loop (the dwords picked at
            // run time): fully unrolled, the scheduler issues every group's MFMAs ahead of the folds and runs out of registers.  BT == 1 unrolls
            // and the picks fold away.
            auto unit = [&](int un) {
                uint32_t w[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int q = un * DPU + k;
                    w[k] = k >= DPU ? 0u : q == 0 ? ws[0] : q == 1 ? ws[1] : q == 2 ? ws[2] : ws[3];
                }
                const char *xu = sl + un * ((US / 2) * 2048);
                const char *pu = sl + tof + pl + un * (GPU * 64);
#pragma unroll
                for (int gl = 0; gl < GPU; ++gl) {
                    const float4 sc = *reinterpret_cast<const float4 *>(pu + (pof + gl * 64));
                    const float4 zr = *reinterpret_cast<const float4 *>(pu + (pof + 1024 + gl * 64));
                    f32x4_t acc[BT], sx[BT];
#pragma unroll
                    for (int b = 0; b < BT; ++b) acc[b] = sx[b] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int s = 0; s < SPG; ++s) {
                        const int t = gl * SPG + s;                    // step inside the unit
                        const u32x4 a = Q::frag4(w[0], w[1], w[2], w[3], t);
#pragma unroll
                        for (int b = 0; b < BT; ++b) {
                            const u32x4 xf = *reinterpret_cast<const u32x4 *>(xu + ((t & 1) ? rd1 : rd0) + (b * XB1 + (t >> 1) * 2048));
                            acc[b] = ACT::mfma(a, xf, acc[b]);
                            sx[b] = ACT::mfma(ones, xf, sx[b]);
                        }
                    }
                    const float s4[4] = {sc.x, sc.y, sc.z, sc.w};
                    const float z4[4] = {Q::OFF + zr.x, Q::OFF + zr.y, Q::OFF + zr.z, Q::OFF + zr.w};
#pragma unroll
                    for (int b = 0; b < BT; ++b)
#pragma unroll
                        for (int i = 0; i < 4; ++i) tot[b][i] += s4[i] * (acc[b][i] - z4[i] * sx[b][i]);
                }
            };
            if constexpr (BT > 1) {
#pragma unroll 1
                for (int un = 0; un < NU; ++un) unit(un);
            } else {
#pragma unroll
                for (int un = 0; un < NU; ++un) unit(un);
            }
        }
    }
    __builtin_amdgcn_s_barrier();                                      // every ring read retired: LDS is free
    float *xch = reinterpret_cast<float *>(smem);                      // [NCW][BT][4][64] k-part partials
    if (KSP > 1 && hh > 0) {
#pragma unroll
        for (int b = 0; b < BT; ++b) {
            float *p = xch + (wave * BT + b) * 256 + lane;
            p[0] = tot[b][0]; p[64] = tot[b][1]; p[128] = tot[b][2]; p[192] = tot[b][3];
        }
    }
    const uint32_t rtc = live ? rt : ntile - 1;
    const int64_t r0 = (int64_t)rtc * 16 + 4 * g;
    const float4 bi = A.bias ? *reinterpret_cast<const float4 *>(A.bias + r0) : make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();
    if (hh == 0 && live) {
#pragma unroll
        for (int b = 0; b < BT; ++b) {
            f32x4_t a = tot[b];
#pragma unroll
            for (int h = 1; h < KSP; ++h) {
                const float *p = xch + ((h * NW + wt) * BT + b) * 256 + lane;
                a[0] += p[0]; a[1] += p[64]; a[2] += p[128]; a[3] += p[192];
            }
            const int64_t row = b0 + 16 * b + j;
            if (row >= A.bs) continue;
            const float o0 = a[0] + bi.x, o1 = a[1] + bi.y, o2 = a[2] + bi.z, o3 = a[3] + bi.w;
            if (A.y_f32) {
                *reinterpret_cast<float4 *>((float *)A.y + row * A.m + r0) = make_float4(o0, o1, o2, o3);
            } else {
                uint2 pk;
                if (A.y_f16) {
                    pk.x = (uint32_t)f32_to_f16_bits(o0) | ((uint32_t)f32_to_f16_bits(o1) << 16);
                    pk.y = (uint32_t)f32_to_f16_bits(o2) | ((uint32_t)f32_to_f16_bits(o3) << 16);
                } else {
                    pk.x = (uint32_t)f32_to_bf16_bits(o0) | ((uint32_t)f32_to_bf16_bits(o1) << 16);
                    pk.y = (uint32_t)f32_to_bf16_bits(o2) | ((uint32_t)f32_to_bf16_bits(o3) << 16);
                }
                *reinterpret_cast<uint2 *>((uint16_t *)A.y + row * A.m + r0) = pk;
            }
        }
    }
}

template <int CB, class ACT, int G, int BT, int NW, int KSP, int SPW, int D>
int launch_gw(const GwArgs &A, hipStream_t s)
{
    typedef GwCfg<CB, G, BT, NW, KSP, SPW, D> C;
    constexpr auto kern = dq_gw_kernel<CB, ACT, G, BT, NW, KSP, SPW, D>;
    if (int rc = qa_lds<kern>(C::LDS, "dequant_gemm_groupwise")) return rc;
    const uint32_t ntile = (uint32_t)(A.m / 16);
    kern<<<dim3((ntile + NW - 1) / NW, (unsigned)((A.bs + 16 * BT - 1) / (16 * BT))), C::THREADS, C::LDS, s>>>(A, ntile);
    QA_LAUNCH_CHECK("quipamd_dequant_gemm_groupwise");
    return QUIPAMD_OK;
}

// the regime is a rule of bs alone; the forms inside a regime are fixed
template <int CB, class ACT, int G> int run_gw(const GwArgs &A, hipStream_t s)
{
    if (A.bs <= 16) return launch_gw<CB, ACT, G, 1, 1, 4, 1, 3>(A, s);
    return launch_gw<CB, ACT, G, 4, 4, 1, 1, 3>(A, s);
}

template <int CB, class ACT> int run_gw_g(int G, const GwArgs &A, hipStream_t s)
{
    return G == 32 ? run_gw<CB, ACT, 32>(A, s) : G == 64 ? run_gw<CB, ACT, 64>(A, s) : run_gw<CB, ACT, 128>(A, s);
}

inline bool al16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}   // namespace

extern "C" int quipamd_dequant_gemm_groupwise(const void *x, int x_dtype, const int32_t *qweight, int bits, int groupsize, const float *gscale,
                                              const float *gzero, const float *bias, void *y, int y_dtype, int64_t bs, int64_t m, int64_t d,
                                              void *stream)
{
    QA_REQUIRE(x && qweight && gscale && gzero && y, QUIPAMD_ERR_ARG, "dequant_gemm_groupwise: null pointer");
    QA_REQUIRE(bits == 2 || bits == 3 || bits == 4, QUIPAMD_ERR_ARG, "dequant_gemm_groupwise: bits %d (2, 3 or 4)", bits);
    QA_REQUIRE(groupsize == 32 || groupsize == 64 || groupsize == 128, QUIPAMD_ERR_UNSUPPORTED,
               "dequant_gemm_groupwise: groupsize %d (32, 64 or 128)", groupsize);
    QA_REQUIRE(x_dtype == QUIPAMD_F16 || x_dtype == QUIPAMD_BF16, QUIPAMD_ERR_UNSUPPORTED, "dequant_gemm_groupwise: x is f16 / bf16 only (dtype %d)",
               x_dtype);
    QA_REQUIRE(y_dtype == QUIPAMD_F32 || y_dtype == QUIPAMD_F16 || y_dtype == QUIPAMD_BF16, QUIPAMD_ERR_ARG, "dequant_gemm_groupwise: bad y dtype %d",
               y_dtype);
    QA_REQUIRE(bs >= 1, QUIPAMD_ERR_SHAPE, "dequant_gemm_groupwise: at least one row (bs %lld)", (long long)bs);
    const int cb = bits == 2 ? 2 : 4, kc = 512 / cb;
    QA_REQUIRE(m >= 16 && m % 16 == 0, QUIPAMD_ERR_SHAPE, "dequant_gemm_groupwise: m %lld is not a multiple of 16", (long long)m);
    QA_REQUIRE(d >= kc && d % kc == 0, QUIPAMD_ERR_SHAPE, "dequant_gemm_groupwise: d %lld is not a multiple of %d (512 / bits)", (long long)d, kc);
    // 32-bit byte offsets inside the kernel: the code words, a table and 16 rows of x each stay below 2 GiB
    QA_REQUIRE(m * d * cb / 8 < (1ll << 31) && (d / groupsize) * m * 4 < (1ll << 31) && d * 32 < (1ll << 31) && (bs + 63) / 64 <= 65535,
               QUIPAMD_ERR_SHAPE, "dequant_gemm_groupwise: %lld x %lld x %lld is beyond the kernel's 32-bit offsets", (long long)bs, (long long)m,
               (long long)d);
    QA_REQUIRE(al16(x) && al16(qweight) && al16(gscale) && al16(gzero) && al16(bias) && al16(y), QUIPAMD_ERR_ARG,
               "dequant_gemm_groupwise: every pointer must be 16-byte aligned");
    GwArgs A{(const uint16_t *)x, (const u32x4 *)qweight, gscale, gzero, bias, y, y_dtype == QUIPAMD_F32, y_dtype == QUIPAMD_F16, bs, m, d};
    hipStream_t s = (hipStream_t)stream;
    if (cb == 2) return x_dtype == QUIPAMD_F16 ? run_gw_g<2, ActF16>(groupsize, A, s) : run_gw_g<2, ActBF16>(groupsize, A, s);
    return x_dtype == QUIPAMD_F16 ? run_gw_g<4, ActF16>(groupsize, A, s) : run_gw_g<4, ActBF16>(groupsize, A, s);
}
