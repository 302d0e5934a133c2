// k2_plan.h -- which kernel serves a fused dequant-GEMM call (quipamd_dequant_gemm, _cfg, _grouped), as plain C++.
//
// k2_plan() is a total function of (shape, overrides): it returns the kernel, the template parameters of its instantiation, the k-slices and
// the number of launches -- or the status and message of the refusal.  It includes no HIP header, reads no global and no environment, and
// sees no pointer, so quipamd_dequant_gemm_plan can answer "what would this call run" on a machine without a GPU.  The launch code
// (k2r1_run in dqgemm.hip, k2v2_run in dqgemm_v2.hip, k2w3_run in dqgemm_w3.hip) executes a plan and decides nothing.
// Not part of a plan: the limits a launch_* template checks on its own grid (packed weights >= 4 GiB in the streaming kernels, more batch
// tiles than grid.y holds) and the pointer checks of the call.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include "quip_amd.h"

// ---- the override values that callers pass as numbers (include/quip_amd.h documents them; tests and bench.py pass them) --------------------
enum { K2_FAM_AUTO = 0, K2_FAM_OLD = 1, K2_FAM_H = 2, K2_FAM_S = 3, K2_FAM_MB = 4, K2_FAM_PF = 5, K2_FAM_NONE = 99 };
enum { K2_H_REGISTER_X = 44 };           // family h, p1: dq_hr_kernel (x straight into registers) instead of 4 waves of the LDS-DMA form
enum {                                   // family mb, p1: workgroup tile (rows x batch rows) and loader waves
    K2_MB_128x64_L2 = 22, K2_MB_128x64_L4 = 23, K2_MB_256x128_L2 = 44, K2_MB_256x128_L4 = 45,
    K2_MB_256x128_L3 = 46, K2_MB_256x128_T32 = 47, K2_MB_WIDE_L2 = 48, K2_MB_WIDE_L4 = 49       // 46..49: round-5 lab forms, 2 bit, forced only
};
enum { K2_SG_7x2 = 72, K2_SG_4x2 = 74, K2_SG_8x1 = 81 };   // quipamd_dequant_gemm_grouped_config: dq_sg_kernel <7,2,1,3> / <4,2,1,4> / <8,1,2,3>
// which grouped weight-stream form serves the big grouped GEMMs of a 5..16-row step by default (0: none, the grouped h kernel).
// profiles/r06b_grouped_forms.jsonl (Llama-2-7B, one box, alternating, ms per step at 16 / 8 sequences): grouped h kernel with 4 row tiles
// 3.21 / 2.78; dq_sg <4,2,1,4> 3.14 / 2.78; <7,2,1,3> 3.00 / 2.63; <8,1,2,3> 3.08 / 2.70.
enum { K2_SG_DEFAULT = K2_SG_7x2 };

struct K2Shape {
    int x_dtype;              // QUIPAMD_BF16 | QUIPAMD_F16
    int bits, cbits;          // code bits as passed; container bits (3-bit codes ride in the 4-bit container of the STREAM layout)
    int layout, y_dtype, accumulate, qfn, ngroups;
    int64_t bs, m, d;
};

inline K2Shape k2_shape(int ngroups, int x_dtype, int bits, int layout, int qfn, int y_dtype, int accumulate, int64_t bs, int64_t m, int64_t d)
{
    return K2Shape{x_dtype, bits, (bits == 3 && layout == QUIPAMD_LAYOUT_STREAM) ? 4 : bits, layout, y_dtype, accumulate, qfn, ngroups, bs, m, d};
}

// The three override sources.  All 0 = the shape heuristic.
struct K2Cfg {                // the cfg argument of quipamd_dequant_gemm_cfg: per call
    int family, p1, p2, rt;
};
struct K2Tune {               // quipamd_tune_dequant_gemm: per calling thread, round-1 kernels
    int rt, bt, nw, ksplit;   // row tiles per workgroup, batch tiles per wave, waves (tile kernel: chunks in flight = nw / rt), k-slices
    int depth;                // chunk groups in flight per workgroup of the tile kernel
    bool force_batched;       // depth 9: the batched kernel with `rt` row tiles per wave (it has no depth, so the value doubles as the switch;
                              // the tile kernel refuses it like any depth it has no instantiation for)
    bool any() const { return rt || bt || nw || ksplit || depth; }
};
struct K2Force {
    K2Cfg cfg;
    K2Tune tune;
    int grouped_form;         // quipamd_dequant_gemm_grouped_config: process-wide
};

// the one place that sees the packed argument of quipamd_tune_dequant_gemm: split + 100 * depth
inline K2Tune k2_tune_decode(int rt, int bt, int nw, int split)
{
    return K2Tune{rt, bt, nw, split % 100, split / 100, split / 100 == 9};
}

struct K2Plan {
    int status;               // QUIPAMD_OK, or the refusal (msg)
    bool args_ok;             // the arguments passed validation: a refusal is then the kernel choice's, made behind the call's pointer checks
    int kernel;               // QUIPAMD_K2_*; the meaning of p[] per kernel is documented with the enum (include/quip_amd.h)
    int p[5];
    int kslices;              // k-slices over workgroups (fp32 atomics into y): > 1 only in the round-1 tile kernel under the accumulate contract
    int launches;             // 1: the whole call is one launch; ngroups: one launch per problem of a group; 0: nothing to do
    char msg[224];
};

inline K2Plan k2_take(int kernel, int launches, int p0 = 0, int p1 = 0, int p2 = 0, int p3 = 0, int p4 = 0, int kslices = 1)
{
    K2Plan r{};
    r.status = QUIPAMD_OK; r.args_ok = true; r.kernel = kernel; r.kslices = kslices; r.launches = launches;
    r.p[0] = p0; r.p[1] = p1; r.p[2] = p2; r.p[3] = p3; r.p[4] = p4;
    return r;
}

#if defined(__GNUC__)
__attribute__((format(printf, 3, 4)))
#endif
inline K2Plan k2_refuse(int status, bool args_ok, const char *fmt, ...)
{
    K2Plan r{};
    r.status = status; r.args_ok = args_ok; r.kernel = QUIPAMD_K2_NONE;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(r.msg, sizeof r.msg, fmt, ap);
    va_end(ap);
    return r;
}
#define K2_REQUIRE(cond, code, args_ok, ...) \
    do {                                     \
        if (!(cond)) return k2_refuse((code), (args_ok), __VA_ARGS__); \
    } while (0)

// ---- the STREAM3 layout (dqgemm_w3.hip): one kernel family, one launch per problem --------------------------------------------------------
// Row tiles per workgroup (NW; K is split over 8 / NW waves per tile): cost = rounds of 256 one-per-CU workgroups x NW, ties to the larger NW
// (x is ingested once per workgroup).  Measured at bs 16, us, with each shape forced in a lab build (profiles/w3_native_vs_container.jsonl
// has the chosen ones): 8192 x 8192 NW 1 / 2 / 4 15.1 / 10.5 / 14.8; 7168 x 28672 39.1 / 28.0 / 40.6; 28672 x 7168 NW 4 / 7 / 8 27.1 / 20.3 /
// 21.7; 4096 x 4096 NW 1 / 2 5.9 / 6.8.  Only those five shapes were timed: the rule is what they agree on, row counts between them
// (5120, 13824, 16384, 32000 ...) are served by it unmeasured.  Every configuration is checked against fp64 in tests/test_gpu_stream3.py.
inline K2Plan k2_plan_w3(const K2Shape &c, const K2Cfg &cfg)
{
    K2_REQUIRE(c.bits == 3, QUIPAMD_ERR_UNSUPPORTED, false, "dequant_gemm: the STREAM3 layout holds 3-bit codes only (bits=%d)", c.bits);
    K2_REQUIRE(c.qfn == QUIPAMD_QFN_B || c.qfn == QUIPAMD_QFN_A, QUIPAMD_ERR_ARG, false, "dequant_gemm: qfn must be a or b");
    K2_REQUIRE(cfg.family == 0 && cfg.p1 == 0 && cfg.p2 == 0 && cfg.rt == 0, QUIPAMD_ERR_UNSUPPORTED, false,
               "dequant_gemm: no forced kernel configurations for the STREAM3 layout");
    K2_REQUIRE(c.m % 16 == 0 && c.d % 256 == 0 && c.d > 0, QUIPAMD_ERR_SHAPE, false,
               "dequant_gemm: STREAM3 layout needs m %% 16 == 0 and d %% 256 == 0 (m=%lld d=%lld)", (long long)c.m, (long long)c.d);
    K2_REQUIRE(c.d * 32 < ((int64_t)1 << 31) && c.m * c.d * 3 / 8 < ((int64_t)1 << 32), QUIPAMD_ERR_SHAPE, false,
               "dequant_gemm(STREAM3): 32-bit buffer offsets: packed weights >= 4 GiB or a 16-row slab of x >= 2 GiB (m=%lld d=%lld)",
               (long long)c.m, (long long)c.d);
    K2_REQUIRE((c.bs + 15) / 16 <= 65535, QUIPAMD_ERR_SHAPE, false, "dequant_gemm(STREAM3): bs too large (%lld)", (long long)c.bs);
    const int64_t ntile = c.m / 16;
    int nw = 1;
    int64_t best = -1;
    static const int nws[] = {1, 2, 4, 7, 8};
    for (int n : nws) {
        const int64_t cost = (((ntile + n - 1) / n + 255) / 256) * n;
        if (best < 0 || cost <= best) { best = cost; nw = n; }
    }
    // <NW, KSP, SPW, D>: K over KSP waves per tile, SPW stages per wave and ring step, a D-deep LDS ring
    if (nw == 1) return k2_take(QUIPAMD_K2_W3, c.ngroups, 1, 8, 1, 2);
    if (nw == 2) return k2_take(QUIPAMD_K2_W3, c.ngroups, 2, 4, 1, 3);
    if (nw == 4) return k2_take(QUIPAMD_K2_W3, c.ngroups, 4, 2, 1, 4);
    if (nw == 8) return k2_take(QUIPAMD_K2_W3, c.ngroups, 8, 1, 2, 3);
    return k2_take(QUIPAMD_K2_W3, c.ngroups, 7, 2, 1, 3);
}

// ---- the second-generation kernels (dqgemm_v2.h), one problem -------------------------------------------------------------------------------
// They come first; `false` = declined, the shape is better served by the round-1 kernels (bf16 only).  fp16 activations (quant.py:226-229
// widens x, it never narrows it: an fp16 model keeps all its activation bits on the fp16 MFMA pipe) exist only here, so every fp16 shape is
// taken.  `launches`: what the plan reports (1, or ngroups when a group falls back to one launch per problem).
inline bool k2_plan_v2(const K2Shape &c, const K2Cfg &cfg, int launches, K2Plan &out)
{
    const int BITS = c.cbits;
    const int64_t m = c.m, d = c.d, bs = c.bs;
    const int64_t ntile = m / 16, nkc = d / (512 / BITS);
    const bool f16 = c.x_dtype == QUIPAMD_F16;
    int fam = cfg.family, p1 = cfg.p1, p2 = cfg.p2;
    if (fam == K2_FAM_OLD) return false;
    // (family 5, the round-3 prefill kernel -- every 2-bit tile dequantised once per workgroup into LDS, 32x32x16 mainloop -- measured SLOWER
    //  than the mb kernel at every prefill shape, profiles/r03t_k2_prefill.jsonl, and left the library in round 4: scripts/dqgemm_pf_lab.hip)
    if (fam == K2_FAM_PF) {
        out = k2_refuse(QUIPAMD_ERR_UNSUPPORTED, true, "dequant_gemm: kernel family 5 (prefill lab) is not part of the library");
        return true;
    }
    const bool h_fits = bs <= 16 && nkc <= (BITS == 2 ? 16 : 32);
    const bool mb_ok = d % 256 == 0;
    auto take = [&](int kernel, int a = 0, int b = 0, int c2 = 0, int d2 = 0, int e = 0) { out = k2_take(kernel, launches, a, b, c2, d2, e); return true; };
    if (fam == K2_FAM_AUTO) {
        // measured on MI355X, profiles/r02*_k2lab.log (cold weights):
        //   h: every shape whose K fits one pass of LDS (d <= 4096) and whose grid is not many rounds of 1-per-CU workgroups
        //   s: tall layers (>= 1024 row tiles), where a weight stream pays; below that the round-1 kernels, which split K
        //      over 16 waves, are faster
        //   mb: bs > 16 when there are >= ~200 workgroup tiles of 256 x 128
        if (bs <= 16) {
            // round 6: 16 < chunks <= 32 (d <= 8192) at bs <= 8 -- the one-pass kernel with 8-row slabs (dq_h_body.inc HALF: 4 KiB per chunk):
            // OPT's fc2 (2048 x 8192) in a blocked-operator decode step, which the round-1 tile kernel served in 6.6 us
            if (BITS == 2) {
                if (bs <= 8 && nkc > 16 && nkc <= 32 && ntile <= 512) return take(QUIPAMD_K2_H_HALF, 1, 8, 4);
                // 9..16 rows: the same kernel as a GROUPED launch of two problems that share the weights -- rows 0..7 and rows 8.. of x and y
                // (blockIdx.y): every weight tile is streamed twice, but 2 x ntile workgroups fit one round up to 128 row tiles, where the
                // weight-stream family (1 tile x 8 k-parts per workgroup) took 7.1 us for OPT's fc2 at 16 rows
                if (bs > 8 && nkc > 16 && nkc <= 32 && ntile <= 128 && !c.accumulate) return take(QUIPAMD_K2_H_HALF_X2, 1, 8, 4);
            }
            if (h_fits && ntile <= 768) fam = K2_FAM_H;
            else if (ntile >= 1024 && d % 256 == 0) fam = K2_FAM_S;
            else if (f16) fam = h_fits ? K2_FAM_H : (d % 256 == 0) ? K2_FAM_S : K2_FAM_NONE;   // fp16 exists only here: any shape a kernel can hold
            else return false;
        } else {
            const int64_t tiles = ((m + 255) / 256) * ((bs + 127) / 128);
            if (mb_ok && ((tiles >= 200 && BITS == 2) || f16)) fam = K2_FAM_MB;   // 4 bit: the big tile does not fit LDS, round 1 wins
            else if (f16) fam = K2_FAM_NONE;
            else return false;
        }
    }
    auto refuse = [&](const K2Plan &r) { out = r; return true; };
    if (fam == K2_FAM_H) {
        if (!h_fits) return refuse(k2_refuse(QUIPAMD_ERR_UNSUPPORTED, true, "dequant_gemm: kernel family h needs bs <= 16 and d <= %d", 4096));
        // p = <RT, NW, NCH>: row tiles per workgroup, waves, chunks per wave (HALF / EXACT follow from bs <= 8 and d == NW * NCH chunks: launch_h)
        if (BITS == 2) {
            // d = 4096 (16 chunks): 4 waves x 4 adjacent chunks since round 5 -- 4.33-4.42 us cold against 4.64-4.69 for 8 x 2 with the same
            // chunk order (profiles/r05h_k2lab_hl.txt; with rounds 2-4's interleaved chunks 8 x 2 was the faster one); d <= 2048: 8 x 1
            if (p1 == 0) { p1 = nkc <= 8 ? 8 : 4; p2 = nkc <= 8 ? 1 : 4; }
            // row tiles per workgroup (cfg rt; 0 = by the grid): more than one round of 256 one-per-CU workgroups pays the ingest of x once
            // per round -- 11008 x 4096: 10.5 us at 1 tile, 10.0 at 2, 8.2 at 4; 8192 x 2048: 4.70 / 4.39; at 256 tiles (the headline)
            // 1 tile stays the fastest: 4.37 against 5.44 / 7.63 (profiles/r05p_k2lab_rt.txt)
            int rt = cfg.rt;
            if (rt == 0) rt = (ntile > 512 && ntile % 4 == 0 && nkc > 8) ? 4 : (ntile > 256 && ntile % 2 == 0) ? 2 : 1;
            if (rt == 2 && ntile % 2 == 0) {
                if (p1 == 8 && p2 == 1 && nkc <= 8) return take(QUIPAMD_K2_H, 2, 8, 1);
                if (p1 == 4 && p2 == 4) return take(QUIPAMD_K2_H, 2, 4, 4);
            }
            if (rt == 4 && ntile % 4 == 0 && p1 == 4 && p2 == 4) return take(QUIPAMD_K2_H, 4, 4, 4);
            // round 6: x straight into registers (dq_hr_kernel), exact fit d = 4096 only.  p1 = 44 forces it, p1 = 4 keeps the LDS-DMA form
            if (p1 == K2_H_REGISTER_X && p2 == 4) {
                if (nkc != 16)
                    return refuse(k2_refuse(QUIPAMD_ERR_UNSUPPORTED, true, "dequant_gemm: the register-x form holds d = 4096 only (d=%lld)", (long long)d));
                return take(QUIPAMD_K2_HR, 1, 4, 4);
            }
            if (p1 == 8 && p2 == 1 && nkc <= 8) return take(QUIPAMD_K2_H, 1, 8, 1);
            if (p1 == 8 && p2 == 2) return take(QUIPAMD_K2_H, 1, 8, 2);
            if (p1 == 16 && p2 == 1 && nkc <= 16) return take(QUIPAMD_K2_H, 1, 16, 1);
            if (p1 == 4 && p2 == 4) return take(QUIPAMD_K2_H, 1, 4, 4);
        } else {
            if (p1 == 0) { p1 = 8; p2 = nkc <= 16 ? 2 : 4; }
            if (p1 == 8 && p2 == 2 && nkc <= 16) return take(QUIPAMD_K2_H, 1, 8, 2);
            if (p1 == 8 && p2 == 4) return take(QUIPAMD_K2_H, 1, 8, 4);
        }
        return refuse(k2_refuse(QUIPAMD_ERR_UNSUPPORTED, true, "dequant_gemm: no h kernel for nw=%d nch=%d (d=%lld)", p1, p2, (long long)d));
    }
    if (fam == K2_FAM_S) {
        if (!(bs <= 16 && d % 256 == 0))
            return refuse(k2_refuse(QUIPAMD_ERR_UNSUPPORTED, true, "dequant_gemm: kernel family s needs bs <= 16 and d %% 256 == 0"));
        if (p1 == 0) {
            // one workgroup per CU and whole rounds: 7 row tiles per workgroup fit 1792 tiles (28672 rows) exactly, 8 fit 2048
            // (32768 rows: 18.0 us with 8 x 256 workgroups, 27 us with 293 workgroups of 7 -- profiles/r02l_k2lab_s.log)
            // and 4 fit 1024 (16384 rows: 13.1 us with 256 workgroups of 4, 15.0 with 147 of 7 -- profiles/r04q_k2_s_cfgs.jsonl).  Cost = rounds of
            // 256 workgroups x tiles per workgroup; ties go to the larger workgroup (32768 rows: 8 x 256 18.8 us, 4 x 512 25.5)
            const int64_t r4 = ((ntile + 3) / 4 + 255) / 256, r7 = ((ntile + 6) / 7 + 255) / 256, r8 = ((ntile + 7) / 8 + 255) / 256;
            // short and wide (reached with fp16 activations only: a 5..16-row decode step's fc2 / down_proj GEMM): fill the CUs first --
            // 2048 x 8192: 12.1 us with 4 tiles per workgroup (32 workgroups), 7.8 with 2, 7.1 with 1; 4096 x 11008: 15.5 / 9.9 / 9.95
            // (profiles/r05d_k2_s_shortwide.jsonl)
            if (ntile <= 128) { p1 = 1; p2 = 8; }
            else if (ntile <= 256) { p1 = 2; p2 = 4; }
            else if (r4 * 4 < r7 * 7 && r4 * 4 < r8 * 8) { p1 = 4; p2 = 2; }
            else if (r8 * 8 < r7 * 7) { p1 = 8; p2 = 1; }
            else { p1 = 7; p2 = 2; }
        }
        // p = <NW, KSP, SPW, D>: row tiles per workgroup, K over KSP waves per tile, stages per wave and ring step, ring depth.
        // short and wide (few row tiles, K beyond one LDS pass: OPT's fc2, 2048 x 8192, in a 5..16-row decode step): 4 tiles per workgroup
        // leave 32 workgroups on 256 CUs (12.3 us, profiles/r05c); one or two tiles per workgroup with K over 8 / 4 waves fill 128 / 64
        if (p1 == 1 && p2 == 8) return take(QUIPAMD_K2_S, 1, 8, 1, 2);
        if (p1 == 2 && p2 == 4) return take(QUIPAMD_K2_S, 2, 4, 1, 3);
        if (p1 == 7 && p2 == 2) return take(QUIPAMD_K2_S, 7, 2, 1, 3);
        // (round 6, lab: ring depth 4 / 5 and two stages per k-half and ring step for the 7 x 2 form -- 15.2 / 16.0 / 15.6 us against 15.0 at
        //  28672 x 7168 bs 16, profiles/r06G_k2_s_cfgs.jsonl: the per-step barrier is not what the compute waves wait for; not in the library)
        if (p1 == 4 && p2 == 2) return take(QUIPAMD_K2_S, 4, 2, 1, 4);
        if (p1 == 8 && p2 == 1) return take(QUIPAMD_K2_S, 8, 1, 2, 3);
        return refuse(k2_refuse(QUIPAMD_ERR_UNSUPPORTED, true, "dequant_gemm: no s kernel for nw=%d ksp=%d", p1, p2));
    }
    if (fam == K2_FAM_MB) {
        if (!mb_ok) return refuse(k2_refuse(QUIPAMD_ERR_UNSUPPORTED, true, "dequant_gemm: kernel family mb needs d %% 256 == 0"));
        // FOUR loader waves since round 5 (45 / 23; 44 / 22 are the two-loader forms of rounds 2-4).  The loaders were the bound: a loader
        // issues its share of the stage's 80 DMA instructions (each behind an s_mov m0), waits for ALL of them, meets the barrier; with
        // one loader 593 TF, two 998, three 1272, four 1323 at 28672 x 7168 bs 256 (4096^2 x 2048: 1078 -> 1268), six 585 -- 14 waves leave 128 registers per wave, the 4 x 4 tiles need 150
        // (profiles/r05j_k2lab_mb.txt, r05k_k2lab_mb_loaders.txt).  Halving the VALU per MFMA instead (48: 4 x 8 tiles per wave) bought nothing.
        if (p1 == 0) p1 = (((m + 255) / 256) * ((bs + 127) / 128) >= 200) ? K2_MB_256x128_L4 : K2_MB_128x64_L4;
        // p = <WB, RTw, BTw, NL, T32> (WR = 4 row groups of waves in every form): batch groups of waves, row / batch tiles per wave, loader waves
        if (p1 == K2_MB_256x128_L2 || p1 == K2_MB_256x128_L4)              // 256 rows x 128 batch rows, 4 x 4 tiles per wave (4 bit: 128 rows)
            return take(QUIPAMD_K2_MB, 2, BITS == 2 ? 4 : 2, 4, p1 == K2_MB_256x128_L4 ? 4 : 2);
        if (p1 == K2_MB_128x64_L2) return take(QUIPAMD_K2_MB, 2, 2, 2, 2);   // 128 rows x  64 batch rows
        if (p1 == K2_MB_128x64_L4) return take(QUIPAMD_K2_MB, 2, 2, 2, 4);
        if (BITS == 2) {
            // round 5 lab configurations (forced only)
            if (p1 == K2_MB_256x128_L3) return take(QUIPAMD_K2_MB, 2, 4, 4, 3);
            // the same tile on v_mfma_f32_32x32x16 (dq_mb_kernel<..., T32>)
            if (p1 == K2_MB_256x128_T32) return take(QUIPAMD_K2_MB, 2, 4, 4, 4, 1);
            // ONE compute wave per SIMD with 4 x 8 accumulator tiles: every dequantised A fragment feeds 8 MFMAs instead of 4 (VALU per MFMA
            // 2.35 -> ~1.2), same workgroup tile, same LDS reads per step: 992 vs 998 TF with two loaders, 1256 vs 1323 with four
            if (p1 == K2_MB_WIDE_L2) return take(QUIPAMD_K2_MB, 1, 4, 8, 2);
            if (p1 == K2_MB_WIDE_L4) return take(QUIPAMD_K2_MB, 1, 4, 8, 4);
        }
        return refuse(k2_refuse(QUIPAMD_ERR_UNSUPPORTED, true, "dequant_gemm: no mb kernel %d", p1));
    }
    return refuse(k2_refuse(QUIPAMD_ERR_UNSUPPORTED, true, "dequant_gemm: fp16 activations need d %% 256 == 0 (d=%lld)", (long long)d));
}

// ---- 2..3 fp16 problems of ONE shape as one launch (dq_hg_kernel / dq_sg_kernel: the problem picked by blockIdx.y) -----------------------
// `false`: the grouped kernels do not hold the shape, the group runs as one launch per problem.
inline bool k2_plan_v2_grouped(const K2Shape &c, int form, K2Plan &out)
{
    const int ngroups = c.ngroups, BITS = c.cbits;
    const int64_t nkc = c.d / (512 / BITS), tiles = c.m / 16;
    // the shapes a decode step groups: fp16, <= 16 rows, K within one LDS pass; the h kernel's own limit of 768 row tiles per problem
    if (ngroups < 2 || ngroups > 3 || c.x_dtype != QUIPAMD_F16 || c.bs > 16 || nkc > (BITS == 2 ? 16 : 32) || c.accumulate || tiles > 768)
        return false;
    auto take = [&](int kernel, int a, int b, int c2, int d2 = 0) { out = k2_take(kernel, 1, a, b, c2, d2); return true; };
    if (BITS == 2 && nkc > 8) {
        // Row tiles per workgroup: every workgroup pulls ALL of x~ (128 KiB at d = 4096), so a grid of many rounds of one-per-CU workgroups
        // pays that ingest once per round -- Llama's gate / up at 16 rows is 2 x 688 tiles = 5.4 rounds of 256 at RT 1.  With RT row tiles
        // per workgroup the grid is RT times smaller and each x~ slab feeds RT weight tiles.  (For ONE round -- the headline, 256 tiles -- RT > 1
        // lost at every shape in round 2; form 1 | 2 | 4 forces it for A/B runs.)
        // (8 row tiles -- Llama's gate / up as ONE round of 172 workgroups -- measured slower than 4: Llama-2-7B at 16 sequences 3.27 ms per step against
        //  3.18, at 8 sequences 2.88 against 2.76, profiles/r05w_hg_rt8_llama.txt; the instantiation is not kept.)
        // Round 6: beyond two rounds of one-per-CU workgroups the grouped WEIGHT-STREAM kernel (dq_sg_kernel: x~ staged once per 4 / 7 / 8 row
        // tiles by a loader wave, weights through the LDS ring) instead of the h kernel, whose every workgroup ingests all of x~ by itself.
        // form 74 / 72 / 81 force its <4,2,1,4> / <7,2,1,3> / <8,1,2,3> forms, 1 / 2 / 4 the h kernel's row tiles (A/B runs).
        int sg = (tiles * ngroups > 512) ? K2_SG_DEFAULT : 0;
        if (form == K2_SG_4x2 || form == K2_SG_7x2 || form == K2_SG_8x1) sg = form;
        else if (form == 1 || form == 2 || form == 4) sg = 0;
        if (sg == K2_SG_4x2) return take(QUIPAMD_K2_SG, 4, 2, 1, 4);
        if (sg == K2_SG_7x2) return take(QUIPAMD_K2_SG, 7, 2, 1, 3);
        if (sg == K2_SG_8x1) return take(QUIPAMD_K2_SG, 8, 1, 2, 3);
        int rt = 1;
        if (tiles * ngroups > 256 && tiles % 2 == 0) rt = 2;
        if (tiles * ngroups > 512 && tiles % 4 == 0) rt = 4;
        if ((form == 1 || form == 2 || form == 4) && tiles % form == 0) rt = form;
        return take(QUIPAMD_K2_HG, rt, 4, 4);
    }
    if (BITS == 2) {                                                                 // d <= 2048: 8 waves x 1 chunk
        int rt = (tiles * ngroups > 256 && tiles % 2 == 0) ? 2 : 1;
        if ((form == 1 || form == 2) && tiles % form == 0) rt = form;
        return take(QUIPAMD_K2_HG, rt, 8, 1);
    }
    return take(QUIPAMD_K2_HG, 1, 8, nkc <= 16 ? 2 : 4);
}

// ---- the round-1 kernels (dqgemm.hip; bf16) ---------------------------------------------------------------------------------------------------
// Shape heuristic.  BT: as many batch tiles per wave as the batch has (weights streamed once per 64 batch
// rows).  RT: row tiles per workgroup -- more rows per workgroup means fewer x bytes into the chip
// (every workgroup ingests the whole x), but the grid must still cover the 256 CUs.
inline K2Plan k2_plan_r1(const K2Shape &c, const K2Tune &t)
{
    const int BITS = c.cbits, KC = 512 / BITS, ngroups = c.ngroups;
    const int64_t ntile = c.m / 16;
    const int64_t nb = (c.bs + 15) / 16;
    if (nb == 1 && t.bt == 0) {
        // tile kernel.  rt: row tiles per workgroup (x slab reuse); cw: chunks in flight per workgroup;
        // S: k-slices over workgroups (atomics; accumulate contract only).
        const int64_t nkc = c.d / KC;
        const bool can_split = c.accumulate && c.y_dtype == QUIPAMD_F32;
        // Choices below are the winners of the shape sweeps under profiles/r01f_* (2-bit, bs 1 and 16).  Large m / long K:
        // the per-wave kernel (every wave streams RT weight tiles per chunk: more bytes in flight per wave, private slabs);
        // small m: the tile kernel (all of a CU's bytes in flight at once, parallel reducers, optional split-K).
        const bool tuned = t.rt != 0 || t.nw != 0 || t.ksplit != 0 || t.depth != 0;
        int rt = 1, cw = 8, S = 1;
        if (!tuned && ntile % 4 == 0 && ntile >= 1024) return k2_take(QUIPAMD_K2_R1_WAVE, ngroups, 4, 1, 8);
        if (!tuned && ntile % 4 == 0 && ntile >= 640 && nkc >= 16) return k2_take(QUIPAMD_K2_R1_WAVE, ngroups, 4, 1, 16);
        if (!tuned && ntile % 2 == 0 && ntile >= 384 && nkc >= 24) return k2_take(QUIPAMD_K2_R1_WAVE, ngroups, 2, 1, 16);
        if (can_split && ntile % 2 == 0 && ntile / 2 < 256) {
            // small m under the accumulate contract: 8-wave workgroups (several resident per CU), k split over
            // workgroups until there are ~512 of them (measured best at 4096x4096: rt 2, cw 4, S 4)
            rt = 2; cw = 4;
            S = (int)((512 + ntile / 2 - 1) / (ntile / 2));
            if (S > nkc / cw) S = (int)(nkc / cw);
            if (S < 1) S = 1;
        }
        if (t.rt > 0 && ntile % t.rt == 0) { rt = t.rt; cw = 16 / rt; }
        if (t.nw > 0) cw = t.nw / rt > 0 ? t.nw / rt : 1;
        if (t.ksplit > 0) S = can_split ? t.ksplit : 1;
        int depth = 1;                       // measured: 2 or 4 groups in flight buy nothing at 4096^2 (profiles/r01f)
        if (t.depth > 0) depth = t.depth;
        // the instantiations: <RT, CW> with one group of chunks in flight, and with two where the slabs stay within 128 KiB of LDS
        static const int tile_forms[][2] = {{1, 16}, {1, 8}, {1, 4}, {1, 2}, {1, 1}, {2, 1}, {2, 8}, {2, 4}, {2, 2}, {4, 4}, {4, 2}, {4, 1}, {8, 2}, {8, 1}};
        for (const auto &f : tile_forms) {
            if (rt != f[0] || cw != f[1] || (f[0] == 8 && BITS != 2)) continue;
            if (depth == 1 || (depth == 2 && (size_t)cw * 2 * 16 * KC * 2 <= 128 * 1024))
                return k2_take(QUIPAMD_K2_R1_TILE, 1, rt, cw, depth, 0, 0, S);      // one launch: grid.y walks the problems of a group
            return k2_refuse(QUIPAMD_ERR_UNSUPPORTED, true, "dequant_gemm: depth %d does not fit LDS for cw=%d", depth, cw);
        }
        return k2_refuse(QUIPAMD_ERR_UNSUPPORTED, true, "dequant_gemm: no tile kernel for rt=%d cw=%d", rt, cw);
    }
    // bs > 16: one batch tile per workgroup (grid.y walks the batch tiles, weights re-streamed from L2 / Infinity Cache)
    // with as many row tiles per wave as the grid allows beat the BT > 1 variants at every swept shape.
    const int64_t nby64 = (c.bs + 63) / 64;
    if (t.bt == 0 && t.rt == 0 && t.nw == 0 && ngroups == 1 && !t.depth && ((nby64 >= 2 && ntile >= 512) || (nb >= 3 && ntile >= 1024))) {
        // batched kernel: (2*RT*16 rows) x 64 batch rows per workgroup; RT by how many workgroups the grid then has.
        // Wins for bs > 64 on m >= 8192 (or one 64-row batch tile on m >= 16384); on shorter matrices the per-wave kernel,
        // whose 16 waves split K, is faster (profiles/r01h_k2_batched_sweep.jsonl, r01h_k2_default_config_all_shapes.jsonl).
        if (ntile % 8 == 0 && (ntile / 8) * nby64 >= 512) return k2_take(QUIPAMD_K2_R1_BATCHED, 1, 4);
        if (ntile % 4 == 0 && (ntile / 4) * nby64 >= 256) return k2_take(QUIPAMD_K2_R1_BATCHED, 1, 2);
        if (ntile % 2 == 0) return k2_take(QUIPAMD_K2_R1_BATCHED, 1, 1);
    }
    if (t.force_batched && ngroups == 1) {                        // tuning: force the batched kernel, RT = t.rt
        if (t.rt == 4 && ntile % 8 == 0) return k2_take(QUIPAMD_K2_R1_BATCHED, 1, 4);
        if (t.rt == 2 && ntile % 4 == 0) return k2_take(QUIPAMD_K2_R1_BATCHED, 1, 2);
        if (t.rt == 1 && ntile % 2 == 0) return k2_take(QUIPAMD_K2_R1_BATCHED, 1, 1);
        return k2_refuse(QUIPAMD_ERR_UNSUPPORTED, true, "dequant_gemm: batched kernel needs rt in {1,2,4} dividing the row tiles");
    }
    int rt, bt = 1, nw = 16;
    if (ntile % 4 == 0 && (ntile / 4) * nb >= 128) rt = 4;
    else if (ntile % 2 == 0 && (ntile / 2) * nb >= 128) rt = 2;
    else rt = 1;
    if (t.rt > 0 && ntile % t.rt == 0) rt = t.rt;
    if (t.bt > 0) bt = t.bt;
    if (t.nw > 0) nw = t.nw;
    static const int wave_forms[][3] = {{1, 1, 16}, {2, 1, 16}, {4, 1, 16}, {1, 1, 8}, {2, 1, 8}, {4, 1, 8}, {1, 1, 4}, {2, 1, 4}, {4, 1, 4},
                                        {1, 2, 8}, {2, 2, 8}, {1, 2, 4}, {2, 2, 4}, {1, 4, 4}, {2, 4, 4}};
    for (const auto &f : wave_forms)
        if (rt == f[0] && bt == f[1] && nw == f[2]) return k2_take(QUIPAMD_K2_R1_WAVE, ngroups, rt, bt, nw);   // one problem of a group per launch
    return k2_refuse(QUIPAMD_ERR_UNSUPPORTED, true, "dequant_gemm: no kernel for rt=%d bt=%d nw=%d", rt, bt, nw);
}

// ---- the whole decision --------------------------------------------------------------------------------------------------------------------------
inline K2Plan k2_plan(const K2Shape &c, const K2Force &f)
{
    const int ngroups = c.ngroups;
    K2_REQUIRE(ngroups >= 1 && ngroups <= 4, QUIPAMD_ERR_ARG, false, "dequant_gemm: 1..4 problems per call");
    K2_REQUIRE(c.x_dtype == QUIPAMD_BF16 || c.x_dtype == QUIPAMD_F16, QUIPAMD_ERR_UNSUPPORTED, false, "dequant_gemm: x must be bf16 or fp16");
    K2_REQUIRE(c.y_dtype == c.x_dtype || c.y_dtype == QUIPAMD_F32, QUIPAMD_ERR_UNSUPPORTED, false, "dequant_gemm: y must be f32 or x's dtype");
    K2_REQUIRE(!c.accumulate || c.y_dtype == QUIPAMD_F32, QUIPAMD_ERR_UNSUPPORTED, false, "dequant_gemm: accumulate needs f32 y");
    // the native 3-bit layout has its own kernel family (dqgemm_w3.hip), taken on the layout value before anything below
    if (c.layout == QUIPAMD_LAYOUT_STREAM3) return k2_plan_w3(c, f.cfg);
    K2_REQUIRE(c.layout == QUIPAMD_LAYOUT_STREAM, QUIPAMD_ERR_UNSUPPORTED, false,
               "dequant_gemm: qweight must be in STREAM layout (repack with quipamd_unpack/quipamd_pack)");
    K2_REQUIRE(c.bits == 2 || c.bits == 3 || c.bits == 4, QUIPAMD_ERR_UNSUPPORTED, false, "dequant_gemm: bits must be 2, 3 or 4");
    const int bits = c.cbits;
    K2_REQUIRE(c.qfn == QUIPAMD_QFN_B || c.qfn == QUIPAMD_QFN_A, QUIPAMD_ERR_ARG, false, "dequant_gemm: qfn must be a or b");
    K2_REQUIRE(c.bs * c.d * 2 < ((int64_t)1 << 31) && c.m * c.d * bits / 8 < ((int64_t)1 << 40), QUIPAMD_ERR_SHAPE, false,
               "dequant_gemm: x larger than 2 GiB is not supported by the 32-bit buffer offsets (bs=%lld d=%lld)", (long long)c.bs, (long long)c.d);
    K2_REQUIRE(c.m % 16 == 0 && c.d % (512 / bits) == 0, QUIPAMD_ERR_SHAPE, false,
               "dequant_gemm: needs m %% 16 == 0 and d %% %d == 0 (m=%lld d=%lld)", 512 / bits, (long long)c.m, (long long)c.d);
    if (c.bs == 0 || c.m == 0) return k2_take(QUIPAMD_K2_NONE, 0);
    // A thread under quipamd_tune_dequant_gemm asks for the round-1 kernels, unless the call itself names a family
    const bool v2 = !(f.tune.any() && f.cfg.family == 0);
    K2Plan p;
    // second-generation kernels first; they decline the shapes the round-1 kernels serve better
    if (ngroups == 1 && v2 && k2_plan_v2(c, f.cfg, 1, p)) return p;
    if (ngroups > 1 && c.x_dtype == QUIPAMD_F16 && v2) {
        // fp16 activations exist only in the second-generation kernels: 2..3 problems of one shape as ONE launch of a grouped kernel where
        // it holds the shape, else one launch per problem (the shape heuristic; a cfg is per single call)
        if (ngroups <= 3 && c.qfn == QUIPAMD_QFN_B && k2_plan_v2_grouped(c, f.grouped_form, p)) return p;
        if (k2_plan_v2(c, K2Cfg{0, 0, 0, 0}, ngroups, p)) return p;
        return k2_refuse(QUIPAMD_ERR_UNSUPPORTED, true, "dequant_gemm_grouped: no fp16 kernel for this shape (m=%lld d=%lld bs=%lld)",
                         (long long)c.m, (long long)c.d, (long long)c.bs);
    }
    K2_REQUIRE(c.x_dtype == QUIPAMD_BF16, QUIPAMD_ERR_UNSUPPORTED, true, "dequant_gemm: the round-1 kernels are bf16 only");
    return k2_plan_r1(c, f.tune);
}
