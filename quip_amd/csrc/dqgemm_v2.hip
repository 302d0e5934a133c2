// dqgemm_v2.hip -- instantiations of the second-generation K2 kernels (dqgemm_v2.h) and the switch from a plan to one of them.
// Which kernel serves a call is decided in k2_plan.h (k2_plan_v2, k2_plan_v2_grouped); k2v2_run() below executes that plan and decides
// nothing.  The set of instantiations is the set of cases in the three switches.
#include "dqgemm_v2.h"
#include "k2_dispatch.h"

namespace {

#define K2_FORM3(A_, B_, C_) if (p.p[0] == A_ && p.p[1] == B_ && p.p[2] == C_)
#define K2_FORM4(A_, B_, C_, D_) if (p.p[0] == A_ && p.p[1] == B_ && p.p[2] == C_ && p.p[3] == D_)
#define K2_FORM_MB(WB_, RT_, BT_, NL_, T32_) \
    if (p.p[0] == WB_ && p.p[1] == RT_ && p.p[2] == BT_ && p.p[3] == NL_ && p.p[4] == T32_) return launch_mb2<BITS, ACT, 4, WB_, RT_, BT_, NL_, T32_>(A, s)

// one problem
template <int BITS, class ACT>
int run_one(const K2Plan &p, const K2Args &A, hipStream_t s)
{
    switch (p.kernel) {
    case QUIPAMD_K2_H:                                                  // <RT, NW, NCH>
        if constexpr (BITS == 2) {
            K2_FORM3(2, 8, 1) return launch_h<2, ACT, 2, 8, 1>(A, s);
            K2_FORM3(2, 4, 4) return launch_h<2, ACT, 2, 4, 4>(A, s);
            K2_FORM3(4, 4, 4) return launch_h<2, ACT, 4, 4, 4>(A, s);
            K2_FORM3(1, 8, 1) return launch_h<2, ACT, 1, 8, 1>(A, s);
            K2_FORM3(1, 8, 2) return launch_h<2, ACT, 1, 8, 2>(A, s);
            K2_FORM3(1, 16, 1) return launch_h<2, ACT, 1, 16, 1>(A, s);
            K2_FORM3(1, 4, 4) return launch_h<2, ACT, 1, 4, 4>(A, s);
        } else {
            K2_FORM3(1, 8, 2) return launch_h<4, ACT, 1, 8, 2>(A, s);
            K2_FORM3(1, 8, 4) return launch_h<4, ACT, 1, 8, 4>(A, s);
        }
        break;
    case QUIPAMD_K2_H_HALF:                                             // 8-row slabs, <1, 8, 4>; EXACT: d = 8192
        if constexpr (BITS == 2)
            return A.d / 256 == 32 ? launch_h2<2, ACT, 1, 8, 4, true, true>(A, s) : launch_h2<2, ACT, 1, 8, 4, true, false>(A, s);
        break;
    case QUIPAMD_K2_H_HALF_X2:                                          // rows 0..7 and rows 8.. of x and y as two problems that share the weights
        if constexpr (BITS == 2) {
            K2GArgs G;
            G.g[0] = A; G.g[1] = A; G.g[2] = A;
            G.g[0].e.bs = 8;
            G.g[1].e.bs = A.e.bs - 8;
            G.g[1].x = A.x + 8 * A.d;
            G.g[1].e.y = (char *)A.e.y + (size_t)8 * A.e.m * (A.e.y_f32 ? 4 : 2);
            return A.d / 256 == 32 ? launch_h2g<2, ACT, 1, 8, 4, true, true>(G, 2, s) : launch_h2g<2, ACT, 1, 8, 4, true, false>(G, 2, s);
        }
        break;
    case QUIPAMD_K2_HR:
        if constexpr (BITS == 2) return launch_hr<2, ACT, 4, 4>(A, s);
        break;
    case QUIPAMD_K2_S:                                                  // <NW, KSP, SPW, D>
        K2_FORM4(1, 8, 1, 2) return launch_s<BITS, ACT, 1, 8, 1, 2>(A, s);
        K2_FORM4(2, 4, 1, 3) return launch_s<BITS, ACT, 2, 4, 1, 3>(A, s);
        K2_FORM4(7, 2, 1, 3) return launch_s<BITS, ACT, 7, 2, 1, 3>(A, s);
        K2_FORM4(4, 2, 1, 4) return launch_s<BITS, ACT, 4, 2, 1, 4>(A, s);
        K2_FORM4(8, 1, 2, 3) return launch_s<BITS, ACT, 8, 1, 2, 3>(A, s);
        break;
    case QUIPAMD_K2_MB:                                                 // <WB, RTw, BTw, NL, T32>, WR = 4
        K2_FORM_MB(2, 2, 2, 2, false);
        K2_FORM_MB(2, 2, 2, 4, false);
        if constexpr (BITS == 2) {
            K2_FORM_MB(2, 4, 4, 2, false);
            K2_FORM_MB(2, 4, 4, 4, false);
            K2_FORM_MB(2, 4, 4, 3, false);
            K2_FORM_MB(2, 4, 4, 4, true);
            K2_FORM_MB(1, 4, 8, 2, false);
            K2_FORM_MB(1, 4, 8, 4, false);
        } else {
            K2_FORM_MB(2, 2, 4, 2, false);
            K2_FORM_MB(2, 2, 4, 4, false);
        }
        break;
    }
    return qa_fail(QUIPAMD_ERR_UNSUPPORTED, "dequant_gemm: the plan names no instantiation (kernel %d: %d %d %d %d %d, %d bits)", p.kernel, p.p[0],
                   p.p[1], p.p[2], p.p[3], p.p[4], BITS);
}

// 2..3 fp16 problems of one shape in one launch
int run_grouped(const K2Plan &p, const K2GArgs &G, int ngroups, int bits, hipStream_t s)
{
    if (p.kernel == QUIPAMD_K2_SG && bits == 2) {                       // <NW, KSP, SPW, D>
        K2_FORM4(4, 2, 1, 4) return launch_sg<2, ActF16, 4, 2, 1, 4>(G, ngroups, s);
        K2_FORM4(7, 2, 1, 3) return launch_sg<2, ActF16, 7, 2, 1, 3>(G, ngroups, s);
        K2_FORM4(8, 1, 2, 3) return launch_sg<2, ActF16, 8, 1, 2, 3>(G, ngroups, s);
    }
    if (p.kernel == QUIPAMD_K2_HG && bits == 2) {                       // <RT, NW, NCH>
        K2_FORM3(4, 4, 4) return launch_hg<2, ActF16, 4, 4, 4>(G, ngroups, s);
        K2_FORM3(2, 4, 4) return launch_hg<2, ActF16, 2, 4, 4>(G, ngroups, s);
        K2_FORM3(1, 4, 4) return launch_hg<2, ActF16, 1, 4, 4>(G, ngroups, s);
        K2_FORM3(2, 8, 1) return launch_hg<2, ActF16, 2, 8, 1>(G, ngroups, s);
        K2_FORM3(1, 8, 1) return launch_hg<2, ActF16, 1, 8, 1>(G, ngroups, s);
    }
    if (p.kernel == QUIPAMD_K2_HG && bits == 4) {
        K2_FORM3(1, 8, 2) return launch_hg<4, ActF16, 1, 8, 2>(G, ngroups, s);
        K2_FORM3(1, 8, 4) return launch_hg<4, ActF16, 1, 8, 4>(G, ngroups, s);
    }
    return qa_fail(QUIPAMD_ERR_UNSUPPORTED, "dequant_gemm_grouped: the plan names no instantiation (kernel %d: %d %d %d %d, %d bits)", p.kernel,
                   p.p[0], p.p[1], p.p[2], p.p[3], bits);
}
#undef K2_FORM3
#undef K2_FORM4
#undef K2_FORM_MB

}   // namespace

int k2v2_run(const K2Plan &p, const K2Shape &c, const K2Problem *pr, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (p.kernel == QUIPAMD_K2_HG || p.kernel == QUIPAMD_K2_SG) {
        K2GArgs G;
        for (int i = 0; i < 3; ++i) k2_fill_args(G.g[i], c, pr[i < c.ngroups ? i : 0]);
        return run_grouped(p, G, c.ngroups, c.cbits, s);
    }
    const bool f16 = c.x_dtype == QUIPAMD_F16;
    for (int gi = 0; gi < p.launches; ++gi) {
        K2Args A;
        k2_fill_args(A, c, pr[gi]);
        const int rc = f16 ? (c.cbits == 2 ? run_one<2, ActF16>(p, A, s) : run_one<4, ActF16>(p, A, s))
                           : (c.cbits == 2 ? run_one<2, ActBF16>(p, A, s) : run_one<4, ActBF16>(p, A, s));
        if (rc != QUIPAMD_OK) return rc;
    }
    return QUIPAMD_OK;
}
