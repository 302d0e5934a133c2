// k2_dispatch.h -- what the three K2 translation units share: the plan (k2_plan.h), the pointers of one problem, and the functions that
// execute a plan.  (EpiArgs / K2Args live in an anonymous namespace per translation unit -- the kernels' symbols carry it -- so the
// pointers cross as this plain record and each unit fills its own argument structs from it and the shape.)
#pragma once
#include "k2_plan.h"

struct K2Problem {
    const void *x;            // [bs, d] bf16 / fp16
    const void *qweight;
    const float *scale, *zero, *bias;
    void *y;
};

// execute a plan whose kernel is the unit's (h .. mb: dqgemm_v2.hip; w3: dqgemm_w3.hip); pr[0 .. ngroups).  QUIPAMD_OK or an error status
int k2v2_run(const K2Plan &p, const K2Shape &c, const K2Problem *pr, void *stream);
int k2w3_run(const K2Plan &p, const K2Shape &c, const K2Problem *pr, void *stream);

// The per-problem argument records, filled in ONE place.  EPI = the unit's EpiArgs, ARGS = its K2Args.
template <class EPI> inline void k2_fill_epi(EPI &e, const K2Shape &c, const K2Problem &p)
{
    e.scale = p.scale; e.zero = p.zero; e.bias = p.bias; e.y = p.y;
    e.qfn = c.qfn; e.maxq = (1 << c.bits) - 1;              // the grid of the codes as passed: 7 for 3-bit codes in the 4-bit container
    e.two_over_maxq = 2.0f / (float)e.maxq;
    e.y_f32 = c.y_dtype == QUIPAMD_F32; e.y_f16 = c.y_dtype == QUIPAMD_F16; e.accumulate = c.accumulate; e.bs = c.bs; e.m = c.m;
}
template <class ARGS> inline void k2_fill_args(ARGS &A, const K2Shape &c, const K2Problem &p)
{
    A.x = (decltype(A.x))p.x; A.qw = (decltype(A.qw))p.qweight; A.d = c.d;
    k2_fill_epi(A.e, c, p);
}
