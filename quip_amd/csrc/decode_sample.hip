// decode_sample.hip -- one token per row by temperature / top-k / top-p sampling, ONE launch (include/quip_amd_sample.h)
//
// One workgroup of 1024 threads per row, like argmax_rows_kernel.  The row is read in segments of 512 consecutive entries, one wave per
// segment, eight entries per lane (one 16-byte load where the row allows it); it is read again from L2 by every pass:
//
//   pass 0    the maximum and its first index (argmax_rows' comparison).  Greedy rows end here.
//   select    both truncations are a cut (key, ties) in the order "z descending, ties by smaller index": key is the inverted
//             order-preserving uint32 image of z, so the order is key ascending.  A radix select over the key finds the cut: digits of
//             12, 10 and 10 bits, per digit an LDS histogram of counts (top-k walks them) and of masses (top-p walks them; top-k takes
//             its softmax denominator from them).  The 12-bit histogram is over the whole row and serves both selects, the two
//             narrower ones are over the entries of the threshold bin only: 3 passes for one truncation, 5 for both.
//   draw      one pass forms the survivors' mass per segment, a block scan finds the segment that holds u * Z, one wave walks its 512
//             entries in index order.
//
// Determinism: a weight is the fp32 exp(z - max z); every SUM of weights is carried in 2^-40 fixed point, in 64-bit integers (at most
// 2^18 terms of at most 2^40).  Integer addition is associative, so the LDS atomics of the histograms, the wave reductions and the scans
// give the same bits in any order -- there is no floating-point sum in this file.  The draw compares integers: C_i * 2^24 > (x0 >> 8) * Z.
//
// The device code is csrc/sample_body.h, which decode_generate.hip (stop tokens, repetition penalty, per-row parameters) shares.
#include "common.h"
#include "quip_amd_sample.h"
#include "sample_body.h"

namespace {

struct SampleArgs {
    const void *logits;
    int n, vec;
    int64_t ld;
    const quipamd_sample_params *params;
    const int64_t *counter;
    int64_t *out;
    float *logprob;
    int32_t *kept_n;
    float *kept_mass;
    int32_t *clear;
    int64_t clear_n;
};

template <class TI> __global__ __launch_bounds__(1024) void sample_rows_kernel(SampleArgs A)
{
    typedef typename DT<TI>::storage storage;
    __shared__ Shared S;
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x;
    const storage *row = (const storage *)A.logits + r * A.ld;

    if (A.clear)
        for (int64_t i = tid; i < A.clear_n; i += 1024) A.clear[r * A.clear_n + i] = -1;

    int tok, kn;
    float lp, kmass;
    sample_row<TI, false>(S, row, A.n, A.vec, Pen{nullptr, 1.f}, A.params->temperature, A.params->top_p, A.params->top_k, &A.params->seed, A.counter,
                          (uint32_t)r, tok, lp, kn, kmass);
    if (tid == 0) {
        A.out[r] = tok;
        if (A.logprob) A.logprob[r] = lp;
        if (A.kept_n) A.kept_n[r] = kn;
        if (A.kept_mass) A.kept_mass[r] = kmass;
    }
}

}   // namespace

extern "C" int quipamd_sample_rows(const void *logits, int dtype, int64_t rows, int64_t n, int64_t ld, const quipamd_sample_params *params,
                                   const int64_t *counter, int64_t *out, float *logprob, int32_t *kept_n, float *kept_mass, int32_t *clear,
                                   int64_t clear_n, void *stream)
{
    QA_REQUIRE(rows >= 0 && rows <= 65535 && n >= 1 && n <= SAMPLE_MAX_N && ld >= n, QUIPAMD_ERR_SHAPE,
               "sample_rows: bad shape (rows %lld in 0..65535, n %lld in 1..%d, ld %lld >= n)", (long long)rows, (long long)n, SAMPLE_MAX_N, (long long)ld);
    QA_REQUIRE(!clear || clear_n > 0, QUIPAMD_ERR_ARG, "sample_rows: clear needs clear_n > 0 (got %lld)", (long long)clear_n);
    QA_REQUIRE(dtype == QUIPAMD_F32 || dtype == QUIPAMD_F16 || dtype == QUIPAMD_BF16, QUIPAMD_ERR_ARG, "bad dtype %d", dtype);
    if (rows == 0) return QUIPAMD_OK;
    QA_REQUIRE(logits && params && counter && out, QUIPAMD_ERR_ARG, "sample_rows: null pointer");
    SampleArgs A;
    A.logits = logits; A.n = (int)n; A.ld = ld; A.params = params; A.counter = counter; A.out = out; A.logprob = logprob; A.kept_n = kept_n;
    A.kept_mass = kept_mass; A.clear = clear; A.clear_n = clear ? clear_n : 0;
    A.vec = (dtype != QUIPAMD_F32 && (uintptr_t)logits % 16 == 0 && ld % 8 == 0) ? 1 : 0;          // every row starts on a 16-byte boundary
    hipStream_t s = (hipStream_t)stream;
    QA_DISPATCH_DTYPE(dtype, TI, (sample_rows_kernel<TI><<<(unsigned)rows, 1024, 0, s>>>(A)));
    QA_LAUNCH_CHECK("quipamd_sample_rows");
    return QUIPAMD_OK;
}
