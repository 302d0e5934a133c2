// decode_generate.hip -- the launch that ends a decode step under generation control, ONE launch (include/quip_amd_generate.h):
// quipamd_sample_rows' token per row with per-row parameters, a repetition penalty over the row's history, and stop tokens.
//
// One workgroup of 1024 threads per row; the passes over the row are sample_row() of csrc/sample_body.h, the code quipamd_sample_rows runs.
// Around them, per row:
//
//   history   hist[r, c - 1] = fed[r] (c = *counter), then one bit per vocabulary entry in LDS: bit id is set for every id in
//             hist[r, 0 : min(c, hist_cap)] that lies in [0, n) (atomicOr; a barrier).  The passes penalise entry i as they LOAD it when
//             bit i is set (sample_body.h's PEN flag), so "once per distinct id" is the bitmap, all passes see one row, and the logits stay
//             as the model wrote them.  A row with penalty 1 or nothing to read runs the unpenalised instantiation and builds no bitmap.
//   stop      a row that is done on entry returns pad_id before any pass; a row whose token is a stop id sets done and stop_pos.
//
// LDS: sample_body.h's Shared (about 60 KiB) and behind it the bitmap, n / 8 bytes (32 KiB at n = 262144), both in the dynamic region;
// with a history the launch asks for more than the default limit, which qa_lds<> raises.  Nothing here depends on timing: the only
// cross-thread hand-offs are LDS words between barriers of one workgroup, and the sums are sample_body.h's integers.
#include "common.h"
#include "quip_amd_generate.h"
#include "sample_body.h"

namespace {

constexpr size_t SHARED_BYTES = (sizeof(Shared) + 15) / 16 * 16;

struct GenerateArgs {
    const void *logits;
    int n, vec;
    int64_t ld;
    const quipamd_generate_params *params;
    const int64_t *counter;
    int32_t *hist;
    int64_t hist_cap, ld_hist;
    const int64_t *fed;
    const int32_t *stop_ids;
    int n_stop;
    int32_t pad_id;
    int32_t *done;
    int64_t *stop_pos;
    int64_t *out;
    float *logprob;
    int32_t *kept_n;
    float *kept_mass;
    int32_t *clear;
    int64_t clear_n;
};

template <class TI> __global__ __launch_bounds__(1024) void generate_rows_kernel(GenerateArgs A)
{
    typedef typename DT<TI>::storage storage;
    extern __shared__ __attribute__((aligned(16))) unsigned char generate_lds[];
    Shared &S = *reinterpret_cast<Shared *>(generate_lds);
    uint32_t *seen = reinterpret_cast<uint32_t *>(generate_lds + SHARED_BYTES);      // (n + 31) / 32 words when A.hist is given, else nothing
    const int tid = threadIdx.x;
    const int n = A.n;
    const int64_t r = blockIdx.x;
    const storage *row = (const storage *)A.logits + r * A.ld;

    if (A.clear)
        for (int64_t i = tid; i < A.clear_n; i += 1024) A.clear[r * A.clear_n + i] = -1;

    const int64_t c = *A.counter;
    int32_t *hist = A.hist ? A.hist + r * A.ld_hist : nullptr;
    const bool feed = hist && A.fed && c >= 1 && c - 1 < A.hist_cap;
    const int32_t fed = feed ? (int32_t)A.fed[r] : 0;                                // read here, in front of every barrier: `out` may be `fed`
    if (feed && tid == 0) hist[c - 1] = fed;
    const bool here = hist && c >= 0 && c < A.hist_cap;                              // position c exists in the history

    if (A.done && A.done[r] != 0) {                                                  // (the whole workgroup: done[r] is written by its thread 0 only, below)
        if (tid == 0) {
            A.out[r] = A.pad_id;
            if (A.logprob) A.logprob[r] = 0.f;
            if (A.kept_n) A.kept_n[r] = 0;
            if (A.kept_mass) A.kept_mass[r] = 1.f;
            if (here) hist[c] = A.pad_id;
        }
        return;
    }

    const quipamd_generate_params *prm = A.params + r;
    const float T = prm->temperature, P = prm->top_p, rp = prm->repetition_penalty;
    const int K = prm->top_k;
    const int hl = !hist ? 0 : c < 0 ? 0 : c < A.hist_cap ? (int)c : (int)A.hist_cap;   // positions 0 .. hl - 1 are read
    const bool pen_on = hl > 0 && rp != 1.f;

    int tok, kn;
    float lp, kmass;
    if (pen_on) {
        const int words = (n + 31) >> 5;
        for (int i = tid; i < words; i += 1024) seen[i] = 0;
        __syncthreads();
        for (int i = tid; i < hl; i += 1024) {
            const int32_t id = (feed && i == c - 1) ? fed : hist[i];                 // (the store above is another thread's: take the value itself)
            if (id >= 0 && id < n) atomicOr(&seen[id >> 5], 1u << (id & 31));
        }
        __syncthreads();
        sample_row<TI, true>(S, row, n, A.vec, Pen{seen, rp}, T, P, K, &prm->seed, A.counter, (uint32_t)r, tok, lp, kn, kmass);
    } else {
        sample_row<TI, false>(S, row, n, A.vec, Pen{nullptr, 1.f}, T, P, K, &prm->seed, A.counter, (uint32_t)r, tok, lp, kn, kmass);
    }

    if (tid == 0) {
        A.out[r] = tok;
        if (A.logprob) A.logprob[r] = lp;
        if (A.kept_n) A.kept_n[r] = kn;
        if (A.kept_mass) A.kept_mass[r] = kmass;
        if (here) hist[c] = tok;
        bool stop = false;
        for (int j = 0; j < A.n_stop; ++j) stop = stop || A.stop_ids[j] == tok;
        if (stop) {
            if (A.done) A.done[r] = 1;
            if (A.stop_pos) A.stop_pos[r] = c;
        }
    }
}

template <class TI> int launch_generate(const GenerateArgs &A, int64_t rows, size_t lds, hipStream_t s)
{
    constexpr auto kern = generate_rows_kernel<TI>;
    if (int rc = qa_lds<kern>(lds, "generate_rows")) return rc;
    kern<<<(unsigned)rows, 1024, lds, s>>>(A);
    QA_LAUNCH_CHECK("quipamd_generate_rows");
    return QUIPAMD_OK;
}

}   // namespace

extern "C" int quipamd_generate_rows(const void *logits, int dtype, int64_t rows, int64_t n, int64_t ld, const quipamd_generate_params *params,
                                     const int64_t *counter, int32_t *hist, int64_t hist_cap, int64_t ld_hist, const int64_t *fed,
                                     const int32_t *stop_ids, int64_t n_stop, int64_t pad_id, int32_t *done, int64_t *stop_pos, int64_t *out,
                                     float *logprob, int32_t *kept_n, float *kept_mass, int32_t *clear, int64_t clear_n, void *stream)
{
    QA_REQUIRE(rows >= 0 && rows <= 65535 && n >= 1 && n <= SAMPLE_MAX_N && ld >= n, QUIPAMD_ERR_SHAPE,
               "generate_rows: bad shape (rows %lld in 0..65535, n %lld in 1..%d, ld %lld >= n)", (long long)rows, (long long)n, SAMPLE_MAX_N, (long long)ld);
    QA_REQUIRE(!clear || clear_n > 0, QUIPAMD_ERR_ARG, "generate_rows: clear needs clear_n > 0 (got %lld)", (long long)clear_n);
    QA_REQUIRE(dtype == QUIPAMD_F32 || dtype == QUIPAMD_F16 || dtype == QUIPAMD_BF16, QUIPAMD_ERR_ARG, "bad dtype %d", dtype);
    QA_REQUIRE(n_stop >= 0 && n_stop <= QUIPAMD_GENERATE_MAX_STOP, QUIPAMD_ERR_ARG, "generate_rows: n_stop %lld outside 0..%d", (long long)n_stop,
               QUIPAMD_GENERATE_MAX_STOP);
    QA_REQUIRE(!hist || (hist_cap >= 1 && hist_cap <= 0x7fffffffll && ld_hist >= hist_cap), QUIPAMD_ERR_SHAPE,
               "generate_rows: hist needs hist_cap >= 1 and ld_hist >= hist_cap (got hist_cap %lld, ld_hist %lld)", (long long)hist_cap, (long long)ld_hist);
    QA_REQUIRE(pad_id >= 0 && pad_id <= 0x7fffffffll, QUIPAMD_ERR_ARG, "generate_rows: pad_id %lld outside 0..2^31-1", (long long)pad_id);
    if (rows == 0) return QUIPAMD_OK;
    QA_REQUIRE(logits && params && counter && out, QUIPAMD_ERR_ARG, "generate_rows: null pointer");
    GenerateArgs A;
    A.logits = logits; A.n = (int)n; A.ld = ld; A.params = params; A.counter = counter;
    A.hist = hist; A.hist_cap = hist ? hist_cap : 0; A.ld_hist = hist ? ld_hist : 0; A.fed = fed;
    A.stop_ids = stop_ids; A.n_stop = stop_ids ? (int)n_stop : 0; A.pad_id = (int32_t)pad_id; A.done = done; A.stop_pos = stop_pos;
    A.out = out; A.logprob = logprob; A.kept_n = kept_n; A.kept_mass = kept_mass; A.clear = clear; A.clear_n = clear ? clear_n : 0;
    A.vec = (dtype != QUIPAMD_F32 && (uintptr_t)logits % 16 == 0 && ld % 8 == 0) ? 1 : 0;          // every row starts on a 16-byte boundary
    const size_t lds = SHARED_BYTES + (hist ? ((size_t)(n + 31) / 32 * 4 + 15) / 16 * 16 : 0);    // the bitmap is sized by n
    hipStream_t s = (hipStream_t)stream;
    QA_DISPATCH_DTYPE(dtype, TI, return launch_generate<TI>(A, rows, lds, s));
    return QUIPAMD_OK;
}
