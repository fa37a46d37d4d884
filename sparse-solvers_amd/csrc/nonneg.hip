// nonneg.hip — coding under x >= 0, a fit that only adds atoms (include/ss_hip.h):
//   ss_hip_nonneg_top_correlations_*, ss_hip_nonneg_refit_records_*.
//
// Parts-based dictionaries — training faces or spectra as columns, abundances in unmixing, SRC variants that forbid subtracting one
// subject from another — want min || y_b - A x ||_2 over sparse x >= 0.  The unconstrained coders cannot give it: their selection
// ranks |a_i . r_b| and their refit lets a coefficient take either sign.  Two pieces make the non-negative coder, and everything
// around them is the code that exists: the product tile, the radix selection, the Gram panel, the residual norms, the coder's loop.
//
// THE SELECTION is top_correlations' with one more condition on a candidate.  Kernels, per chunk of signals:
//   tc_launch_record_check / tc_launch_residual_block / tc_launch_dots (topcorr.hip) and coh_launch_norms (coherence.hip): the
//                record check, r_b, dot(i, b) and rn_i of top_correlations — the same kernels, the same words.  No second product.
//   k_nn_select  one workgroup per signal: k_tc_select's statements with another key — the record's columns struck out by index, a
//                column with !(dot > 0) is no candidate, the key is dot * rn_i, tc_select.h's selection (tc_select_sorted).
// ORDER (build flag -ffp-contract=off):
//   candidates   i < n, not stored in record b, rn_i != 0, dot(i, b) > 0: a comparison on the stored word of T — a zero, a negative
//                and a NaN dot fail it, as does the NaN that strikes a stored column out.  Never arithmetic.
//   s(i, b)      = (double)dot * rn_i: one multiplication.  dot > 0 and rn_i > 0, so s >= 0 and its bits order as it does; for such
//                a dot it is the word |dot| * rn_i of top_correlations.
//   coef         = (T)((double)dot * (rn_i * rn_i)): top_correlations' statement.
// CONTRACT: row b of the outputs is a function of (A, y_b, record b, k) alone; the prefix property in k holds (the selection is a
// maximum under a total order: score descending, index ascending).  At n <= SS_HIP_TOPCORR_KMAX the result is the subsequence of
// top_correlations(k = n)'s entries with coef > 0, word for word, padded behind with NONE / 0: the candidates are a subset, a kept
// candidate's key is the same word, and a total order restricted to a subset is the subsequence.  (coef > 0 and dot > 0 name the same
// columns unless dot * rn_i^2 underflows in T.)
//
// THE REFIT is refit.hip's unit with a flag (refit_nonneg): k_rf_check and k_rf_gram as they are — the same partials, the same
// chunk order, the sums over the chunks in double — and k_rf_nnls in k_rf_solve's place: Lawson-Hanson on the normal equations, one
// workgroup per signal, in double, in LDS.  Its order, the entry threshold, the pivot test and the iteration cap are stated once in
// refit.hip's header (NNLS ORDER).  The residual norms are refit_records' (record_residual_norms on the records as written).
// There is no weighted and no grouped non-negative fit: the weighted Gram panel and the group selection would each need their own
// flag through this path (out of scope).
// No floating-point atomics.  Nothing depends on B, on the chunking, on the launch geometry, on where the pointers live or on what
// the context did before.
#include "ss_hip_internal.h"
#include "record_common.h"
#include "tc_select.h"

#include <algorithm>
#include <cmath>

namespace sship {

namespace {

struct NonnegState {
    unsigned char* buf = nullptr;      // per call: inverse norms, staged records and outputs; per chunk: residuals, dots, a host caller's signals
    size_t bytes = 0;
};

NonnegState* state_of(ss_hip_ctx* ctx)
{
    if (!ctx->nn) ctx->nn = new NonnegState();
    return static_cast<NonnegState*>(ctx->nn);
}

__device__ inline float nn_nan(float) { return __int_as_float(0x7fc00000); }
__device__ inline double nn_nan(double) { return __longlong_as_double(0x7ff8000000000000ll); }

// D: the chunk's dots, row b of it is this workgroup's to strike columns out of; rec == nullptr: no records
template <typename T>
__global__ __launch_bounds__(256)
void k_nn_select(T* __restrict__ D, uint32_t n, uint32_t n_pad, const double* __restrict__ rinv, const unsigned char* __restrict__ rec,
                 size_t rb, uint32_t kmax, uint32_t k, uint32_t* __restrict__ oidx, T* __restrict__ ocoef, double* __restrict__ oscore)
{
    __shared__ TcSelectLds lds;
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    T* d = D + (size_t)b * n_pad;
    oidx += (size_t)b * k;
    ocoef += (size_t)b * k;
    oscore += (size_t)b * k;
    if (rec) {
        const unsigned char* r = rec + (size_t)b * rb;
        const uint32_t K = *reinterpret_cast<const uint32_t*>(r);
        if (K > kmax) {                                          // a truncated record does not hold its support: no candidates
            for (uint32_t t = tid; t < k; t += 256u) { oidx[t] = kTcNone; ocoef[t] = T(0); oscore[t] = 0.0; }
            return;
        }
        const uint32_t* idx = reinterpret_cast<const uint32_t*>(r + 16);
        for (uint32_t e = tid; e < K; e += 256u) d[idx[e]] = nn_nan(T(0));        // (idx < n: tc_launch_record_check)
        __threadfence_block();
        __syncthreads();
    }
    // the key of column i, false for a column that is no candidate
    auto keyof = [&](uint32_t i, unsigned long long& key) -> bool {
        const double r = rinv[i];
        if (r == 0.0) return false;
        const T dot = d[i];
        if (!(dot > T(0))) return false;
        const double s = (double)dot * r;
        if (!(s == s)) return false;
        key = (unsigned long long)__double_as_longlong(s);
        return true;
    };
    const uint32_t L = tc_select_sorted(lds, n, k, keyof);
    for (uint32_t t = tid; t < k; t += 256u) {
        if (t < L) {
            const uint32_t i = lds.lidx[t];
            const double r = rinv[i];
            oidx[t] = i;
            ocoef[t] = (T)((double)d[i] * (r * r));
            oscore[t] = __longlong_as_double((long long)lds.lkey[t]);
        } else {
            oidx[t] = kTcNone;
            ocoef[t] = T(0);
            oscore[t] = 0.0;
        }
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------

bool nn_grow(NonnegState* ns, size_t need, const char* who, char* err, size_t errlen)
{
    try {
        grow(ns->buf, ns->bytes, need, "hipMalloc(non-negative top correlations workspace)");
    } catch (const HipFail& f) {
        if (f.code != hipErrorOutOfMemory) throw;
        (void)hipGetLastError();
        set_err(err, errlen, std::string(who) + ": no device memory for a workspace of " + std::to_string(need) + " bytes");
        return false;
    }
    return true;
}

// top_correlations' host side (topcorr.hip: topcorr_impl) with k_nn_select as the selection launch
template <typename T>
int ntop_impl(ss_hip_ctx* ctx, const T* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const void* records, uint32_t kmax, uint32_t k,
              uint32_t* idx, T* coef, double* score, char* err, size_t errlen)
{
    static const char* who = "nonneg_top_correlations";
    HIPCHK(hipSetDevice(ctx->device));
    NonnegState* ns = state_of(ctx);
    hipStream_t st = ctx->stream;
    const size_t m = ctx->m, rb = records ? record_bytes(kmax, sizeof(T)) : 0;
    const uint32_t ldm = ctx->ldm, n = (uint32_t)ctx->n, n_pad = ctx->n_pad, Bu = (uint32_t)B;
    const uint32_t rtiles = (uint32_t)((m + kClsTileRows - 1) / kClsTileRows);
    const bool rec_dev = records && on_device(records), y_dev = on_device(Y);

    // the chunk: whole signal tiles under top_correlations' byte budget
    const size_t per = (size_t)ldm * sizeof(T) + (size_t)n_pad * sizeof(T) + (size_t)rtiles * 4u * sizeof(double) + (y_dev ? 0 : m * sizeof(T));
    size_t chunk = std::max<size_t>(kTcTile, std::min<size_t>(kTcChunkMax, kTcChunkBytes / per) / kTcTile * kTcTile);
    if (ctx->tc_chunk_max > 0) chunk = std::min<size_t>(chunk, (size_t)ctx->tc_chunk_max);
    chunk = std::min(chunk, B);
    const size_t chunk_pad = (chunk + kTcTile - 1) / kTcTile * kTcTile;

    auto carve = [&](unsigned char* base, auto&& use) {
        Carver cv(base);
        double* rinv = cv.take<double>(n_pad);
        uint32_t* bad = cv.take<uint32_t>(1);
        unsigned char* stage = (records && !rec_dev) ? cv.take<unsigned char>(B * rb) : nullptr;
        uint32_t* oi = cv.take<uint32_t>(B * k);
        T* oc = cv.take<T>(B * k);
        double* os = cv.take<double>(B * k);
        T* R = cv.take<T>(chunk_pad * ldm);
        T* D = cv.take<T>(chunk_pad * n_pad);
        double* part = cv.take<double>(chunk * rtiles * 4u);
        T* ybuf = y_dev ? nullptr : cv.take<T>(chunk * m);
        use(rinv, bad, stage, oi, oc, os, R, D, part, ybuf);
        return cv.off;
    };
    if (!nn_grow(ns, carve(nullptr, [](auto...) {}), who, err, errlen)) return SS_HIP_ENOMEM;

    int rc = SS_HIP_OK;
    carve(ns->buf, [&](double* rinv, uint32_t* bad, unsigned char* stage, uint32_t* oi, T* oc, double* os, T* R, T* D, double* part, T* ybuf) {
        const unsigned char* din = static_cast<const unsigned char*>(records);
        if (records) {
            if (!rec_dev) { HIPCHK(hipMemcpyAsync(stage, records, B * rb, hipMemcpyHostToDevice, st)); din = stage; }
            HIPCHK(tc_launch_record_check(ctx, din, rb, kmax, Bu, bad));
            uint32_t first_bad = kTcNone;
            HIPCHK(hipMemcpyAsync(&first_bad, bad, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));            // (nothing has been written when a record is invalid)
            if (first_bad != kTcNone) { rc = bad_index(first_bad, who, err, errlen); return; }
        }
        HIPCHK(coh_launch_norms<T>(ctx, rinv));
        std::vector<T> tmp;
        for (size_t b0 = 0; b0 < B; b0 += chunk) {
            const uint32_t Bc = (uint32_t)std::min(chunk, B - b0);
            const T* yd = Y + (ptrdiff_t)b0 * y_stride;
            long long ys = y_stride, yi = incy;
            if (!y_dev) { upload_rows<T>(ctx, ybuf, Y, y_stride, incy, b0, Bc, tmp); yd = ybuf; ys = (long long)m; yi = 1; }
            HIPCHK(tc_launch_residual_block<T>(ctx, yd, ys, yi, records ? din + b0 * rb : nullptr, rb, kmax, Bc, R, part));
            HIPCHK(tc_launch_dots<T>(ctx, R, Bc, D));
            hipLaunchKernelGGL((k_nn_select<T>), dim3(Bc), dim3(256), 0, st, D, n, n_pad, (const double*)rinv, records ? din + b0 * rb : nullptr, rb,
                               kmax, k, oi + b0 * k, oc + b0 * k, os + b0 * k);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipMemcpyAsync(idx, oi, B * k * sizeof(uint32_t), hipMemcpyDefault, st));
        if (coef) HIPCHK(hipMemcpyAsync(coef, oc, B * k * sizeof(T), hipMemcpyDefault, st));
        if (score) HIPCHK(hipMemcpyAsync(score, os, B * k * sizeof(double), hipMemcpyDefault, st));
        HIPCHK(hipStreamSynchronize(st));
    });
    return rc;
}

// top_correlations' checks in its order
template <typename T>
int ntop_entry(ss_hip_ctx* ctx, const T* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const void* records, uint32_t kmax, uint32_t k,
               uint32_t* idx, T* coef, double* score, char* err, size_t errlen)
{
    static const char* who = "nonneg_top_correlations";
    // (without records kmax is ignored: the checks see a capacity that passes)
    int rc = check_common<T>(ctx, who, records, false, records ? kmax : 1u, err, errlen);
    if (rc != SS_HIP_OK) return rc;
    if (!Y || !idx) { set_err(err, errlen, "nonneg_top_correlations: Y and idx must not be null"); return SS_HIP_EINVAL; }
    if (k == 0 || k > (uint32_t)SS_HIP_TOPCORR_KMAX) {
        set_err(err, errlen, std::string(who) + ": k must be 1.." + std::to_string(SS_HIP_TOPCORR_KMAX));
        return SS_HIP_EINVAL;
    }
    if (incy <= 0 || y_stride <= 0) { set_err(err, errlen, "nonneg_top_correlations: increments and strides must be positive"); return SS_HIP_EINVAL; }
    if (B == 0) return SS_HIP_OK;                             // (every argument above was checked all the same)
    if (B >= 0x80000000ull) { set_err(err, errlen, "nonneg_top_correlations: B must stay below 2^31"); return SS_HIP_EINVAL; }
    return guarded(err, errlen, who, [&] { return ntop_impl<T>(ctx, Y, B, y_stride, incy, records, kmax, k, idx, coef, score, err, errlen); });
}

}  // namespace

void nonneg_free(ss_hip_ctx* ctx)
{
    NonnegState* ns = static_cast<NonnegState*>(ctx->nn);
    if (!ns) return;
    if (ns->buf) (void)hipFree(ns->buf);
    delete ns;
    ctx->nn = nullptr;
}

}  // namespace sship

using namespace sship;

extern "C" {

int ss_hip_nonneg_top_correlations_f32(ss_hip_ctx* ctx, const float* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const void* records,
                                       uint32_t kmax, uint32_t k, uint32_t* idx, float* coef, double* score, char* err, size_t errlen)
{
    return ntop_entry<float>(ctx, Y, B, y_stride, incy, records, kmax, k, idx, coef, score, err, errlen);
}
int ss_hip_nonneg_top_correlations_f64(ss_hip_ctx* ctx, const double* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const void* records,
                                       uint32_t kmax, uint32_t k, uint32_t* idx, double* coef, double* score, char* err, size_t errlen)
{
    return ntop_entry<double>(ctx, Y, B, y_stride, incy, records, kmax, k, idx, coef, score, err, errlen);
}

int ss_hip_nonneg_refit_records_f32(ss_hip_ctx* ctx, const float* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const void* records,
                                    uint32_t kmax, void* records_out, double* resnorm, uint32_t* status, uint32_t* dropped, char* err,
                                    size_t errlen)
{
    return refit_nonneg<float>(ctx, Y, B, y_stride, incy, records, kmax, records_out, resnorm, status, dropped, err, errlen);
}
int ss_hip_nonneg_refit_records_f64(ss_hip_ctx* ctx, const double* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const void* records,
                                    uint32_t kmax, void* records_out, double* resnorm, uint32_t* status, uint32_t* dropped, char* err,
                                    size_t errlen)
{
    return refit_nonneg<double>(ctx, Y, B, y_stride, incy, records, kmax, records_out, resnorm, status, dropped, err, errlen);
}

}  // extern "C"
