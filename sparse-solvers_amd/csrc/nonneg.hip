// nonneg.hip — coding under x >= 0, a fit that only adds atoms (include/ss_hip.h):
//   ss_hip_nonneg_top_correlations_*, ss_hip_nonneg_refit_records_*.
//
// Parts-based dictionaries — training faces or spectra as columns, abundances in unmixing, SRC variants that forbid subtracting one
// subject from another — want min || y_b - A x ||_2 over sparse x >= 0.  The unconstrained coders cannot give it: their selection
// ranks |a_i . r_b| and their refit lets a coefficient take either sign.  Two pieces make the non-negative coder, and everything
// around them is the code that exists: the product tile, the radix selection, the Gram panel, the residual norms, the coder's loop.
//
// THE SELECTION is top_correlations' with one more condition on a candidate: the driver (tc_driver.h), the record check, r_b,
// dot(i, b), rn_i and the selection kernel k_tc_select (tc_select.h) are the shared ones — the same kernels, the same words, no
// second product.  This unit supplies the scorer NnScorer alone: a column with !(dot > 0) is no candidate, the key is dot * rn_i.
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
// There is no weighted and no grouped non-negative fit: the weighted Gram panel would need its own flag through the refit, and the
// selections a scorer of their own (out of scope).
// No floating-point atomics.  Nothing depends on B, on the chunking, on the launch geometry, on where the pointers live or on what
// the context did before.
#include "ss_hip_internal.h"
#include "tc_driver.h"

#include <algorithm>
#include <cmath>

namespace sship {

namespace {

// the non-negative scorer for k_tc_select (tc_select.h): a column with !(dot > 0) is no candidate, s = dot * rn_i
template <typename T> struct NnScorer {
    const double* __restrict__ rinv;
    __device__ const NnScorer& row(uint32_t, uint32_t) const { return *this; }
    __device__ bool key(const T* d, uint32_t i, unsigned long long& key) const
    {
        const double r = rinv[i];
        if (r == 0.0) return false;
        const T dot = d[i];
        if (!(dot > T(0))) return false;
        const double s = (double)dot * r;
        if (!(s == s)) return false;
        key = (unsigned long long)__double_as_longlong(s);
        return true;
    }
    __device__ T coef(const T* d, uint32_t i) const
    {
        const double r = rinv[i];
        return (T)((double)d[i] * (r * r));
    }
};

}  // namespace

}  // namespace sship

using namespace sship;

extern "C" {

int ss_hip_nonneg_top_correlations_f32(ss_hip_ctx* ctx, const float* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const void* records,
                                       uint32_t kmax, uint32_t k, uint32_t* idx, float* coef, double* score, char* err, size_t errlen)
{
    return tc_dots_entry<float, NnScorer<float>>(ctx, { "nonneg_top_correlations", Y, B, y_stride, incy, records, kmax, k, idx, coef, score, err, errlen });
}
int ss_hip_nonneg_top_correlations_f64(ss_hip_ctx* ctx, const double* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const void* records,
                                       uint32_t kmax, uint32_t k, uint32_t* idx, double* coef, double* score, char* err, size_t errlen)
{
    return tc_dots_entry<double, NnScorer<double>>(ctx, { "nonneg_top_correlations", Y, B, y_stride, incy, records, kmax, k, idx, coef, score, err, errlen });
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
