// lasso.hip — coding at a penalty the caller names, the fixed-lambda LASSO and the elastic net on compact records (include/ss_hip.h):
//   ss_hip_lasso_refit_records_*.
//
// The greedy record coders stop at a sparsity or a residual; the Homotopy solve walks the whole path and its record is a LASSO
// solution at whatever lambda it ended on.  sparse_encode(..., algorithm = 'lasso_*', alpha = ...), the coding step of l1 dictionary
// learning (Lee et al.; Mairal et al.) and the l1 form of SRC all name ONE lambda for every signal and want
//   min_x 1/2 || y_b - A x ||^2 + lam_b sum_i ||a_i|| |x_i| + 1/2 ridge sum_i ||a_i||^2 x_i^2
// for B signals at once with A and the records on the device.  The working-set coder is three record calls a round:
// top_correlations (its score |a_i . r_b| / ||a_i|| against lam_b is this problem's optimality condition over all n columns),
// extend_records, and this call on the record's columns.
//
// THE CALL is refit.hip's unit with a flag (refit_lasso): k_rf_check and k_rf_gram as they are — the same partials, the same chunk
// order, the sums over the chunks in double — k_rf_cap behind the check as for the non-negative refit, and k_rf_lasso in k_rf_solve's
// place: the non-negative refit's active-set method with a sign and a penalty, one workgroup per signal, in double, in LDS.  Its
// order, the entry threshold, the pivot test and the iteration cap are stated once in refit.hip's header (LASSO ORDER).  The lam_b
// are checked on the device beside the records' indices, before anything is written.  The residual norms are refit_records'
// (record_residual_norms on the records as written).
// There is no non-negative, weighted or grouped LASSO and no lambda path (out of scope).
// No floating-point atomics, no absolute constant.  Nothing depends on B, on the chunking, on the launch geometry, on where the
// pointers live or on what the context did before.
#include "ss_hip_internal.h"

using namespace sship;

extern "C" {

int ss_hip_lasso_refit_records_f32(ss_hip_ctx* ctx, const float* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const void* records,
                                   uint32_t kmax, void* records_out, const double* lam, ptrdiff_t lam_stride, double ridge, double* resnorm,
                                   uint32_t* status, uint32_t* dropped, char* err, size_t errlen)
{
    return refit_lasso<float>(ctx, Y, B, y_stride, incy, records, kmax, records_out, lam, lam_stride, ridge, resnorm, status, dropped, err, errlen);
}
int ss_hip_lasso_refit_records_f64(ss_hip_ctx* ctx, const double* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const void* records,
                                   uint32_t kmax, void* records_out, const double* lam, ptrdiff_t lam_stride, double ridge, double* resnorm,
                                   uint32_t* status, uint32_t* dropped, char* err, size_t errlen)
{
    return refit_lasso<double>(ctx, Y, B, y_stride, incy, records, kmax, records_out, lam, lam_stride, ridge, resnorm, status, dropped, err, errlen);
}

}  // extern "C"
