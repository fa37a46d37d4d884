// pursuit.hip — the backward step of the record coders, a fit that takes atoms out again (include/ss_hip.h):
//   ss_hip_prune_records_*.
//
// Every coder built on the record calls only moves forward: top_correlations -> extend_records -> refit_records, and an atom that
// has entered a record stays.  Subspace pursuit (Dai & Milenkovic), CoSaMP (Needell & Tropp) and OLS with backward elimination
// need the other half: after a merge, keep the `keep` entries that matter and refit on them.  Composed from the calls that exist
// that is two Gram panels a round — a refit on the merged support T, a pick on the host, a refit on the kept support S — and the
// panel is the larger part of a refit.
//
// THE CALL is refit.hip's unit with a flag (refit_prune): k_rf_check and k_rf_gram as they are — the same partials, the same chunk
// order, the sums over the chunks in double — and k_rf_prune in k_rf_solve's place.  A panel element G_ij is one accumulator chain
// over the rows whichever tile holds it, a function of columns i and j and of y alone, so the panel of S is a sub-block of the panel
// of T word for word: one call forms the panel once, solves, scores, selects and solves the sub-block, and what it writes is bit for
// bit what ss_hip_refit_records_* returns for the pruned record.  The scores, the triangular inverse behind the BACKWARD rule, the
// selection and the written record are stated once in refit.hip's header (PRUNE ORDER).  The residual norms are refit_records'
// (record_residual_norms on the records as written).
// There is no weighted, grouped or non-negative pruning (out of scope).
// No floating-point atomics, no absolute constant.  Nothing depends on B, on the chunking, on the launch geometry, on where the
// pointers live or on what the context did before.
#include "ss_hip_internal.h"

using namespace sship;

extern "C" {

int ss_hip_prune_records_f32(ss_hip_ctx* ctx, const float* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const void* records,
                             uint32_t kmax, void* records_out, uint32_t keep, uint32_t rule, double min_share, double* resnorm,
                             uint32_t* status, uint32_t* dropped, double* score, char* err, size_t errlen)
{
    return refit_prune<float>(ctx, Y, B, y_stride, incy, records, kmax, records_out, keep, rule, min_share, resnorm, status, dropped, score, err, errlen);
}
int ss_hip_prune_records_f64(ss_hip_ctx* ctx, const double* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const void* records,
                             uint32_t kmax, void* records_out, uint32_t keep, uint32_t rule, double min_share, double* resnorm,
                             uint32_t* status, uint32_t* dropped, double* score, char* err, size_t errlen)
{
    return refit_prune<double>(ctx, Y, B, y_stride, incy, records, kmax, records_out, keep, rule, min_share, resnorm, status, dropped, score, err, errlen);
}

}  // extern "C"
