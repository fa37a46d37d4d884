/*
 * ss_hip.h — C-ABI of the MI355X (gfx950) Homotopy l1 hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++ or torch types,
 * no exceptions.  Every entry point returns 0 on success or a non-zero
 * ss_hip_status and writes a NUL-terminated message into `err` (if non-NULL).
 * The C++14 host layer (include/ss/*.h) and the pybind11 module call nothing
 * else; a maintainer of the reference would bind exactly these symbols from a
 * new `op<compute_mode::HIP, T>` specialisation.
 *
 * Citations are file:line under /root/reference.
 *
 * Data pointers (A, y, x, Y, X, r, c) may be HOST or DEVICE pointers; the library
 * asks the HIP runtime which.  The sensing matrix is copied to the device (and
 * re-laid-out column-contiguous) once, at create time — the natural upload point
 * because ss::solver captures A at construction (include/ss/ss.h:98-105).  Later
 * mutation of the caller's A is not observed.
 */
#ifndef SS_HIP_H
#define SS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SS_HIP_ABI_VERSION 7     /* (5: the per-reason counters of round 4; 6: screen_rescued / screen_rescue_tried, the colshard _f64 entry points;
                                    7: the OMP batch entry points and their counters; added under 7 since: the IRLS batch
                                    entry points ss_hip_irls_solve_batch_*, option "irls_batch_max", and the counters
                                    irls_batch_signals / irls_batch_rounds at the end of ss_hip_stats; classification from compact records:
                                    ss_hip_set_classes, ss_hip_reconstruct_records_*, ss_hip_class_residuals_*, ss_hip_homotopy_classify_batch_* —
                                    no new option key, no new field of ss_hip_stats; ss_hip_homotopy_replace_columns_*;
                                    the atom update of dictionary learning, ss_hip_homotopy_atom_update_*, with the test-aid option
                                    "dl_chunk_max" — no new field of ss_hip_stats; the least-squares refit of compact records,
                                    ss_hip_refit_records_* — no new option key, no new field of ss_hip_stats; the sequential atom and
                                    coefficient sweep of K-SVD, ss_hip_homotopy_ksvd_sweep_* — no new option key, no new field of
                                    ss_hip_stats; the top correlations of residuals and the record extension of the stagewise coders,
                                    ss_hip_top_correlations_* and ss_hip_extend_records_*, with the test-aid option "tc_chunk_max" — no
                                    new field of ss_hip_stats; joint sparse coding of signal groups, ss_hip_group_top_correlations_* and
                                    ss_hip_group_class_residuals_* — no new option key, no new field of ss_hip_stats; the atom step of
                                    dictionary learning under row weights, ss_hip_weighted_atom_update_* — no new option key, no new
                                    field of ss_hip_stats; block-sparse coding, the class top correlations
                                    ss_hip_class_top_correlations_* — no new option key, no new field of ss_hip_stats) */

typedef struct ss_hip_ctx ss_hip_ctx;

typedef enum ss_hip_status {
    SS_HIP_OK            = 0,
    SS_HIP_EINVAL        = 1,  /* precondition violated (homotopy-cpu.cpp:193-199 asserts) */
    SS_HIP_ENODEVICE     = 2,  /* no usable HIP device                                     */
    SS_HIP_ERUNTIME      = 3,  /* a HIP runtime call failed (message carries hipGetErrorString) */
    SS_HIP_ENOMEM        = 4,
    SS_HIP_ECAPACITY     = 5,  /* active set outgrew the workspace capacity                */
    SS_HIP_ETYPE         = 6   /* f32 entry point called on an f64 context or vice versa   */
} ss_hip_status;

/* Number of HIP devices visible to this process (0 if none / runtime unusable). */
int ss_hip_device_count(void);

/* "major.minor.patch" of this library; ABI version above. */
const char* ss_hip_version(void);

/*
 * Replaces the state construction of ss::solver<T, homotopy_policy>
 * (include/ss/ss.h:98-105, include/ss/policies.h:42): captures the m x n sensing
 * matrix, element (i,j) at A[i*stride_row + j*stride_col] (strides in ELEMENTS;
 * row-major, padded row-major and column-major views all accepted, the layout
 * rules of src/linalg/blas_wrapper.h:63-94 generalised).
 * Returns NULL on failure (message in err).
 */
ss_hip_ctx* ss_hip_homotopy_create_f32(const float* A, size_t m, size_t n,
                                       ptrdiff_t stride_row, ptrdiff_t stride_col,
                                       int device, char* err, size_t errlen);
ss_hip_ctx* ss_hip_homotopy_create_f64(const double* A, size_t m, size_t n,
                                       ptrdiff_t stride_row, ptrdiff_t stride_col,
                                       int device, char* err, size_t errlen);

void ss_hip_homotopy_destroy(ss_hip_ctx* ctx);

/*
 * Replaces S columns of a live context's dictionary in place (added under ABI version 7): column cols[s] of the m x n
 * matrix becomes V(:, s), element (i, s) at V[i*stride_row + s*stride_col] (strides in ELEMENTS, the layouts create
 * accepts).  cols and V may each be a host or a device pointer (the library asks the runtime which).
 *
 * The call returns when the update is complete; every later call on the context sees the new dictionary, and returns
 * what a context created from the updated matrix with the same options returns — the same words where both take the
 * same route.  Every copy the context derives from A is kept current, not dropped: the column-contiguous copy (padding
 * rows stay zero), the screened forms' fp16 / fp8 copies with their column norms and their two global scales (re-derived
 * from per-column maxima: a new column can raise max |A|, replacing the column that held it can lower it; a whole copy
 * is converted again only when its scale exponent moved; a copy that has not been made yet is not made here), the OMP
 * certificate's norms, and G = A^T A (the tiles that meet a replaced column, formed by the kernel and in the order of
 * the build: bit for bit the G a fresh build forms; not counted in gram_full_builds).  The step-aside windows of the
 * forms, learned on the old dictionary, start again.  Labels (ss_hip_set_classes), options, statistics, the last trace
 * and the workspace stay as they are.
 *
 * Validation happens before anything is written: a failing call leaves the context exactly as it was.
 *   SS_HIP_EINVAL  null ctx, cols or V; an IRLS or a column-sharded context; a column >= n; a column named twice
 *   SS_HIP_ETYPE   the element type of the call is not the context's
 *   S == 0         SS_HIP_OK, nothing touched
 * m and n do not change; columns cannot be appended.
 */
int ss_hip_homotopy_replace_columns_f32(ss_hip_ctx* ctx, const uint32_t* cols, size_t S,
                                        const float* V, ptrdiff_t stride_row, ptrdiff_t stride_col,
                                        char* err, size_t errlen);
int ss_hip_homotopy_replace_columns_f64(ss_hip_ctx* ctx, const uint32_t* cols, size_t S,
                                        const double* V, ptrdiff_t stride_row, ptrdiff_t stride_col,
                                        char* err, size_t errlen);

/*
 * Replaces solve_homotopy::op<compute_mode, T> (src/solvers/homotopy.h:27-38,
 * run_solver src/solvers/homotopy-cpu.cpp:186-275):
 *   min ||x||_1  s.t.  A x = y
 *   y   : m elements, increment incy (elements)
 *   x   : n elements, increment incx; fully overwritten
 *   tol : eps(T) <= tol < 1;   max_iter > 0
 *   iter_out / err_out : ss::homotopy_report{iter, solution_error} (policies.h:25-32)
 */
int ss_hip_homotopy_solve_f32(ss_hip_ctx* ctx, const float* y, ptrdiff_t incy,
                              float tol, uint32_t max_iter,
                              float* x, ptrdiff_t incx,
                              uint32_t* iter_out, double* err_out,
                              char* err, size_t errlen);
int ss_hip_homotopy_solve_f64(ss_hip_ctx* ctx, const double* y, ptrdiff_t incy,
                              double tol, uint32_t max_iter,
                              double* x, ptrdiff_t incx,
                              uint32_t* iter_out, double* err_out,
                              char* err, size_t errlen);

/*
 * Orthogonal matching pursuit on the same context (NOT in the reference, which ships only
 * homotopy and irls: include/ss/ss.h:60-64; BASELINE.json names an `ss::omp` solver).  Greedy:
 *   r = y;  while (iter < max_iter && ||A^T r||_inf > tol) {
 *       idx = argmax |A^T r|;  S += idx;  x_S = argmin ||y - A_S x_S||_2;  r = y - A_S x_S;  }
 * Reuses the correlation sweep (one right-hand side), the arg-max epilogue and the bordered
 * (A_S^T A_S)^-1 of the Homotopy path.  Same argument meaning as ss_hip_homotopy_solve_*;
 * the report is {iterations, ||A^T r||_inf at exit}.
 */
int ss_hip_omp_solve_f32(ss_hip_ctx* ctx, const float* y, ptrdiff_t incy,
                         float tol, uint32_t max_iter, float* x, ptrdiff_t incx,
                         uint32_t* iter_out, double* err_out, char* err, size_t errlen);
int ss_hip_omp_solve_f64(ss_hip_ctx* ctx, const double* y, ptrdiff_t incy,
                         double tol, uint32_t max_iter, double* x, ptrdiff_t incx,
                         uint32_t* iter_out, double* err_out, char* err, size_t errlen);

/*
 * Batch of B signals sharing the context's sensing matrix: signal b is
 * Y[b*y_stride + i*incy], its solution X[b*x_stride + j*incx].
 * iter_out[B], err_out[B] receive the per-signal reports.
 * fp32 batches advance in lock-step on the MFMA units — from "batch_cols_min" (default 24) signals in the column
 * form (per round one pass over the matrix forms the Gram columns of the entering columns), from "batch_gram_min"
 * (default 512) in the Gram form on G = A^T A; where neither applies, from "batch_min" (default 192) the 2B
 * correlation GEMVs of a round become two GEMMs over the shared matrix.  Smaller batches and fp64 run one signal at a
 * time (the single-signal engine, see option "engine").  The lock-step forms agree with the single-signal engine
 * to rounding (same supports and iteration counts), not bit for bit.
 */
int ss_hip_homotopy_solve_batch_f32(ss_hip_ctx* ctx, const float* Y, size_t B,
                                    ptrdiff_t y_stride, ptrdiff_t incy,
                                    float tol, uint32_t max_iter,
                                    float* X, ptrdiff_t x_stride, ptrdiff_t incx,
                                    uint32_t* iter_out, double* err_out,
                                    char* err, size_t errlen);
int ss_hip_homotopy_solve_batch_f64(ss_hip_ctx* ctx, const double* Y, size_t B,
                                    ptrdiff_t y_stride, ptrdiff_t incy,
                                    double tol, uint32_t max_iter,
                                    double* X, ptrdiff_t x_stride, ptrdiff_t incx,
                                    uint32_t* iter_out, double* err_out,
                                    char* err, size_t errlen);

/*
 * The same batch with COMPACT output: one fixed-size record per signal instead of a dense row of n
 * coefficients (4096 signals x 65536 columns are 1 GiB dense, 3 MiB compact) — what a batched caller such
 * as the reference's benchmark driver (src/solvers/homotopy_bench.cpp:39-48) keeps of a solve, and the unit
 * the multi-GPU path gathers (one RCCL all_gather of records, no dense X anywhere).  Record b starts at
 * records + b * ss_hip_record_bytes(kmax, is_f64) and holds, packed on the device from the solver's own
 * support lists (no scan of x):
 *     uint32 K          number of non-zero coefficients of x_b (may exceed kmax: then only the first kmax,
 *                       by column index, are stored)
 *     uint32 iter       homotopy_report::iter        (policies.h:25-32)
 *     double err        homotopy_report::solution_error
 *     uint32 idx[kmax]  their column indices, ascending; unused entries 0
 *     T      val[kmax]  their values; unused entries 0
 * `records` may be a host or a device pointer (B * record_bytes bytes, 8-byte aligned).
 */
size_t ss_hip_record_bytes(uint32_t kmax, int is_f64);
int ss_hip_homotopy_solve_batch_compact_f32(ss_hip_ctx* ctx, const float* Y, size_t B,
                                            ptrdiff_t y_stride, ptrdiff_t incy,
                                            float tol, uint32_t max_iter, uint32_t kmax,
                                            void* records, char* err, size_t errlen);
int ss_hip_homotopy_solve_batch_compact_f64(ss_hip_ctx* ctx, const double* Y, size_t B,
                                            ptrdiff_t y_stride, ptrdiff_t incy,
                                            double tol, uint32_t max_iter, uint32_t kmax,
                                            void* records, char* err, size_t errlen);

/*
 * OMP batch (ABI version 7): B signals sharing the context's sensing matrix, solved by orthogonal matching pursuit
 * (ss_hip_omp_solve_*).  Arguments, record layout and validation are those of the Homotopy batch above
 * (SS_HIP_ETYPE on a dtype mismatch; SS_HIP_EINVAL on an IRLS context, max_iter == 0, a tolerance outside
 * [eps, 1), non-positive increments, null pointers; B == 0 returns SS_HIP_OK).  The report is {iterations, error
 * at exit}.  For a signal a chunk certified, the error is the maximum of |A^T r| over the signal's SUBSET columns at
 * exit (its 448 best-ranked columns in fp32, 256 in fp64), every other column being certified below 15/16 tol (below
 * 7/8 of that maximum where the budget ended the path above tol): it is at most ||A^T r||_inf and can be well below it
 * (a column outside the subset at tol / 2: 1.5e-3 reported against 5e-3).  It is ||A^T r||_inf itself when the signal
 * was solved alone by an engine; the single-signal screened form reports its subset's maximum in the same way.
 * CONTRACT: signal b's result is what ss_hip_omp_solve_* returns for it alone — the same picks, support and
 * iteration count, coefficients equal to rounding; a signal no chunk form certifies is solved alone by the
 * single-signal ladder, and then its result is that solve's bit for bit.
 * (The IRLS batch, ss_hip_irls_solve_batch_* below, is bit for bit for every signal: see there.)
 * Forms, in this order (ss_hip_stats::omp_batch_signals / omp_batch_redone count what the chunks of all of them certify / hand on):
 *   fp32, B >= 4, G = A^T A at hand (option "gram_full_after", or an earlier batch formed it), or B >= max("batch_gram_min", 1536)
 *         and G fits the budget: the Gram form (csrc/ompbatch.hip), chunks of 256 — c0 by the batch GEMM, every signal's path
 *         on its 448 best-ranked columns with their Gram matrix gathered from G, every logged state certified against all
 *         columns by one MFMA pass over the rows of G at the signal's support (omp_gram_signals);
 *   fp32, B >= 4, dictionaries the screened form takes ("batch_screen"): chunks of 64 in the screened form in OMP mode —
 *         the same path on the subset, every state certified by the pass over the fp16 copy (screen_signals / screen_redone);
 *   fp64, B >= 4: the resident tier's batch in OMP mode (screen_signals, screen_resident; screen_tier2 for what it hands on);
 *   everything else (B < 4, a trace requested, engine 3, shapes the forms refuse): one signal at a time, ss_hip_omp_solve_*.
 */
int ss_hip_omp_solve_batch_f32(ss_hip_ctx* ctx, const float* Y, size_t B,
                               ptrdiff_t y_stride, ptrdiff_t incy,
                               float tol, uint32_t max_iter,
                               float* X, ptrdiff_t x_stride, ptrdiff_t incx,
                               uint32_t* iter_out, double* err_out,
                               char* err, size_t errlen);
int ss_hip_omp_solve_batch_f64(ss_hip_ctx* ctx, const double* Y, size_t B,
                               ptrdiff_t y_stride, ptrdiff_t incy,
                               double tol, uint32_t max_iter,
                               double* X, ptrdiff_t x_stride, ptrdiff_t incx,
                               uint32_t* iter_out, double* err_out,
                               char* err, size_t errlen);
int ss_hip_omp_solve_batch_compact_f32(ss_hip_ctx* ctx, const float* Y, size_t B,
                                       ptrdiff_t y_stride, ptrdiff_t incy,
                                       float tol, uint32_t max_iter, uint32_t kmax,
                                       void* records, char* err, size_t errlen);
int ss_hip_omp_solve_batch_compact_f64(ss_hip_ctx* ctx, const double* Y, size_t B,
                                       ptrdiff_t y_stride, ptrdiff_t incy,
                                       double tol, uint32_t max_iter, uint32_t kmax,
                                       void* records, char* err, size_t errlen);

/*
 * Sparse-representation classification from compact records (added under ABI version 7; csrc/classify.hip; NOT in the
 * reference).  The dictionary's columns are training samples grouped by class; a signal coded by l1 minimisation is assigned
 * to the class c whose columns alone reconstruct it best, r_c(y) = ||y - A delta_c(x)||_2, and the sparsity concentration
 * index of x says whether to reject it (Wright et al.; Yang et al., "Fast l1-minimization algorithms for robust face
 * recognition").  The input is the record of ss_hip_homotopy_solve_batch_compact_* / ss_hip_omp_solve_batch_compact_* (same
 * kmax): only the record's columns of A are read — sum K_b * m elements, not m * n per signal.
 * All data pointers may be host or device pointers.  Validation: SS_HIP_EINVAL for a null ctx, records, Y, Yhat or best, an
 * IRLS or column-sharded context, kmax outside 1..4096, records not 8-byte aligned, non-positive increments, r_stride <
 * num_classes, class_residuals / classify before set_classes, a label >= num_classes, a record index >= n (found on the
 * device, never used as an address; the outputs of such a call are unspecified); SS_HIP_ETYPE on a dtype mismatch; B == 0
 * returns SS_HIP_OK and touches nothing.
 * A TRUNCATED record (K > kmax) does not hold its whole solution: best[b] = 0xffffffff, its row of R and sci[b] are NaN, its
 * reconstruction is that of the stored entries, and the call still returns SS_HIP_OK.
 * CONTRACT: signal b's row of R, best[b], sci[b] and row of Yhat are a function of its record, its y, the labels and A —
 * bit for bit the same alone or in any batch, with host or device pointers, whatever the context did before.  Every sum
 * runs in one documented order (csrc/classify.hip): no floating-point atomics, no dependence on B or on the
 * internal chunking.  None of these calls changes what any solve returns.
 */
/* class of every dictionary column: labels[n] (host or device), values < num_classes, num_classes >= 1.
   May be called again to replace them.  Never changes what any solve returns. */
int ss_hip_set_classes(ss_hip_ctx* ctx, const uint32_t* labels, uint32_t num_classes, char* err, size_t errlen);

/* Yhat_b = A x_b for B compact records: row b at Yhat[b*yh_stride + i*incyh], i < m.  The entries are added in the record's
   order (ascending column), in the context's precision.  Needs no classes. */
int ss_hip_reconstruct_records_f32(ss_hip_ctx* ctx, const void* records, size_t B, uint32_t kmax,
                                   float* Yhat, ptrdiff_t yh_stride, ptrdiff_t incyh, char* err, size_t errlen);
int ss_hip_reconstruct_records_f64(ss_hip_ctx* ctx, const void* records, size_t B, uint32_t kmax,
                                   double* Yhat, ptrdiff_t yh_stride, ptrdiff_t incyh, char* err, size_t errlen);

/* R[b*r_stride + c] = ||y_b - A delta_c(x_b)||_2 for c < num_classes (R may be NULL; a class without a stored entry gets
   ||y_b||_2), best[b] = left-most arg-min over c of that row as stored, sci[b] (may be NULL) =
   (C * max_c ||delta_c x||_1 / ||x||_1 - 1) / (C - 1) in double — 0 when x == 0, else 1 when C == 1.
   y_i - (A delta_c x)_i is taken in the context's precision, its square and all sums of squares in double. */
int ss_hip_class_residuals_f32(ss_hip_ctx* ctx, const float* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy,
                               const void* records, uint32_t kmax,
                               float* R, ptrdiff_t r_stride, uint32_t* best, double* sci, char* err, size_t errlen);
int ss_hip_class_residuals_f64(ss_hip_ctx* ctx, const double* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy,
                               const void* records, uint32_t kmax,
                               double* R, ptrdiff_t r_stride, uint32_t* best, double* sci, char* err, size_t errlen);

/* ss_hip_homotopy_solve_batch_compact_* followed by ss_hip_class_residuals_* without leaving the device: a host Y is uploaded
   once, and the records stay in the context's staging when `records` is NULL (otherwise they are also written there: the bytes
   solve_batch_compact returns).  tol / max_iter as for the solve. */
int ss_hip_homotopy_classify_batch_f32(ss_hip_ctx* ctx, const float* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy,
                                       float tol, uint32_t max_iter, uint32_t kmax, void* records,
                                       float* R, ptrdiff_t r_stride, uint32_t* best, double* sci, char* err, size_t errlen);
int ss_hip_homotopy_classify_batch_f64(ss_hip_ctx* ctx, const double* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy,
                                       double tol, uint32_t max_iter, uint32_t kmax, void* records,
                                       double* R, ptrdiff_t r_stride, uint32_t* best, double* sci, char* err, size_t errlen);

/*
 * The atom step of dictionary learning (approximate K-SVD: Rubinstein, Zibulevsky, Elad 2008) from compact records (added under
 * ABI version 7; csrc/dictlearn.hip; NOT in the reference).  Y holds B signals (row b at Y[b*y_stride + i*incy]), `records` their
 * compact records (ss_hip_homotopy_solve_batch_compact_* / ss_hip_omp_solve_batch_compact_*, same kmax), cols[S] the atoms
 * (columns) to update; cols == NULL means all n atoms (S is ignored, V is m x n).  For every requested atom j
 *     r_b = y_b - A x_b                          A x_b accumulated as ss_hip_reconstruct_records_* does, in the context's precision
 *     U_j = the signals that COUNT (K_b <= kmax: the record is not truncated) and whose record holds column j, in ascending b;
 *           w_b = that record's value for j
 *     g_j = sum_{b in U_j} w_b r_b + (sum_{b in U_j} w_b^2) a_j        (= E_j w: the error matrix without atom j's own share)
 *     v_j = g_j / ||g_j||_2
 * and the atom is LEFT AS IT IS (v_j = the stored column, bit for bit) when U_j is empty or ||g_j||_2 is zero or not finite.  All
 * atoms are computed against the same old dictionary and the same residuals (the parallel, Jacobi variant of the sweep: atoms that
 * share signals do not see each other's update; for S = 1 and a unit-norm old atom the objective cannot rise, for several atoms
 * that share signals it can — DESIGN.md §3.13d).  The sequential sweep that re-fits each atom's coefficients, carries the residuals
 * along and cannot raise the objective is ss_hip_homotopy_ksvd_sweep_* below.
 *   V(i, s)    at V[i*stride_row + s*stride_col]; may be NULL when apply != 0
 *   usage[s]   (may be NULL) |U_j|; bit 31 is set when the atom had users but was left as it is
 *   objective  (may be NULL) one double: sum ||r_b||_2^2 over the counting signals, BEFORE the update (a record with K = 0
 *              counts and adds ||y_b||^2)
 *   apply != 0 the atoms that changed (usage in 1 .. 2^31 - 1) are written into the context as
 *              ss_hip_homotopy_replace_columns_* with those columns and those V writes them: the same words in every derived copy
 *              (fp16 / fp8 copies, norms, scales, OMP norms, G), the routing reset; when no atom changed nothing is touched
 * All data pointers may be host or device pointers.
 * CONTRACT: an atom's column of V and its usage are a function of the records, Y, A and the atom alone — bit for bit the same
 * whatever else was requested, with host or device pointers, whatever the context did before.  Every sum runs in one documented
 * order (csrc/dictlearn.hip): no floating-point atomics, no dependence on B, on the internal chunking or on the launch geometry.
 * RANGE: the call has no absolute constant, so a change of units by powers of two (A 2^a, Y 2^b, record values 2^(b-a)) returns the
 * same atoms and usage and the objective times 2^2b, word for word — as long as its intermediates stay normal numbers: sum w_b^2
 * (size 2^(2b-2a)), (sum w_b^2) a_ij and w_b r_b,i (2^(2b-a)) in T, ||g_j||^2 (2^(4b-2a)) and ||r_b||^2 (2^2b) in double.  Outside
 * that range a sum rounds as a subnormal (the atom differs in its last bits) or ||g_j||^2 is 0 or infinite (the atom is left as it
 * is, bit 31 of usage); nothing else goes wrong.  tests/test_gpu_scaling.py holds the call to this.
 * Validation happens before anything is written: a failing call leaves the context and the outputs untouched.
 *   SS_HIP_EINVAL  null ctx, Y or records; V null with apply == 0; an IRLS or a column-sharded context; kmax outside 1..4096;
 *                  records not 8-byte aligned; a non-positive incy, y_stride (for every B, B == 1 included), stride_row or
 *                  stride_col (the two of V only when V is given); a column >= n or named twice in cols; a record
 *                  index >= n (found on the device, never used as an address)
 *   SS_HIP_ETYPE   the element type of the call is not the context's
 *   B == 0, or S == 0 with cols given: SS_HIP_OK, nothing touched — after the checks above that need no data (null pointers, context,
 *                  type, kmax, alignment, increments and strides), which such a call fails like any other
 */
int ss_hip_homotopy_atom_update_f32(ss_hip_ctx* ctx, const float* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy,
                                    const void* records, uint32_t kmax,
                                    const uint32_t* cols, size_t S,
                                    float* V, ptrdiff_t stride_row, ptrdiff_t stride_col,
                                    uint32_t* usage, double* objective, uint32_t apply,
                                    char* err, size_t errlen);
int ss_hip_homotopy_atom_update_f64(ss_hip_ctx* ctx, const double* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy,
                                    const void* records, uint32_t kmax,
                                    const uint32_t* cols, size_t S,
                                    double* V, ptrdiff_t stride_row, ptrdiff_t stride_col,
                                    uint32_t* usage, double* objective, uint32_t apply,
                                    char* err, size_t errlen);

/*
 * The K-SVD sweep: the atoms of cols one after the other, each atom's coefficients re-fitted and the residuals carried along (the
 * sequential atom step of approximate K-SVD; added under ABI version 7; csrc/ksvd.hip; NOT in the reference).  Y, records, kmax,
 * V, usage as for ss_hip_homotopy_atom_update_*; cols[S] names distinct atoms in PROCESSING ORDER (cols == NULL: all n atoms in
 * ascending order, S is ignored, V is m x n); records_out receives the records with the re-fitted values and may be `records`
 * itself (in place) or disjoint from it.  A signal counts when K_b <= kmax.  The working residual starts as r_b = y_b - A x_b (the
 * words of ss_hip_homotopy_atom_update_*) and objective[0] = sum ||r_b||^2 (that call's objective, word for word).  Then for
 * s = 0 .. S - 1, j = cols[s], U_j = the counting signals whose record holds j in ascending b, w_b = the INPUT record's value for j:
 *     sigma = sum w_b^2 (double, ascending b, rounded once to T);  g_i starts at sigma * a_ij and takes w_b * r_b,i in ascending b
 *     (T, one chain per element);  ||g||^2 in double — ss_hip_homotopy_atom_update_*'s order with the CURRENT residuals.
 *     U_j empty, or ||g||_2 zero or not finite: the atom is LEFT AS IT IS — v_j = the stored column bit for bit, no record value and
 *     no residual is touched, usage[s] as in ss_hip_homotopy_atom_update_* (bit 31: had users, left as it is).  Otherwise
 *     v_j,i  = g_i / (T)||g||_2
 *     rho    = sum_i (double)a_ij (double)v_j,i,     t_b = sum_i (double)r_b,i (double)v_j,i for every user (one summation order,
 *              a function of m alone: csrc/ksvd.hip)
 *     w'_b   = (T)(t_b + (double)w_b rho)                                     (row b of E_j^T v_j,  E_j = R_U + a_j w^T)
 *     r_b,i <- (r_b,i + w_b a_ij) - w'_b v_j,i      each product and sum rounded in T, a_ij the STORED column
 *     the output record's value for j becomes w'_b (a value that comes out 0 stays in the record).
 * objective[1] = sum ||r_b||^2 of the final working residuals, in the order of objective[0].  In the output records K, iter, err,
 * idx, the unused tail and every value of an atom not in cols are copied word for word; a truncated record is copied unchanged and
 * adds +0 to both objectives; a record with K = 0 counts.
 * MONOTONE BY CONSTRUCTION: with E = R_U + a w^T the minimiser over the atom for fixed w is E w / ||w||^2, which has the direction
 * of v; w' = E^T v is the minimiser over the coefficients for the unit v.  Hence ||E - v w'^T||_F <= ||E - a w^T||_F whatever the
 * norm of a: no atom step, and therefore no sweep, raises the objective in exact arithmetic; and the output records are the
 * coefficients of the new atoms.
 *   flags      SS_HIP_KSVD_APPLY: after the sweep the atoms that changed (usage in 1 .. 2^31 - 1) are written into the context as
 *              ss_hip_homotopy_replace_columns_* writes them (nothing is touched when no atom changed);
 *              SS_HIP_KSVD_SERIAL: a test aid, an argument of this call only — one atom per level (the plain sequential order)
 *   V          may be NULL;  usage (S words) may be NULL;  objective may be NULL, else it receives TWO doubles: before, after
 * All data pointers may be host or device pointers.
 * SCHEDULE: an atom's step touches only its own users' residuals and record values, so atoms that share no signal commute exactly.
 * The atoms run level by level of that dependency order (level[s] = 1 + the largest level of an earlier atom of cols that shares a
 * signal with s; csrc/ks_levels.h), every level in parallel.  The residual block B * ldm * sizeof(T) of ALL signals is resident.
 * CONTRACT: the outputs are a function of (records, Y, A, cols as an ordered list) alone — bit for bit the same with or without
 * SS_HIP_KSVD_SERIAL, with host or device pointers, in place or out of place, whatever the context did before, whatever the launch
 * geometry.  The columns of V, the usage and the record values of the first S' atoms of cols are those of a call with
 * cols[0 .. S').  For an atom that no earlier atom of cols shares a signal with, the column of V and usage are
 * ss_hip_homotopy_atom_update_*'s words.  No floating-point atomics.  No call changes what any solve returns.
 * RANGE: as for ss_hip_homotopy_atom_update_* — under A 2^a, Y 2^b, record values 2^(b-a) the atoms and usage are the same words, the
 * output values (coefficients of unit atoms) the unscaled ones times 2^b and both objectives times 2^2b, as long as sigma (2^(2b-2a)),
 * sigma a_ij and w_b r_b,i (2^(2b-a)) stay normal numbers of T and ||g||^2 (2^(4b-2a)) of double.
 * Validation happens before anything is written: a failing call leaves the context and every output untouched.
 *   SS_HIP_EINVAL  null ctx, Y, records or records_out; V null without SS_HIP_KSVD_APPLY and usage and objective both null (nothing
 *                  asked for); an IRLS or a column-sharded context; kmax outside 1..4096; records or records_out not 8-byte
 *                  aligned; a partial overlap of records and records_out; a non-positive incy or y_stride, or stride_row /
 *                  stride_col when V is given; an unknown flag bit; a column >= n or named twice in cols; a record index >= n
 *                  (found on the device, never used as an address); a requested atom listed twice in one counting record
 *   SS_HIP_ETYPE   the element type of the call is not the context's
 *   SS_HIP_ENOMEM  the workspace cannot be had (the message names the bytes): the residual block cannot be chunked over the
 *                  signals, because an atom needs all its users at once
 *   B == 0, or S == 0 with cols given: SS_HIP_OK, nothing touched — after the checks above that need no data
 */
#define SS_HIP_KSVD_APPLY  1u   /* write the changed atoms into the context (as ss_hip_homotopy_replace_columns_* does) */
#define SS_HIP_KSVD_SERIAL 2u   /* test aid, an argument of this call only: one atom per level (the plain sequential order) */
int ss_hip_homotopy_ksvd_sweep_f32(ss_hip_ctx* ctx, const float* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy,
                                   const void* records, uint32_t kmax, void* records_out,
                                   const uint32_t* cols, size_t S,
                                   float* V, ptrdiff_t stride_row, ptrdiff_t stride_col,
                                   uint32_t* usage, double* objective, uint32_t flags,
                                   char* err, size_t errlen);
int ss_hip_homotopy_ksvd_sweep_f64(ss_hip_ctx* ctx, const double* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy,
                                   const void* records, uint32_t kmax, void* records_out,
                                   const uint32_t* cols, size_t S,
                                   double* V, ptrdiff_t stride_row, ptrdiff_t stride_col,
                                   uint32_t* usage, double* objective, uint32_t flags,
                                   char* err, size_t errlen);

/*
 * The least-squares refit of compact records on their supports — debiasing (added under ABI version 7; csrc/refit.hip; NOT in the
 * reference).  A Homotopy record holds the LASSO solution at lambda ~ tol: the support is right, every coefficient is shrunk by the
 * l1 penalty (|A_S^T (y - A_S x)| = lambda on the support).  For signal b, with S the record's stored columns in record order and K
 * their number,
 *     records_out[b] = the input record with val[0 .. K) replaced by z = argmin || y_b - A_S z ||_2, rounded once to T;
 *                      K, iter, err, idx and the unused tail are copied word for word; a coefficient that comes out as 0 stays in
 *                      the record; for every status other than SS_HIP_REFIT_DONE the record is copied unchanged
 *     resnorm[b]     (may be NULL) || y_b - A x ||_2 of the record as written to records_out: the words ss_hip_class_residuals_*
 *                      returns in R[b][0] for that record with every column in class 0 (widened to double; NaN for a TRUNCATED
 *                      record, || y_b ||_2 for K = 0)
 *     status[b]      (may be NULL) one of SS_HIP_REFIT_*
 * records_out may be `records` itself (in place) or disjoint from it; any other overlap is undefined.  Y holds the B signals (row b
 * at Y[b*y_stride + i*incy]); all data pointers may be host or device pointers.
 * ARITHMETIC (one documented order: csrc/refit.hip): G = A_S^T A_S and h = A_S^T y are formed together, y as
 * column K of the panel, lower triangle only, products and sums in the context's precision on the matrix cores; the rows are split
 * into chunks of 1024 (a function of m alone), the chunk partials added in double in ascending chunk order; the normal equations
 * are solved in double for both element types by a Cholesky factorisation.  A signal is SS_HIP_REFIT_SINGULAR when for some j
 * !(d_j > 8 K eps(T) G_jj), d_j the j-th pivot before its square root: a column listed twice and an all-zero column always are.
 * The columns are always read from A, never from a resident A^T A.
 * CONTRACT: signal b's output record, resnorm[b] and status[b] are a function of its input record, its y and A alone — bit for bit
 * the same alone or in any batch, in any batch order, with host or device pointers, in place or out of place, across the internal
 * chunking, whatever the context did before.  No floating-point atomics.  No call changes what any solve returns.
 * Validation happens before anything is written: a failing call leaves the outputs untouched.
 *   SS_HIP_EINVAL  null ctx, Y, records or records_out; an IRLS or a column-sharded context; kmax outside 1..4096; records or
 *                  records_out not 8-byte aligned; a non-positive incy or y_stride; a record index >= n (found on the device,
 *                  never used as an address)
 *   SS_HIP_ETYPE   the element type of the call is not the context's
 *   B == 0         SS_HIP_OK, nothing touched — after the checks above that need no data
 */
#define SS_HIP_REFIT_KMAX 160
/* status[b] */
#define SS_HIP_REFIT_DONE 0       /* values replaced by the least-squares fit            */
#define SS_HIP_REFIT_EMPTY 1      /* K == 0: nothing to fit                              */
#define SS_HIP_REFIT_TRUNCATED 2  /* K > kmax: the record does not hold its support      */
#define SS_HIP_REFIT_TOO_LARGE 3  /* kmax >= K > SS_HIP_REFIT_KMAX                       */
#define SS_HIP_REFIT_SINGULAR 4   /* the support's Gram matrix failed the pivot test     */

int ss_hip_refit_records_f32(ss_hip_ctx* ctx, const float* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy,
                             const void* records, uint32_t kmax, void* records_out,
                             double* resnorm, uint32_t* status, char* err, size_t errlen);
int ss_hip_refit_records_f64(ss_hip_ctx* ctx, const double* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy,
                             const void* records, uint32_t kmax, void* records_out,
                             double* resnorm, uint32_t* status, char* err, size_t errlen);

/*
 * The coherence of atoms: for every query atom its largest normalised correlation with any OTHER atom, and which atom that is (added
 * under ABI version 7; csrc/coherence.hip; NOT in the reference).  cols[S] names the query atoms; cols == NULL means all n (S is
 * ignored, the outputs have n entries).  A column may be named more than once: the call reads the context and changes nothing.  For
 * query j = cols[s], with i over the n columns of A,
 *     dot(i, j) = sum_k a_ki a_kj     products and sums in the context's precision on the matrix cores, one accumulator
 *     d_i       = sum_k a_ki^2        in double, formed per call from A (nothing is cached on the context: a column replacement needs
 *                                     no refresh and no stale norm can exist)
 *     s(i, j)   = |dot(i, j)| * (r_i * r_j),  r_i = 1 / sqrt(d_i), in double
 *     mu[s]     = max of s(i, j) over i != j, i not excluded (may be NULL); not clipped: it may exceed 1 by rounding
 *     partner[s] = the smallest i that attains it (may be NULL; mu and partner not both)
 * Column i is EXCLUDED when d_i is 0 or not finite: it is never a partner, and as a query it returns mu = 0, partner =
 * SS_HIP_COHERENCE_NONE — as does every query when no other column is left (n == 1).  Exclusion is by index mask.
 * The queries run in chunks of SS_HIP_COHERENCE_CHUNK against all column tiles (128 x 128 tiles; the workspace holds one (score,
 * index) partial per query of a chunk and column tile, grown on demand, freed with the context).  cols == NULL forms every (i, j) and
 * (j, i): twice the flops of the triangular build of G, for one code path.  G is neither read nor written, resident or not.
 * cols, mu and partner may each be host or device pointers.
 * ARITHMETIC (one documented order: csrc/coherence.hip): |s - s_float64| <= gamma_m + 1e-12 with
 * gamma_m = m u / (1 - m u), u = 2^-24 (fp32) or 2^-53 (fp64).
 * CONTRACT: mu[s] and partner[s] are a function of A and cols[s] alone — bit for bit the same whatever else is in cols, in any
 * order of cols, for cols == NULL, with host or device pointers, across the query chunking, whatever the context did before.  No
 * floating-point atomics.  No call changes what any solve returns.
 * Validation happens before anything is written: a failing call leaves the outputs untouched.
 *   SS_HIP_EINVAL  null ctx; mu and partner both null; an IRLS or a column-sharded context; a column >= n in cols
 *   SS_HIP_ETYPE   the element type of the call is not the context's
 *   S == 0 with cols given: SS_HIP_OK, nothing touched — after the checks above that need no data
 */
#define SS_HIP_COHERENCE_NONE  0xffffffffu
#define SS_HIP_COHERENCE_CHUNK 4096      /* queries per internal pass */
int ss_hip_atom_coherence_f32(ss_hip_ctx* ctx, const uint32_t* cols, size_t S,
                              double* mu, uint32_t* partner, char* err, size_t errlen);
int ss_hip_atom_coherence_f64(ss_hip_ctx* ctx, const uint32_t* cols, size_t S,
                              double* mu, uint32_t* partner, char* err, size_t errlen);

/*
 * The top correlations of residuals: for every signal the k atoms that best explain what its record leaves over (added under ABI
 * version 7; csrc/topcorr.hip; NOT in the reference).  The primitive of the thresholding coder and of stagewise OMP (one stage =
 * this call, ss_hip_extend_records_*, ss_hip_refit_records_*), of nearest-atom retrieval and of residual diagnostics.  Y holds the
 * B signals (row b at Y[b*y_stride + i*incy]); records: B compact records of capacity kmax, or NULL.  For signal b, with i over
 * the n columns of A,
 *     r_b       = y_b - A x_b          the residual of record b: the words of the atom update and of the K-SVD sweep (the chain
 *                                      of ss_hip_reconstruct_records_*, then one subtraction in T); with records == NULL the
 *                                      words of y_b (kmax is ignored)
 *     dot(i, b) = sum_k a_ki r_kb      products and sums in the context's precision on the matrix cores, one accumulator, one
 *                                      chain from 0 over the rows in ascending K-steps: a function of column i, r_b and m alone
 *     d_i       = sum_k a_ki^2         in double, formed per call from A (ss_hip_atom_coherence_*'s words; nothing is cached on the
 *                                      context: a column replacement needs no refresh), rn_i = 1 / sqrt(d_i)
 *     s(i, b)   = |dot(i, b)| * rn_i   in double
 * The CANDIDATES of signal b are the columns i < n with d_i finite and non-zero that record b does not store (exclusion is by
 * index mask, never by arithmetic); a candidate whose score is NaN is never selected.
 *     idx[b][t]   the candidates by descending score, ties by ascending index, t = 0 .. k - 1
 *     score[b][t] (may be NULL) the candidate's score
 *     coef[b][t]  (may be NULL) (T)((double)dot * rn_i^2): the least-squares coefficient of r_b on that atom alone, with its sign
 * Entries beyond the number of candidates are SS_HIP_TOPCORR_NONE in idx and 0 in coef and score; a truncated record (K > kmax)
 * yields such entries throughout.  1 <= k <= SS_HIP_TOPCORR_KMAX.  All data pointers may be host or device pointers.
 * The signals run in chunks under a byte budget, in ascending order (the workspace holds a chunk's residuals, [.][ldm], and dots,
 * [.][n_pad], grown on demand, freed with the context; option "tc_chunk_max").  G = A^T A is neither read nor written, resident or not.
 * ARITHMETIC (one documented order: csrc/topcorr.hip): |s - s_float64| <= (gamma_m + 1e-12) ||r_b||_2 with
 * gamma_m = m u / (1 - m u), u = 2^-24 (fp32) or 2^-53 (fp64), s_float64 formed from the same words of A and r_b.
 * CONTRACT: row b of the outputs is a function of A, y_b, record b and k alone — bit for bit the same alone or in any batch, in any
 * batch order, with host or device pointers, across the chunking, whatever the context did before, with G resident or not; after
 * a column replacement it is a fresh context's result.  PREFIX PROPERTY: the result for k is the first k entries of the result for
 * any larger k.  No floating-point atomics.  No call changes what any solve returns.
 * Validation happens before anything is written: a failing call leaves the outputs untouched.
 *   SS_HIP_EINVAL  null ctx, Y or idx; an IRLS or a column-sharded context; k outside 1..SS_HIP_TOPCORR_KMAX; with records given:
 *                  kmax outside 1..4096, records not 8-byte aligned; a non-positive incy or y_stride; a record index >= n (found
 *                  on the device, never used as an address)
 *   SS_HIP_ETYPE   the element type of the call is not the context's
 *   SS_HIP_ENOMEM  the workspace could not be had (the message carries its bytes)
 *   B == 0         SS_HIP_OK, nothing touched — after the checks above that need no data
 */
#define SS_HIP_TOPCORR_NONE 0xffffffffu
#define SS_HIP_TOPCORR_KMAX 256
int ss_hip_top_correlations_f32(ss_hip_ctx* ctx, const float* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy,
                                const void* records, uint32_t kmax, uint32_t k,
                                uint32_t* idx, float* coef, double* score, char* err, size_t errlen);
int ss_hip_top_correlations_f64(ss_hip_ctx* ctx, const double* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy,
                                const void* records, uint32_t kmax, uint32_t k,
                                uint32_t* idx, double* coef, double* score, char* err, size_t errlen);

/*
 * The record extension: columns named per signal enter its compact record (added under ABI version 7; csrc/topcorr.hip; NOT in the
 * reference).  Integer and copy work only: every word of the output is exactly predictable.  idx [B][k] (the layout
 * ss_hip_top_correlations_* writes), coef [B][k] or NULL.  For signal b, with K the record's count:
 *     the entries idx[b][0 .. k) are taken in order; an entry is skipped when it is SS_HIP_TOPCORR_NONE, when the record already
 *     stores that column, or when an earlier entry of the row was taken for it; taking stops when K reaches kmax;
 *     a taken column c is inserted in front of the first stored entry whose index is larger than c (at the end when there is
 *     none: an ascending idx[] stays ascending), the entries behind it move up by one; its value is coef[b][t], or 0 when coef
 *     is NULL;
 *     records_out[b] = the record so extended: K grown by added[b] (may be NULL), iter, err, the existing indices and values and
 *     the tail behind the last entry word for word;
 *     a truncated record (K > kmax) is copied unchanged, added[b] = 0.
 * records_out may be `records` itself (in place) or disjoint from it.  All data pointers may be host or device pointers.
 * CONTRACT: record b of the output and added[b] are a function of record b and row b of idx and coef alone; no floating-point
 * arithmetic at all.  No call changes what any solve returns.
 * Validation happens before anything is written: a failing call leaves the outputs untouched.
 *   SS_HIP_EINVAL  null ctx, records, idx or records_out; an IRLS or a column-sharded context; kmax outside 1..4096; records or
 *                  records_out not 8-byte aligned, or overlapping in part; k outside 1..SS_HIP_TOPCORR_KMAX; a record index >= n,
 *                  or an entry of idx >= n that is not SS_HIP_TOPCORR_NONE (found on the device, never used as an address)
 *   SS_HIP_ETYPE   the element type of the call is not the context's
 *   B == 0         SS_HIP_OK, nothing touched — after the checks above that need no data
 */
int ss_hip_extend_records_f32(ss_hip_ctx* ctx, const void* records, size_t B, uint32_t kmax,
                              const uint32_t* idx, const float* coef, uint32_t k,
                              void* records_out, uint32_t* added, char* err, size_t errlen);
int ss_hip_extend_records_f64(ss_hip_ctx* ctx, const void* records, size_t B, uint32_t kmax,
                              const uint32_t* idx, const double* coef, uint32_t k,
                              void* records_out, uint32_t* added, char* err, size_t errlen);

/*
 * Joint sparse coding of signal groups — the group top correlations: for every GROUP of signals the k atoms that best explain what
 * the members' records leave over together (added under ABI version 7; csrc/joint.hip; NOT in the reference).  The selection step of
 * simultaneous OMP (the multiple-measurement-vector model): several observations of one subject share one support.  One stage of
 * the joint coder = this call, ss_hip_extend_records_* with a group's idx row for each of its members, ss_hip_refit_records_*.
 * GROUPS are consecutive runs of signals: group g holds the signals group_off[g] .. group_off[g + 1] - 1; group_off [Gn + 1] starts
 * at 0, ascends strictly, ends at B, and no group holds more than SS_HIP_GROUP_MAX signals.  Y, records, kmax, k: as for
 * ss_hip_top_correlations_*, whose r_b, dot(i, b), d_i and rn_i these are (the same kernels on the same rows).  For group g:
 *     q(i, g)   = sum_b (double)dot(i, b) * (double)dot(i, b)    one accumulator from 0, the members in ascending b, every product and
 *                                                               every sum rounded on its own
 *     s(i, g)   = sqrt(q(i, g)) * rn_i                          in double
 * The CANDIDATES of group g are the columns i < n with d_i finite and non-zero that NO member's record stores (exclusion is by
 * index); a candidate whose score is NaN is never selected; a group with a truncated member (K > kmax) has no candidates.
 *     idx[g][t]   the candidates by descending score, ties by ascending index, t = 0 .. k - 1                      [Gn][k]
 *     score[g][t] (may be NULL) the candidate's score                                                             [Gn][k]
 *     coef[b][t]  (may be NULL) (T)((double)dot(idx[g][t], b) * rn^2) for every member b of g: the member's own single-atom
 *                 coefficient, the value ss_hip_extend_records_* takes                                            [B][k]
 * Entries beyond the number of candidates are SS_HIP_TOPCORR_NONE in idx and 0 in coef and score.  All data pointers, group_off
 * among them, may be host or device pointers.  The signals run in chunks of whole groups under ss_hip_top_correlations_*' byte
 * budget (option "tc_chunk_max"; a cap below the largest group is raised to that group's size); the workspace (a chunk's residuals,
 * dots and score rows [.][n_pad] in double) is the context's, grown on demand, freed with it.  G = A^T A is neither read nor written.
 * ARITHMETIC (one documented order: csrc/joint.hip): |s - s_float64| <= (gamma_m + 1e-12) ||R_g||_F, R_g the
 * residuals of the group, gamma_m as for ss_hip_top_correlations_*.
 * CONTRACT: row g of idx and score and the members' rows of coef are a function of A, the group's signals and records in order, and
 * k alone — bit for bit the same alone or in any batch, under any other grouping of the other signals, with host or device pointers,
 * across the chunking, whatever the context did before, with G resident or not; after a column replacement they are a fresh
 * context's result.  PREFIX PROPERTY in k.  No floating-point atomics.  No call changes what any solve returns.
 * A GROUP OF ONE returns ss_hip_top_correlations_*' idx, score and coef words: in fp32 the square of a dot is exact in double, and in
 * either precision sqrt(fl(x * x)) = |x| in binary round-to-nearest — provided x * x neither underflows nor overflows (fp64 only).
 * Validation happens before anything is written: a failing call leaves the outputs untouched.
 *   SS_HIP_EINVAL  ss_hip_top_correlations_*' list, and: a null group_off or Gn == 0 with B > 0; Gn != 0 with B == 0; offsets that do
 *                  not start at 0, do not ascend strictly or do not end at B; a group of more than SS_HIP_GROUP_MAX signals (found on
 *                  the device — k_js_check — never used as an address)
 *   SS_HIP_ETYPE   the element type of the call is not the context's
 *   SS_HIP_ENOMEM  the workspace could not be had (the message carries its bytes)
 *   B == 0         (then Gn == 0) SS_HIP_OK, nothing touched — after the checks above that need no data
 */
#define SS_HIP_GROUP_MAX 256          /* most signals in one group */
int ss_hip_group_top_correlations_f32(ss_hip_ctx* ctx, const float* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy,
                                      const void* records, uint32_t kmax, const uint32_t* group_off, size_t Gn, uint32_t k,
                                      uint32_t* idx, float* coef, double* score, char* err, size_t errlen);
int ss_hip_group_top_correlations_f64(ss_hip_ctx* ctx, const double* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy,
                                      const void* records, uint32_t kmax, const uint32_t* group_off, size_t Gn, uint32_t k,
                                      uint32_t* idx, double* coef, double* score, char* err, size_t errlen);

/*
 * The group class residuals: the class residuals of compact records added up over the members of every group, and the class each
 * group falls to (added under ABI version 7; csrc/joint.hip; NOT in the reference).  Needs ss_hip_set_classes.  Groups: as above.
 * With R[b][c] the words ss_hip_class_residuals_* returns for signal b,
 *     Rg[g][c] = (T)sqrt(sum_b (double)R[b][c] * (double)R[b][c])    one accumulator from 0, the members in ascending b   [Gn] rows of
 *                                                                    rg_stride >= num_classes elements; may be NULL
 *     best[g]  = the left-most arg-min of row g as stored (a NaN is never smaller)                                        [Gn]
 * A group with a truncated member (K > kmax) gets best = 0xffffffff and a NaN row.  A group of one returns
 * ss_hip_class_residuals_*' R row and best word (the proviso above).  The per-signal rows go through ss_hip_class_residuals_*' own
 * path into a workspace of the context, in chunks of whole groups under a fixed byte budget; they are never written to the caller.
 * Row g is a function of A, the labels and the group's signals and records in order.  No floating-point atomics.
 * Validation happens before anything is written: a failing call leaves the outputs untouched.
 *   SS_HIP_EINVAL  ss_hip_class_residuals_*' list (null ctx, Y, records or best; an IRLS or a column-sharded context; kmax outside
 *                  1..4096; records not 8-byte aligned; no classes set; a non-positive incy or y_stride; rg_stride < num_classes with
 *                  Rg given; a record index >= n), and the offset errors of ss_hip_group_top_correlations_*
 *   SS_HIP_ETYPE   the element type of the call is not the context's
 *   SS_HIP_ENOMEM  the workspace could not be had (the message carries its bytes)
 *   B == 0         (then Gn == 0) SS_HIP_OK, nothing touched
 */
int ss_hip_group_class_residuals_f32(ss_hip_ctx* ctx, const float* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy,
                                     const void* records, uint32_t kmax, const uint32_t* group_off, size_t Gn,
                                     float* Rg, ptrdiff_t rg_stride, uint32_t* best, char* err, size_t errlen);
int ss_hip_group_class_residuals_f64(ss_hip_ctx* ctx, const double* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy,
                                     const void* records, uint32_t kmax, const uint32_t* group_off, size_t Gn,
                                     double* Rg, ptrdiff_t rg_stride, uint32_t* best, char* err, size_t errlen);

/*
 * Block-sparse coding — the class top correlations: for every signal the k CLASSES whose atoms together best explain what its record
 * leaves over, and those classes' atoms as whole blocks (added under ABI version 7; csrc/blockcode.hip; NOT in the reference).  The
 * selection step of block OMP (Eldar, Kuppinger and Boelcskei 2010) and of structured SRC (Elhamifar and Vidal 2011): a query in the
 * span of one subject's training samples uses few classes and many atoms of each.  The transpose of the group top correlations:
 * there the norm runs over the signals of a group, here over the atoms of a class.  Needs ss_hip_set_classes.  One stage of the
 * block coder = this call, ss_hip_extend_records_* with its idx and coef rows, ss_hip_refit_records_*.
 * Y, records, kmax, k: as for ss_hip_top_correlations_*, whose r_b, dot(i, b), d_i, rn_i and per-atom score word
 *     t(i, b)   = |dot(i, b)| * rn_i                            in double
 * these are (the same kernels on the same rows).  The CANDIDATE ATOMS of signal b are the columns i < n with d_i finite and non-zero
 * that record b does not store (exclusion is by index, never by a multiplication by zero and never by the value of a dot).  For class c:
 *     q(c, b)   = sum t(i, b) * t(i, b)                         over the candidate atoms of class c: one accumulator from 0, the columns
 *                                                               in ascending index, every product and every sum rounded on its own
 *     s(c, b)   = sqrt(q(c, b))                                 in double
 * A class is a CANDIDATE when it has at least one candidate atom; a class whose score is NaN is never selected; a truncated record
 * (K > kmax) has no candidates.
 *     cls[b][t]   the candidate classes by descending score, ties by ascending class, t = 0 .. k - 1               [B][k]
 *     score[b][t] (may be NULL) the class's score                                                                  [B][k]
 * Entries behind the last candidate are SS_HIP_TOPCORR_NONE in cls and 0 in score.  1 <= k <= SS_HIP_TOPCORR_KMAX.
 * EMISSION — idx [B][width], coef [B][width], taken [B]; idx may be NULL for a ranking-only call (then coef and taken must be NULL
 * and width is ignored); coef and taken may be NULL on their own; 1 <= width <= SS_HIP_TOPCORR_KMAX, so a row is one
 * ss_hip_extend_records_* takes.  room_b = width, with records min(width, kmax - K_b).  The selected classes are taken in rank order:
 * a class is emitted WHOLE — its candidate atoms in ascending index — if they fit what is left of the room, and emission stops at the
 * first class that does not fit (the prefix rule: no later, smaller class jumps the queue).
 *     idx[b][.]   the emitted atoms, class after class                 coef[b][.]  (T)((double)dot * rn_i^2) of each, as for
 *     taken[b]    the number of classes emitted                                    ss_hip_top_correlations_*
 * Behind the last emitted atom the entries are SS_HIP_TOPCORR_NONE / 0.  A class of more than `room` candidate atoms is ranked but
 * never emitted.  All data pointers may be host or device pointers.  The signals run in chunks under ss_hip_top_correlations_*' byte
 * budget (option "tc_chunk_max"), a signal's bytes being that call's plus a class-score row of 8 num_classes; the workspace is the
 * context's, grown on demand, freed with it.  The inverted index of the labels (the columns of every class in ascending order) is built
 * once after each ss_hip_set_classes and kept on the context.  G = A^T A is neither read nor written.
 * ARITHMETIC (one documented order: csrc/blockcode.hip): |s - s_float64| <= (gamma_m + 1e-12) sqrt(L_c) ||r_b||_2,
 * L_c the class's candidate atoms, gamma_m as for ss_hip_top_correlations_*.
 * CONTRACT: row b of every output is a function of A, the labels, y_b, record b, k and width alone — bit for bit the same alone or in
 * any batch, in any batch order, with host or device pointers, across the chunking, whatever the context did before, with G resident
 * or not; after a column replacement or a new ss_hip_set_classes it is a fresh context's result.  PREFIX PROPERTY: cls and score for k
 * are the first k entries of those for any larger k.  No floating-point atomics.  No call changes what any solve returns.
 * SINGLETONS: when every class is a single atom (labels 0 .. n - 1) the call returns ss_hip_top_correlations_*' words — cls = its idx,
 * equal score words and, with width = k, its idx and coef: sqrt(fl(t * t)) = |t| in binary round-to-nearest — provided t * t neither
 * underflows nor overflows (t between 2^-511 and 2^511 is safe).
 * Validation happens before anything is written: a failing call leaves the outputs untouched.
 *   SS_HIP_EINVAL  ss_hip_top_correlations_*' list (cls in the place of idx), and: no classes set; width outside
 *                  1..SS_HIP_TOPCORR_KMAX with idx given; coef or taken given without idx
 *   SS_HIP_ETYPE   the element type of the call is not the context's
 *   SS_HIP_ENOMEM  the workspace could not be had (the message carries its bytes)
 *   B == 0         SS_HIP_OK, nothing touched — after the checks above that need no data
 */
int ss_hip_class_top_correlations_f32(ss_hip_ctx* ctx, const float* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy,
                                      const void* records, uint32_t kmax, uint32_t k, uint32_t width,
                                      uint32_t* cls, double* score, uint32_t* idx, float* coef, uint32_t* taken,
                                      char* err, size_t errlen);
int ss_hip_class_top_correlations_f64(ss_hip_ctx* ctx, const double* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy,
                                      const void* records, uint32_t kmax, uint32_t k, uint32_t width,
                                      uint32_t* cls, double* score, uint32_t* idx, double* coef, uint32_t* taken,
                                      char* err, size_t errlen);

/*
 * Weighted coding — the weighted top correlations: the selection under a non-negative weight per row and signal, the primitive of
 * coding under occlusion, masks of observed rows and robust (IRLS-style) weights: min sum_k w_kb (y_b - A x)_k^2 (added under ABI
 * version 7; csrc/weighted.hip; NOT in the reference).  One stage of the weighted coder = this call, ss_hip_extend_records_*,
 * ss_hip_weighted_refit_records_*.
 * WEIGHTS, common to the three weighted calls: W holds a weight for every row of every signal in the context's element type, row b
 * at W[b*w_stride + k], k < m (unit increment); w_stride == 0 is ONE weight vector shared by all signals (a common mask), else
 * w_stride >= m.  W may be a host or a device pointer.  Every weight must be finite and >= 0: the first offender (the smallest
 * signal, then row) is found on the device before anything is written, and the call returns SS_HIP_EINVAL with both in the message.
 * The padding rows m .. ldm - 1 weigh zero.  A 0/1 mask is the special case.
 * Y, records, kmax, k, idx, coef, score: as for ss_hip_top_correlations_*.  For signal b, with i over the n columns of A,
 *     r_b       = the residual of ss_hip_top_correlations_* (its words);  rw_b = w_b o r_b, one multiplication in T
 *     dot(i, b) = sum_k a_ki rw_kb          ss_hip_top_correlations_*' product on the matrix cores: one accumulator, one chain from 0
 *                                           over the rows in ascending K-steps
 *     d(i, b)   = sum_k w_kb (a_ki a_ki)    the same tile and chain with the operands (w_b, a_i o a_i), a_ki squared once in T: the
 *                                           weighted norm of atom i as signal b sees it
 *     d_i       = sum_k a_ki^2              in double (ss_hip_atom_coherence_*'s words), wmax_b = max_k w_kb
 *     v(i, b)   = d(i, b) / (wmax_b d_i)    in double: the VISIBLE SHARE of atom i for signal b
 *     s(i, b)   = |dot(i, b)| / sqrt(d(i, b))                                               in double
 * The CANDIDATES of signal b are the columns i < n that record b does not store, with d_i finite and non-zero, d(i, b) > 0 and
 * v(i, b) > min_visible (0 <= min_visible < 1); exclusion is by index mask and comparison, never by arithmetic; a candidate whose
 * score is NaN is never selected.  A signal whose weights are all zero has no candidates.
 *     idx[b][t]   the candidates by descending score, ties by ascending index, t = 0 .. k - 1
 *     score[b][t] (may be NULL) the candidate's score
 *     coef[b][t]  (may be NULL) (T)((double)dot / (double)d(i, b)): the weighted least-squares coefficient of r_b on that atom alone
 * Entries beyond the number of candidates are SS_HIP_TOPCORR_NONE in idx and 0 in coef and score; a truncated record (K > kmax)
 * yields such entries throughout.  1 <= k <= SS_HIP_TOPCORR_KMAX.  The signals run in chunks under ss_hip_top_correlations_*' byte
 * budget (option "tc_chunk_max"); the workspace — per chunk the residuals and the weights, [.][ldm] each, and the two dot blocks,
 * [.][n_pad] each; per call a host caller's weights — is the context's, grown on demand, freed with it.
 * ARITHMETIC (one documented order: csrc/weighted.hip): |s - s_float64| <= (2 gamma_{m+1} + 1e-12) ||r_b||_w with
 * ||r||_w = sqrt(sum_k w_k r_k^2), gamma_j = j u / (1 - j u), u = 2^-24 (fp32) or 2^-53 (fp64), s_float64 formed from the same words
 * of A, w_b and r_b.
 * CONTRACT: row b of the outputs is a function of A, y_b, w_b, record b, k and min_visible alone — bit for bit the same alone or in
 * any batch, in any batch order, with host or device pointers, across the chunking, with w_stride == 0 or a W whose rows repeat the
 * vector, whatever the context did before; after a column replacement it is a fresh context's result.  PREFIX PROPERTY in k.  No
 * floating-point atomics.  No call changes what any solve returns.
 * Validation happens before anything is written: a failing call leaves the outputs untouched.
 *   SS_HIP_EINVAL  ss_hip_top_correlations_*' list, and: a null W; a negative w_stride or one in 1 .. m - 1; min_visible outside
 *                  [0, 1); a weight that is negative or not finite (found on the device)
 *   SS_HIP_ETYPE   the element type of the call is not the context's
 *   SS_HIP_ENOMEM  the workspace could not be had (the message carries its bytes)
 *   B == 0         SS_HIP_OK, nothing touched — after the checks above that need no data
 */
int ss_hip_weighted_top_correlations_f32(ss_hip_ctx* ctx, const float* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy,
                                         const float* W, ptrdiff_t w_stride, const void* records, uint32_t kmax,
                                         double min_visible, uint32_t k,
                                         uint32_t* idx, float* coef, double* score, char* err, size_t errlen);
int ss_hip_weighted_top_correlations_f64(ss_hip_ctx* ctx, const double* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy,
                                         const double* W, ptrdiff_t w_stride, const void* records, uint32_t kmax,
                                         double min_visible, uint32_t k,
                                         uint32_t* idx, double* coef, double* score, char* err, size_t errlen);

/*
 * The weighted refit: ss_hip_refit_records_* under the weights above (added under ABI version 7; csrc/weighted.hip, the kernels
 * of csrc/refit.hip with a weight flag; NOT in the reference).  For signal b with the record's stored columns S,
 *     z = argmin sum_k w_kb (y_b - A_S z)_k^2,      the solution of (A_S^T W_b A_S) z = A_S^T W_b y_b, W_b = diag(w_b).
 * The panel, the row chunks of 1024, the tiles, the MFMA instructions and the summation order are ss_hip_refit_records_*'; the weight
 * is applied while the panel is staged: ONE operand of every product is multiplied by w_k in T (not both by sqrt(w_k)), so an
 * element of a chunk partial is the chain of fma(P[r][i] w_r, P[r][j], .).  Then the same solve: Cholesky in double, the same pivot
 * test against the weighted diagonal, the same SS_HIP_REFIT_* status codes (no new ones; a signal whose weights are all zero is
 * SS_HIP_REFIT_SINGULAR, or SS_HIP_REFIT_EMPTY when K == 0).
 *     resnorm[b] (may be NULL) = sqrt(sum_k w_kb (y_b - A x_b)_k^2) of the record as written: the words
 *                ss_hip_weighted_class_residuals_* gives with every column in class 0
 * PINNED: with every weight exactly 1 the output records, status and resnorm are bit for bit those of ss_hip_refit_records_*; with a
 * 0/1 mask they are those of ss_hip_refit_records_* on a context created from diag(w) A with the signals w o y.
 * CONTRACT and validation: as for ss_hip_refit_records_*, with w_b among what a signal's words are a function of (w_stride == 0 or
 * repeated rows: the same words), and
 *   SS_HIP_EINVAL  a null W; a negative w_stride or one in 1 .. m - 1; a weight that is negative or not finite
 */
int ss_hip_weighted_refit_records_f32(ss_hip_ctx* ctx, const float* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy,
                                      const float* W, ptrdiff_t w_stride, const void* records, uint32_t kmax,
                                      void* records_out, double* resnorm, uint32_t* status, char* err, size_t errlen);
int ss_hip_weighted_refit_records_f64(ss_hip_ctx* ctx, const double* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy,
                                      const double* W, ptrdiff_t w_stride, const void* records, uint32_t kmax,
                                      void* records_out, double* resnorm, uint32_t* status, char* err, size_t errlen);

/*
 * The weighted class residuals: ss_hip_class_residuals_* under the weights above (added under ABI version 7; csrc/weighted.hip, the
 * kernels of csrc/classify.hip with a weight flag; NOT in the reference).  Needs ss_hip_set_classes.
 *     R[b*r_stride + c] = sqrt(sum_k w_kb (y_b - A delta_c(x_b))_k^2)    (a class without a stored entry gets ||y_b||_w)
 * d_k = y_k - (A delta_c x)_k in the context's precision as in the unweighted call, its square in double, multiplied by (double)w_kb
 * before it enters the unweighted call's sums, in their order.  best[b] and sci[b] are formed as in the unweighted call; sci
 * depends on the record alone.  A class none of whose rows is visible reads 0 like any other (and may win the arg-min: the caller
 * who masks everything has asked for it).
 * PINNED: with every weight exactly 1 every output word equals ss_hip_class_residuals_*'s; with a 0/1 mask, that call's words on a
 * context created from diag(w) A with the signals w o y.
 * CONTRACT and validation: as for ss_hip_class_residuals_*, with w_b among what a signal's words are a function of, and
 *   SS_HIP_EINVAL  a null W; a negative w_stride or one in 1 .. m - 1; a weight that is negative or not finite
 */
int ss_hip_weighted_class_residuals_f32(ss_hip_ctx* ctx, const float* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy,
                                        const float* W, ptrdiff_t w_stride, const void* records, uint32_t kmax,
                                        float* R, ptrdiff_t r_stride, uint32_t* best, double* sci, char* err, size_t errlen);
int ss_hip_weighted_class_residuals_f64(ss_hip_ctx* ctx, const double* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy,
                                        const double* W, ptrdiff_t w_stride, const void* records, uint32_t kmax,
                                        double* R, ptrdiff_t r_stride, uint32_t* best, double* sci, char* err, size_t errlen);

/*
 * The weighted atom update: the atom step of dictionary learning under the weights above — learning from masked, occluded or
 * robustly weighted signals, min sum_b sum_k w_kb (y_b - A x_b)_k^2 over the atoms (added under ABI version 7; csrc/wdictlearn.hip;
 * NOT in the reference).  ss_hip_homotopy_atom_update_* on zero-filled signals fits the atoms to the zeros; its chains cannot be had
 * by scaling Y, because the weights differ per signal while the atom is shared.
 * Y, records, kmax, cols, S, V, usage: as for ss_hip_homotopy_atom_update_* (cols == NULL: all n atoms; a truncated record does not
 * count; host or device pointers).  W, w_stride: the WEIGHTS of the weighted calls above.  For every requested atom j, with U_j the
 * counting signals whose record holds j in ascending (b, position in the record), c_b that record's value and r_b = y_b - A x_b the
 * UNWEIGHTED residual (ss_hip_homotopy_atom_update_*'s words):
 *     num_k = sum_{b in U_j} (w_kb c_b) r_kb       den_k = sum_{b in U_j} (w_kb c_b) c_b       row k is SEEN when den_k > 0
 *     d_k   = a_kj + num_k / den_k  (seen)         d_k = a_kj  (not seen: no user observes the row, it carries no information)
 *     nu    = ||d||_2                              v_j = d / nu
 *     records_out: the value c_b of atom j in every counting record becomes c_b * nu
 * t = w_kb * c_b is rounded once in T, then num += t * r_kb and den += t * c_b, every product and sum rounded separately in T, one
 * user after the other in list order, one chain per row, never split; d_k: one division, one addition, the comparison den_k > 0 (no
 * arithmetic masks); ||d||^2 in double in ss_hip_homotopy_atom_update_*'s order; nu = (T) sqrt; v = d / nu; c_b * nu one product in T.
 * The atom is LEFT AS IT IS — V holds the stored column bit for bit and no record value is touched — when U_j is empty, when no row
 * is seen, or when nu is zero or not finite; bit 31 of usage is set in the last two cases.  All atoms see the same old dictionary
 * and residuals (the Jacobi step).  d is the row-wise weighted least-squares minimiser over the atom for fixed c, and the values are
 * rescaled so that v_j c'_b = d c_b: hence, in exact arithmetic, a call whose atoms share no signal (S = 1 in particular) cannot
 * raise sum_b sum_k w_kb (y_b - A x_b)_k^2, whatever the old atom's norm.  Atoms that share signals do not see each other's update.
 *   records_out  (may be NULL) B records: `records` itself (in place) or disjoint from it; every other word of a record — K, iter,
 *                err, idx, the tail, the values of atoms not requested or left as they are, truncated records — is copied word
 *                for word
 *   objective    (may be NULL) one double: sum_b sum_k w_kb r_kb^2 over the counting signals BEFORE the update: every square formed
 *                in double and multiplied by (double) w_kb before it enters ss_hip_homotopy_atom_update_*'s sums, in their order
 *   flags        SS_HIP_WDL_APPLY: the atoms that changed are written into the context as ss_hip_homotopy_atom_update_*'s apply
 *                writes them; when no atom changed nothing is touched
 * PINNED: with every weight exactly 1 objective and usage are ss_hip_homotopy_atom_update_*'s words; V agrees with that call's only
 * to rounding (it starts its chain at (sum c^2) a_j with sum c^2 in double; here den is a chain in T per row).  With a 0/1 mask the
 * hidden entries of Y are never read into a result.
 * CONTRACT: as for ss_hip_homotopy_atom_update_*, with w_b among what the words are a function of: the same words alone or among
 * other atoms, with host or device pointers, across the internal chunking (option "dl_chunk_max"), with w_stride == 0 or a W whose
 * rows repeat the vector, in place or out of place, whatever the context did before.  No floating-point atomics.
 * RANGE: under A 2^a, Y 2^b, record values 2^(b-a), W 2^c the call returns the same changed atoms and usage (an atom that is left
 * is the stored column, in the context's units), nu times 2^a — so the values of changed atoms in records_out are the unscaled
 * call's times 2^b — and the objective times 2^(2b+c), word for word, as long as the intermediates stay normal numbers: w c (2^(c+b-a)), its products with r and c (2^(c+2b-a), 2^(c+2b-2a)) and the quotient in T,
 * ||d||^2 and the squares in double.
 * Validation happens before anything is written: a failing call leaves the context and the outputs untouched.
 *   SS_HIP_EINVAL  ss_hip_homotopy_atom_update_*'s list (V may be null with or without SS_HIP_WDL_APPLY); the weighted calls' list
 *                  (a null W; a negative w_stride or one in 1 .. m - 1; a weight that is negative or not finite, with its signal
 *                  and row); an unknown flag bit; records_out not 8-byte aligned or overlapping records in part; V, usage,
 *                  objective and records_out all null without SS_HIP_WDL_APPLY (nothing was asked for)
 *   SS_HIP_ETYPE   the element type of the call is not the context's
 *   B == 0, or S == 0 with cols given: SS_HIP_OK, nothing touched — after the checks above that need no data
 */
#define SS_HIP_WDL_APPLY 1u
int ss_hip_weighted_atom_update_f32(ss_hip_ctx* ctx, const float* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy,
                                    const float* W, ptrdiff_t w_stride, const void* records, uint32_t kmax, void* records_out,
                                    const uint32_t* cols, size_t S,
                                    float* V, ptrdiff_t stride_row, ptrdiff_t stride_col,
                                    uint32_t* usage, double* objective, uint32_t flags, char* err, size_t errlen);
int ss_hip_weighted_atom_update_f64(ss_hip_ctx* ctx, const double* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy,
                                    const double* W, ptrdiff_t w_stride, const void* records, uint32_t kmax, void* records_out,
                                    const uint32_t* cols, size_t S,
                                    double* V, ptrdiff_t stride_row, ptrdiff_t stride_col,
                                    uint32_t* usage, double* objective, uint32_t flags, char* err, size_t errlen);

/*
 * Robust coding — row weights from record residuals: the step between two codings of a robust (IRLS-style) coder, on the device
 * (added under ABI version 7; csrc/robust.hip; NOT in the reference).  The weighted calls above take the weights of a caller who
 * knows which rows to distrust; this call makes them for corruption at unknown rows (a scarf, a saturated block, a dead channel)
 * from what the last coding left over.  A stays on the device and only the records' columns are read.  A robust coder runs
 * ss_hip_robust_weights_* without records (r = y), codes under W_out with the weighted calls, and repeats from those records.
 * Y, records, kmax: as for ss_hip_top_correlations_* (records == NULL: r_b = the words of y_b, kmax is ignored).  W, w_stride: PRIOR
 * weights in the layout of the weighted calls (a known mask, a confidence; w_stride == 0: one vector for all signals), or W == NULL:
 * every prior weight 1 and w_stride ignored.  Every pointer may be a host or a device pointer.  For signal b, with k over the rows
 * 0 .. m - 1 only (the padding rows m .. ldm - 1 take no part anywhere):
 *     r_kb      = the residual of ss_hip_top_correlations_*, word for word
 *     VISIBLE   a row whose prior weight is > 0 and whose r_kb is finite; v = the number of visible rows
 *     med_b     = the element of rank (v - 1) / 2 (integer division), 0-based and ascending, of |r_kb| over the visible rows: a
 *                 stored word, found by an exact selection on its bits without arithmetic; 0 for v == 0
 *     sigma_b   = max(1.4826022185056018 * (double)med_b, sigma_min), then t = tuning * sigma_b: one operation in double each
 *     f_kb      with a = |(double)r_kb|, decided by comparisons first: 0 for a row that is not visible, else
 *                 SS_HIP_ROBUST_HUBER   a <= t -> 1, else (T)(t / a)
 *                 SS_HIP_ROBUST_TUKEY   a == 0 -> 1; a < t -> u = a / t, q = 1 - u * u, (T)(q * q); else 0
 *                 SS_HIP_ROBUST_CUTOFF  a <= t -> 1, else 0
 *     W_out[b*wo_stride + k] = f_kb * prior_kb, one multiplication in T (f_kb itself for W == NULL)
 *     resid[b*r_stride + k]  (may be NULL) = r_kb
 *     scale[b]               (may be NULL) = sigma_b
 * The scale is about zero, not about the median: the residual of a fit has no location of its own.  sigma_b == 0 (more than half of
 * the residuals exactly zero and sigma_min == 0) gives 1 on the rows that are exactly zero and 0 elsewhere; no NaN is ever produced.
 * A TRUNCATED record (K > kmax) does not hold its support: its W_out row is the prior's words (1 without a prior), its resid row is
 * 0 and scale[b] is NaN.  The usual tunings are 1.345 (Huber), 4.685 (Tukey) and 2.5 (cutoff).  The signals run in chunks under
 * ss_hip_top_correlations_*' byte budget (option "tc_chunk_max"); the workspace — per chunk the residuals [.][ldm], a host caller's
 * signals and rows of the outputs — is the context's, grown on demand, freed with it.
 * CONTRACT: row b of every output is a function of A, y_b, prior_b, record b, loss, tuning and sigma_min alone — bit for bit the
 * same alone or in any batch, in any batch order, with host or device pointers, across the chunking, with w_stride == 0 or a W whose
 * rows repeat the vector, whatever the context did before; after a column replacement it is a fresh context's result.  No
 * floating-point atomics.  No call changes what any solve returns.
 * Validation happens before anything is written: a failing call leaves W_out, resid and scale untouched.
 *   SS_HIP_EINVAL  null ctx, Y or W_out; an IRLS or column-sharded context; with records: kmax outside 1 .. 4096, records not 8-byte
 *                  aligned, a stored column index >= n (found on the device); non-positive incy or y_stride; wo_stride < m, or
 *                  r_stride < m with resid given; with W: a negative w_stride or one in 1 .. m - 1, a weight that is negative or
 *                  not finite (found on the device, with its signal and row); loss > 2; tuning not finite or <= 0; sigma_min not
 *                  finite or < 0; W_out == W
 *   SS_HIP_ETYPE   the element type of the call is not the context's
 *   SS_HIP_ENOMEM  the workspace could not be had (the message carries its bytes)
 *   B == 0         SS_HIP_OK, nothing touched — after the checks above that need no data
 */
#define SS_HIP_ROBUST_HUBER  0u
#define SS_HIP_ROBUST_TUKEY  1u
#define SS_HIP_ROBUST_CUTOFF 2u
int ss_hip_robust_weights_f32(ss_hip_ctx* ctx, const float* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy,
                              const float* W, ptrdiff_t w_stride, const void* records, uint32_t kmax,
                              uint32_t loss, double tuning, double sigma_min,
                              float* W_out, ptrdiff_t wo_stride, float* resid, ptrdiff_t r_stride, double* scale,
                              char* err, size_t errlen);
int ss_hip_robust_weights_f64(ss_hip_ctx* ctx, const double* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy,
                              const double* W, ptrdiff_t w_stride, const void* records, uint32_t kmax,
                              uint32_t loss, double tuning, double sigma_min,
                              double* W_out, ptrdiff_t wo_stride, double* resid, ptrdiff_t r_stride, double* scale,
                              char* err, size_t errlen);

/*
 * Non-negative coding — the positive top correlations: ss_hip_top_correlations_* restricted to the atoms that a fit may ADD (added
 * under ABI version 7; csrc/nonneg.hip; NOT in the reference).  Dictionaries whose atoms are parts — training faces or spectra as
 * columns, abundances in unmixing, SRC variants that forbid subtracting one subject from another — want a code with x >= 0.  One
 * stage of the non-negative coder = this call, ss_hip_extend_records_*, ss_hip_nonneg_refit_records_*.  The parameter list, r_b,
 * dot(i, b), d_i and rn_i are ss_hip_top_correlations_*' (the same kernels through the same launches), and
 *     CANDIDATES  that call's candidates with dot(i, b) > 0: a comparison on the stored word, never arithmetic — a zero, a
 *                 negative and a NaN dot are no candidates
 *     s(i, b)     = dot(i, b) * rn_i in double (positive: its bits order as it does); ties by ascending index
 *     coef[b][t]  (may be NULL) (T)((double)dot * rn_i^2)
 * Entries beyond the number of candidates are SS_HIP_TOPCORR_NONE in idx and 0 in coef and score.
 * CONTRACT: row b of the outputs is a function of A, y_b, record b and k alone, as for ss_hip_top_correlations_*; the PREFIX PROPERTY
 * in k holds.  PINNED: at n <= SS_HIP_TOPCORR_KMAX the result is the subsequence of ss_hip_top_correlations_*(k = n)'s entries with
 * coef > 0, word for word in idx, coef and score, padded behind with SS_HIP_TOPCORR_NONE / 0.
 * Validation, workspace and error codes: as for ss_hip_top_correlations_*.
 */
int ss_hip_nonneg_top_correlations_f32(ss_hip_ctx* ctx, const float* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy,
                                       const void* records, uint32_t kmax, uint32_t k,
                                       uint32_t* idx, float* coef, double* score, char* err, size_t errlen);
int ss_hip_nonneg_top_correlations_f64(ss_hip_ctx* ctx, const double* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy,
                                       const void* records, uint32_t kmax, uint32_t k,
                                       uint32_t* idx, double* coef, double* score, char* err, size_t errlen);

/*
 * The non-negative refit: ss_hip_refit_records_* under z >= 0 (added under ABI version 7; csrc/nonneg.hip, the kernels of
 * csrc/refit.hip with the solve replaced; NOT in the reference).  For signal b with the record's stored columns S, K of them,
 *     z = argmin || y_b - A_S z ||_2  subject to  z >= 0.
 * G = A_S^T A_S, h = A_S^T y_b and y^T y are ss_hip_refit_records_*' words (the same panel, row chunks, tiles and summation
 * order).  On them one workgroup per signal runs the Lawson-Hanson active-set method in double, in LDS, in one documented order
 * (csrc/refit.hip, NNLS ORDER): from P empty and z = 0, the column outside P with the largest w_j = (h - G z)_j
 * among those with w_j > tau_j = 8 K eps(T) sqrt(G_jj y^T y) enters (ties to the smallest record position; none: done); G_PP s = h_P
 * is solved by a Cholesky factor that gains a row on entry and is formed again after a removal; while some s_i <= 0, z moves towards
 * s as far as it stays non-negative and what reaches zero leaves P.  At most 3 K solves a signal.
 *     records_out[b]  for SS_HIP_REFIT_DONE: the entries with (T) z_e > 0, in record order, compacted — K' of them, K' in word 0,
 *                     idx[0 .. K') and val[0 .. K') theirs, idx[K' .. K) and val[K' .. K) zero words; iter, err, the slots behind
 *                     K and the padding copied word for word.  K' = 0 is a valid result.  For every other status the record is
 *                     copied unchanged
 *     resnorm[b]      (may be NULL) as for ss_hip_refit_records_*, of the record as written
 *     status[b]       (may be NULL) SS_HIP_REFIT_*: EMPTY and TRUNCATED as there; SS_HIP_REFIT_TOO_LARGE for kmax >= K >
 *                     SS_HIP_NNLS_KMAX; SS_HIP_REFIT_SINGULAR when a column that passed the entry test fails the pivot test
 *                     !(d > 8 K eps(T) G_jj), or when y^T y, an h_j or a G_jj is not finite; SS_HIP_REFIT_STALLED past the cap
 *     dropped[b]      (may be NULL) K - K' for SS_HIP_REFIT_DONE, else 0
 * A column named twice and an all-zero column never pass the entry test: they are dropped, not SINGULAR.
 * SS_HIP_NNLS_KMAX is 128: G and the factor, two packed triangles in double, share one CU's 160 KiB of LDS; the request is sized
 * from min(kmax, SS_HIP_NNLS_KMAX) (kmax = 96: two workgroups a CU).
 * CONTRACT and validation: as for ss_hip_refit_records_*, dropped[b] among a signal's words.
 */
#define SS_HIP_NNLS_KMAX 128
#define SS_HIP_REFIT_STALLED 5    /* the non-negative refit needed more than 3 K solves    */
int ss_hip_nonneg_refit_records_f32(ss_hip_ctx* ctx, const float* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy,
                                    const void* records, uint32_t kmax, void* records_out,
                                    double* resnorm, uint32_t* status, uint32_t* dropped, char* err, size_t errlen);
int ss_hip_nonneg_refit_records_f64(ss_hip_ctx* ctx, const double* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy,
                                    const void* records, uint32_t kmax, void* records_out,
                                    double* resnorm, uint32_t* status, uint32_t* dropped, char* err, size_t errlen);

/*
 * The backward step — pruning compact records: ss_hip_refit_records_* that takes atoms out again (added under ABI version 7;
 * csrc/pursuit.hip, the kernels of csrc/refit.hip with the solve replaced; NOT in the reference).  Every record coder only adds
 * atoms; subspace pursuit, CoSaMP and OLS with backward elimination also remove them.  One round of subspace pursuit =
 * ss_hip_top_correlations_*, ss_hip_extend_records_*, this call.  For signal b with the record's stored columns T in record order,
 * K of them: G = A_T^T A_T, h = A_T^T y_b and yy = y_b^T y_b are ss_hip_refit_records_*' words (the same panel, row chunks, tiles and
 * summation order), z its solution in double before rounding (the same Cholesky statements, pivot test and back substitution), and
 *     score_e     in double, every product, sum and quotient rounded separately (csrc/refit.hip, PRUNE ORDER):
 *                 SS_HIP_PRUNE_MAGNITUDE  (z_e * z_e) * G_ee — the energy of the atom's own term;
 *                 SS_HIP_PRUNE_BACKWARD   (z_e * z_e) / q_e with q_e = ((G_T)^-1)_ee = sum over i >= e of ((L^-1)_ie)^2 — exactly the
 *                 rise of || y - A_T z ||^2 when atom e alone is removed and the rest refitted.  The rules agree for orthogonal atoms
 *     CANDIDATES  the entries with score_e >= min_share * yy: a comparison, so a NaN never passes
 *     KEPT        the min(keep, candidates) candidates that come first under the total order (score descending, record position
 *                 ascending)
 *     records_out[b]  for SS_HIP_REFIT_DONE: every entry kept: ss_hip_refit_records_*' output record.  Otherwise the normal equations
 *                     of the kept sub-block — the same panel words, summed again from the chunk partials — are solved by the same
 *                     statements in the same order with K' in the pivot test, and the record is written as
 *                     ss_hip_nonneg_refit_records_* writes its record: the kept entries in record order, compacted — K' of them, K'
 *                     in word 0, idx[0 .. K') and val[0 .. K') theirs (each z rounded once to T), idx[K' .. K) and val[K' .. K) zero
 *                     words; iter, err, the slots behind K and the padding copied word for word.  K' = 0 is a valid result.  The
 *                     record is bit for bit what ss_hip_refit_records_* returns for the kept record.  For every other status the
 *                     record is copied unchanged
 *     resnorm[b]      (may be NULL) as for ss_hip_refit_records_*, of the record as written
 *     status[b]       (may be NULL) SS_HIP_REFIT_*: EMPTY, TRUNCATED and TOO_LARGE (K > SS_HIP_REFIT_KMAX) as there;
 *                     SS_HIP_REFIT_SINGULAR when either solve fails the pivot test; else SS_HIP_REFIT_DONE
 *     dropped[b]      (may be NULL) K - K' for SS_HIP_REFIT_DONE, else 0
 *     score[b][e]     (may be NULL; [B][kmax] doubles) score_e by INPUT position for e < K, 0 behind it; a zero row for a status
 *                     other than SS_HIP_REFIT_DONE
 * keep >= 1; rule one of SS_HIP_PRUNE_*; min_share >= 0 and finite.  A NaN in y_b gives NaN scores: K' = 0, SS_HIP_REFIT_DONE, a NaN
 * resnorm.  Y, records, records_out and the four outputs: host or device pointers; records_out may be records (in place).
 * CONTRACT: signal b's outputs are a function of (record b, y_b, A, keep, rule, min_share) alone — bit for bit the same alone or in
 * any batch, in any batch order, with host or device pointers, in place or out of place, across the internal chunking, and whatever
 * the context did before.  No floating-point atomics.  No absolute constant: under A * 2^a, Y * 2^b and record values * 2^(b - a)
 * the kept sets are the same, the values scale by 2^(b - a) and the scores by 2^(2 b).  No option key, no field of ss_hip_stats.
 * Validation: ss_hip_refit_records_*', then SS_HIP_EINVAL for keep = 0, an unknown rule, a negative or non-finite min_share — all
 * before anything is written.  B = 0 is SS_HIP_OK.
 */
#define SS_HIP_PRUNE_MAGNITUDE 0
#define SS_HIP_PRUNE_BACKWARD 1
int ss_hip_prune_records_f32(ss_hip_ctx* ctx, const float* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy,
                             const void* records, uint32_t kmax, void* records_out,
                             uint32_t keep, uint32_t rule, double min_share,
                             double* resnorm, uint32_t* status, uint32_t* dropped, double* score, char* err, size_t errlen);
int ss_hip_prune_records_f64(ss_hip_ctx* ctx, const double* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy,
                             const void* records, uint32_t kmax, void* records_out,
                             uint32_t keep, uint32_t rule, double min_share,
                             double* resnorm, uint32_t* status, uint32_t* dropped, double* score, char* err, size_t errlen);

/*
 * Fixed-penalty LASSO and elastic-net coding — the l1 refit: ss_hip_refit_records_* under a penalty the caller names (added under
 * ABI version 7; csrc/lasso.hip, the kernels of csrc/refit.hip with the solve replaced; NOT in the reference).  The greedy coders
 * stop at a sparsity or a residual and the Homotopy solve ends on whatever lambda its tolerance reaches; sparse_encode(...,
 * alpha = ...), the coding step of l1 dictionary learning and the l1 form of SRC name ONE lambda for all signals.  For signal b
 * with the record's stored columns S in record order, K of them, G = A_S^T A_S, h = A_S^T y_b and yy = y_b^T y_b are
 * ss_hip_refit_records_*' words (the same check, panel, row chunks, tiles and summation order), g_e = sqrt(G_ee), and the call solves
 *     z = argmin  1/2 z^T (G + ridge diag G) z - h^T z + lam_b sum_e g_e |z_e|
 * — min 1/2 || y_b - A_S z ||^2 + lam_b sum_e ||a_e|| |z_e| + 1/2 ridge sum_e ||a_e||^2 z_e^2: the norm-weighted penalty is the
 * score convention of every record coder (for unit-norm atoms the plain LASSO; ridge > 0: the elastic net).  One stage of the
 * working-set coder = ss_hip_top_correlations_* (its score |a_i . r_b| / ||a_i|| against lam_b is this problem's optimality
 * condition over ALL columns), ss_hip_extend_records_*, this call.
 * LASSO ORDER (csrc/refit.hip states it statement for statement): one workgroup per signal, in double, in LDS,
 * every decision taken by every thread from the same words.  From P empty and z = 0:
 *     1. entry test   over the positions e not in P with G_ee > 0:  w_e = (h - G z)_e,  v_e = |w_e| / g_e - lam_b;  the largest v_e
 *                     among those with v_e > tau = 8 K eps(T) sqrt(yy) enters with the sign sigma_e = sign(w_e), ties to the smallest
 *                     record position; none: the signal is done
 *     2. factor row   a row is appended to the packed Cholesky factor of (G + ridge diag G)_PP: the non-negative refit's row with the
 *                     diagonal G_jj (1 + ridge) and the right-hand side h_j - lam_b g_j sigma_j; the pivot test is
 *                     d > 8 K eps(T) G_jj (1 + ridge), a failure SS_HIP_REFIT_SINGULAR
 *     3. inner loop   back-substitute to s.  sigma_p s_p > 0 for every p in P: z_P = s, back to 1.  Otherwise alpha = the minimum over
 *                     the violators of z_p / (z_p - s_p) (0 where sigma_p z_p is not positive; ties to the smallest position in P),
 *                     z = z + alpha (s - z) on P, the minimiser and every e with sigma_e z_e not positive leave P with z_e = 0 exactly
 *                     and their signs forgotten, the factor is formed again row by row.  At most 3 K solves a signal
 *     records_out[b]  as ss_hip_nonneg_refit_records_* writes it: for SS_HIP_REFIT_DONE the entries with (T) z_e != 0, in record
 *                     order, compacted — K' of them, K' in word 0, idx[0 .. K') and val[0 .. K') theirs (z_e rounded once to T),
 *                     idx[K' .. K) and val[K' .. K) zero words; iter, err, the slots behind K and the padding copied word for word.
 *                     K' = 0 is a valid result (lam_b at or above max_e |h_e| / g_e).  For every other status the record is copied
 *                     unchanged
 *     resnorm[b]      (may be NULL) as for ss_hip_refit_records_*, of the record as written
 *     status[b]       (may be NULL) SS_HIP_REFIT_*: EMPTY and TRUNCATED as there; SS_HIP_REFIT_TOO_LARGE for kmax >= K >
 *                     SS_HIP_LASSO_KMAX; SS_HIP_REFIT_SINGULAR when a row fails the pivot test, or when yy, an h_e or a G_ee is not
 *                     finite; SS_HIP_REFIT_STALLED past the cap of 3 K solves
 *     dropped[b]      (may be NULL) K - K' for SS_HIP_REFIT_DONE, else 0
 * lam: lam_stride = 0: lam[0] for every signal; lam_stride = 1: lam[b].  A host or a device pointer.  ridge >= 0 by value.
 * With ridge = 0 the second copy of a column named twice never passes the entry test (it is dropped, not SINGULAR); with ridge > 0
 * the problem is strictly convex and both copies are kept with equal values.
 * SS_HIP_LASSO_KMAX is 128: the non-negative refit's LDS block and two more vectors of K doubles (the signs, the g_e), about 141 KB
 * of one CU's 160 KiB; the request is sized from min(kmax, SS_HIP_LASSO_KMAX).
 * CONTRACT: signal b's words are a function of (record b, y_b, A, lam_b, ridge) alone — bit for bit the same alone or in any batch, in
 * any batch order, with host or device pointers, in place or out of place, across the internal chunking, and whatever the context did
 * before.  No floating-point atomics.  No absolute constant: under A * 2^a, Y * 2^b, lam * 2^b and record values * 2^(b - a) the kept
 * sets are the same and the values scale by 2^(b - a) exactly.  No option key, no field of ss_hip_stats.
 * Validation: ss_hip_refit_records_*', then SS_HIP_EINVAL for a null lam, a lam_stride other than 0 or 1, a negative or non-finite
 * ridge; a lam_b that is negative or not finite is SS_HIP_EINVAL too, found on the device beside the records' index check — all
 * before anything is written.  B = 0 is SS_HIP_OK.
 */
#define SS_HIP_LASSO_KMAX 128
int ss_hip_lasso_refit_records_f32(ss_hip_ctx* ctx, const float* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy,
                                   const void* records, uint32_t kmax, void* records_out,
                                   const double* lam, ptrdiff_t lam_stride, double ridge,
                                   double* resnorm, uint32_t* status, uint32_t* dropped, char* err, size_t errlen);
int ss_hip_lasso_refit_records_f64(ss_hip_ctx* ctx, const double* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy,
                                   const void* records, uint32_t kmax, void* records_out,
                                   const double* lam, ptrdiff_t lam_stride, double ridge,
                                   double* resnorm, uint32_t* status, uint32_t* dropped, char* err, size_t errlen);

/*
 * The correlation sweep on its own, c = A^T r — the blas::xgemv(CblasTrans, ...)
 * of residual_vector (homotopy-cpu.cpp:97).  Runs `repeats` launches (>= 1) and
 * reports the mean kernel time in milliseconds measured with HIP events on the
 * context's stream (ms_out may be NULL).  r: m elements, c: n elements.
 */
int ss_hip_gemv_t_f32(ss_hip_ctx* ctx, const float* r, float* c, int repeats, float* ms_out,
                      char* err, size_t errlen);
int ss_hip_gemv_t_f64(ss_hip_ctx* ctx, const double* r, double* c, int repeats, float* ms_out,
                      char* err, size_t errlen);

/*
 * Batched correlations C[b][:] = A^T R[b][:] for B right-hand sides sharing the context's
 * matrix — the MFMA (fp32 matrix-core) form the batched solver uses once B signals run in
 * lock-step.  R: B rows of m elements (row stride ldR), C: B rows of n elements (ldC).
 * fp32 contexts only.  ms_out: mean GEMM time over `repeats` launches (HIP events).
 */
int ss_hip_gemm_t_f32(ss_hip_ctx* ctx, const float* R, size_t B, ptrdiff_t ldR, float* C, ptrdiff_t ldC,
                      int repeats, float* ms_out, char* err, size_t errlen);

/*
 * Gram columns G[s][:] = A^T a_{cols[s]} for up to 32 dictionary columns (host index list) in
 * ONE pass over the matrix: the "lookahead sweep" of the single-signal solver, which fetches
 * the correlations of the 32 most likely next entrants at once so that most Homotopy
 * iterations need no sweep at all.  32 right-hand sides are 16 flop per byte of A — still
 * HBM-bound on MI355X — computed on the fp32 MFMA units.  G: S rows of n elements (ldG).
 */
int ss_hip_gram_cols_f32(ss_hip_ctx* ctx, const uint32_t* cols, size_t S, float* G, ptrdiff_t ldG,
                         int repeats, float* ms_out, char* err, size_t errlen);
/* the same pass in double precision (v_mfma_f64_16x16x4_f64) */
int ss_hip_gram_cols_f64(ss_hip_ctx* ctx, const uint32_t* cols, size_t S, double* G, ptrdiff_t ldG,
                         int repeats, float* ms_out, char* err, size_t errlen);

/*
 * The same Gram columns for 1..64 dictionary columns, in every form a solve runs the pass in: S <= 32 runs the
 * 32-column pass, S > 32 the 64-column pass (the first lookahead sweep of a solve) — the choice a solve makes.
 * Measurement / test entry; G: S rows of n elements (ldG).  For S <= 32 and tier = 0 the words are
 * ss_hip_gram_cols_*'s.
 *   tier = 0    the context's own configuration (fp32: option sweep32_variant names the tiling of the 32-column pass)
 *   tier = 1    fp64 only: the 32-column pass in 128-column tiles, three workgroups per CU (the 64-column pass has one tiling)
 *   tier = k>=2 fp64 only: the rows split over k workgroups per column tile, the partial sums added up in order (the form
 *               narrow sub-dictionaries of the fp64 screened solve run).  The padded row count (m rounded up to 256) must be
 *               a multiple of 16 k: SS_HIP_EINVAL otherwise.  The partial sums (k * 64 * n_pad doubles) live for the call.
 * The tier is an argument of this call only; the context is left as it was found, whatever the call returns.
 */
int ss_hip_gram_cols_wide_f32(ss_hip_ctx* ctx, const uint32_t* cols, size_t S, int tier, float* G, ptrdiff_t ldG,
                              int repeats, float* ms_out, char* err, size_t errlen);
int ss_hip_gram_cols_wide_f64(ss_hip_ctx* ctx, const uint32_t* cols, size_t S, int tier, double* G, ptrdiff_t ldG,
                              int repeats, float* ms_out, char* err, size_t errlen);

/*
 * Rows of the context's G = A^T A: out[i][0 .. n) = G[rows[i]][0 .. n) for `count` row indices < n (host list; out: host or
 * device memory, row stride ldout >= n).  A context that has not formed G yet forms it here, exactly as its first large batch
 * would: within the budget of option gram_full_gib, by the build option gram_symmetric names, counted in gram_full_builds.
 * SS_HIP_ENOMEM with a message when G does not fit the budget or the free device memory.  fp32 Homotopy contexts only.
 * Measurement / test entry: the entries of G are what the batched Gram forms and the full-G single solve decide on.
 */
int ss_hip_gram_full_rows_f32(ss_hip_ctx* ctx, const uint32_t* rows, size_t count, float* out, ptrdiff_t ldout,
                              char* err, size_t errlen);

/*
 * Gs[i][j] = a_{cols[i]} . a_{cols[j]} for a subset of exactly 256 dictionary columns (host index list; entries
 * >= n give zero rows / columns): the 256 x 256 Gram matrix the early speculative iterations of the single-signal
 * engine run on while the full Gram columns are still being swept (csrc/subgram.hip).  Every entry is, bit for
 * bit, the value ss_hip_gram_cols_f32 returns for the same pair of columns.  Gs: 256 * 256 floats, row-major.
 */
int ss_hip_subset_gram_f32(ss_hip_ctx* ctx, const uint32_t* cols, float* Gs, int repeats, float* ms_out,
                           char* err, size_t errlen);

/*
 * y = A x on the device copy — ss::reconstruct_signal (src/lib.cpp:78-104).
 * x: n elements, y: m elements.
 */
int ss_hip_reconstruct_f32(ss_hip_ctx* ctx, const float* x, float* y, char* err, size_t errlen);
int ss_hip_reconstruct_f64(ss_hip_ctx* ctx, const double* x, double* y, char* err, size_t errlen);

/*
 * ss::norm_l1 (src/linalg/norms.h:22-27, src/lib.cpp:106-112): every column of the m x n matrix is divided,
 * IN PLACE, by its l1 norm sum_i |A(i, j)| (a zero column becomes NaN, like the reference's 0 / 0).  A may be
 * a device buffer (normalised where it lives: a column reduction and a scale kernel) or a host matrix (streamed
 * through the device in row panels); element (i, j) at A[i*stride_row + j*stride_col].  No context is needed:
 * in the reference this runs before the solver is constructed (src/solvers/test_util.h:167).
 */
int ss_hip_norm_l1_f32(float* A, size_t m, size_t n, ptrdiff_t stride_row, ptrdiff_t stride_col,
                       int device, char* err, size_t errlen);
int ss_hip_norm_l1_f64(double* A, size_t m, size_t n, ptrdiff_t stride_row, ptrdiff_t stride_col,
                       int device, char* err, size_t errlen);

/* ---- measurement ---------------------------------------------------------- */

typedef struct ss_hip_stats {
    uint64_t solves;               /* solve calls since the last reset                         */
    uint64_t iterations;           /* homotopy iterations over those solves                    */
    uint64_t sweep_launches;       /* fused 2-RHS sweep launches [c,q] = A^T [r,p] (timed ones) */
    double   sweep_ms;             /* sum of their HIP-event durations (profiling on)          */
    uint64_t sweep_bytes;          /* algorithmic bytes of ONE fused sweep: m*n*s + 2*m*s + 2*n*s */
    uint64_t sweep1_launches;      /* 1-RHS sweep launches (initial c = A^T y)                 */
    double   sweep1_ms;
    uint64_t sweep1_bytes;         /* m*n*s + m*s + n*s                                         */
    double   solve_ms;             /* HIP-event time of whole solves (upload of y .. x ready)  */
    uint64_t batch_rounds;         /* lock-step rounds run by the batched (MFMA) path — as the host
                                      enqueues them, up to "lookahead" rounds ahead of the device: the
                                      rounds queued after the last signal finished are no-ops, and how
                                      many there are depends on timing, not on the signals            */
    uint64_t lookahead_sweeps;     /* 32-RHS lookahead sweeps run by the fp32 single-signal engine */
    uint64_t sweep32_launches;     /* ... of which timed with HIP events (profiling on)         */
    double   sweep32_ms;           /* sum of their durations                                    */
    uint64_t sweep32_bytes;        /* algorithmic bytes of ONE lookahead sweep: m*n*s + 32*m*s + 32*n*s */
    uint64_t gram_fallbacks;       /* solves re-run in residual form: tolerance too tight for Gram-form correlations */
    uint64_t persist_fallbacks;    /* solves re-run without the resident kernel (its grid was not resident)         */
    uint64_t gram_full_builds;     /* times the full Gram matrix A^T A was formed for the batched Gram form        */
    uint64_t solo_solves;          /* solves that ran in the speculative form (one workgroup + verification)        */
    uint64_t solo_retries;         /* speculative launches whose verification failed (the solve went on in the resident form) */
    /* ABI version 2 */
    double   gram_build_ms;        /* HIP-event time of the MFMA GEMM(s) that formed G = A^T A (2 m n^2 flops each; n padded to 256) */
    double   gram_alloc_ms;        /* host wall time of allocating G (hipMalloc of n_pad^2 fp32)                                    */
    uint64_t cq_launches;          /* batched Gram form, profiling on: timed launches of k_la_cq (c, q of every live signal)        */
    double   cq_ms;                /* sum of their HIP-event durations                                                             */
    uint64_t cq_bytes;             /* algorithmic bytes of those launches: per live signal and round (K + 3) n s — K rows of G read,
                                      c0 read, c and q written                                                                     */
    uint64_t sweep64_launches;     /* first lookahead sweeps of fp32 solves that fetched 64 Gram columns in one pass (timed ones)   */
    double   sweep64_ms;           /* sum of their HIP-event durations (profiling on)                                              */
    uint64_t sweep64_flops;        /* algorithmic flops of ONE such pass: 2 * 64 * m * n (MFMA-bound: 16x the flops per byte of A
                                      of a GEMV)                                                                                  */
    uint64_t sweep64_bytes;        /* its algorithmic bytes: m*n*s + 64*m*s + 64*n*s                                               */
    uint64_t batch_col_rounds;     /* rounds of mid-size batches run in the column form (Gram columns of the entering columns
                                      formed per round, 64 signals per pass over A)                                                */
    uint64_t sweep32_timed_cols;   /* dictionary columns covered by ONE timed lookahead launch: n, or — early form with the pass
                                      dealt out by shader engine (option early_se) — the main launch's share of them (57344 of
                                      65536: the rest runs beside it on another stream); its algorithmic bytes are
                                      m*cols*s + 32*m*s + 32*cols*s                                                                 */
    /* ABI version 3 */
    uint64_t sweep32_bytes_timed;  /* algorithmic bytes of the timed lookahead launches, summed launch by launch (a plain pass covers all
                                      n columns, the early form's main launch its share): sweep32_bytes_timed / sweep32_ms is the rate  */
    uint64_t tie_reruns;           /* signals solved again in the reference-order engine because a step-length scan met an exact tie
                                      (option "tie_rerun"): an off-support column attained max|c|, the reference's strict t > 0
                                      (homotopy-cpu.cpp:143-153) skips it for good, and which rounding hits that is luck                 */
    uint64_t ro_resweeps;          /* reference-order engine (engine 3): iterations whose direction had to be rebuilt from the signs of
                                      the re-computed correlations, i.e. that took a second pass over A (otherwise one per iteration)   */
    uint64_t subset_signals;       /* batched Gram form, subset form (csrc/subbatch.hip): signals solved by one workgroup on the 448 columns
                                      with the largest |A^T y| and confirmed against all columns                                        */
    uint64_t subset_redone;        /* ... signals that form declined (left its common path) or whose check failed: solved again in the
                                      lock-step Gram form                                                                              */
    double   sub_solve_ms;         /* profiling on: HIP-event time of the form's selection + per-signal solves                            */
    double   sub_verify_ms;        /* ... and of its check over all columns                                                              */
    double   c0_gemm_ms;           /* ... and of the batch GEMM C0 = Y A (k_gemm_tn_f32: c0 = A^T y of every signal of a chunk)            */
    double   c0_gemm_flops;        /* its algorithmic flops: 2 * rows * ldm * n_pad per chunk (rows = signals padded to 128)               */
    /* ABI version 4 */
    uint64_t screen_signals;       /* single fp32 signals solved in the screened form (csrc/screen.hip): the subset solve on the subset's own
                                      Gram matrix, every state of the path certified against all columns by one pass over the fp16 copy
                                      of A (rigorous error bound; nothing reported comes from that pass)                                  */
    uint64_t screen_redone;        /* ... signals that form declined or could not certify: solved again in the default engine              */
    uint64_t screen_launches;      /* timed launches of the screening pass k_scr_gemm (profiling on)                                      */
    double   screen_ms;            /* sum of their HIP-event durations                                                                    */
    uint64_t screen_bytes;         /* their algorithmic bytes: ldm * n_pad * 2 (fp16 copy of A) + 96 * ldm * 2 + n_pad * 4 each             */
    double   screen_headroom;      /* largest (|c~| + eps) / bound over the columns outside the subset and the states of the LAST
                                      screened solve (< 1: certified; refreshed by ss_hip_get_stats)                                       */
    uint64_t first16_launches;     /* timed launches of the screened form's first pass over the fp16 copy, k_scr_first (option
                                      "screen_first16"; profiling on)                                                                     */
    double   first16_ms;           /* sum of their HIP-event durations                                                                    */
    uint64_t first16_bytes;        /* their algorithmic bytes: ldm * n_pad * 2 (fp16 copy of A) + ldm * 4 (y) + n_pad * 4 (c~0) each        */
    /* ABI version 5 */
    uint64_t screen_resident;      /* screened signals (fp32 and fp64) whose path ran in the resident kernel (csrc/resident.hip: one workgroup,
                                      Gram values in registers) and was certified                                                         */
    uint64_t screen_tier2;         /* fp64: signals the resident tier (256 columns) did not report and the sub-dictionary tier (2048 columns,
                                      launch-per-iteration engine) took next                                                              */
    /* why a signal of the subset / screened forms was NOT reported by the tier that tried it (one signal may count in several;
       a signal that ends up in the default engine is counted once in screen_redone / subset_redone as before)                          */
    uint64_t why_removal;          /* a column would leave the support (only regular paths are certified)                                  */
    uint64_t why_positions;        /* more support columns than the subset kernel holds (72 fp32 / 144 fp64)                               */
    uint64_t why_breakpoints;      /* more states than its log holds (80 / 160)                                                           */
    uint64_t why_guard;            /* tolerance below the Gram-form guard                                                                 */
    uint64_t why_no_candidate;     /* no positive step-length candidate on the subset                                                     */
    uint64_t why_first_state;      /* state 0 not certified: the columns left out of the subset may reach lambda_0 (crowded first state)   */
    uint64_t why_irregular;        /* lambda went up along the path (e.g. derailed by the reference's first-step sign quirk)               */
    uint64_t why_overflow;         /* a residual overflowed the half-precision range                                                      */
    uint64_t why_column;           /* the screening pass (or the subset form's check) could not certify a (column, state)                  */
    uint64_t why_tie;              /* the subset's scan met an exact tie (its view: the default engine decides)                            */
    uint64_t screen_recheck;       /* screened signals whose uncertified (column, state) pairs were re-derived exactly in fp32 and passed   */
    uint64_t res_solve_launches;   /* timed launches (profiling on) of the path kernel of a screened single signal — k_res_solve (or, option
                                      screen_resident = 0, k_sub_solve): ONE workgroup, all iterations of the solve                        */
    double   res_solve_ms;         /* sum of their HIP-event durations                                                                    */
    /* ABI version 6 */
    uint64_t screen_rescued;       /* screened signals (fp32 and fp64 resident tier) certified by the RESCUE: the first attempt declined — a planted column was ranked out
                                      of the subset — its log named the missing columns, the second attempt held them (option "screen_rescue")  */
    uint64_t screen_rescue_tried;  /* rescues attempted                                                                                  */
    /* ABI version 7 */
    uint64_t omp_batch_signals;    /* OMP batches (ss_hip_omp_solve_batch_*): signals a batch CHUNK certified — fp32 Gram or screened form, fp64 resident tier
                                      (not the signals it ran one at a time, nor those it handed to the single-signal ladder)              */
    uint64_t omp_batch_redone;     /* ... signals a chunk declined or could not certify: solved again alone by the single-signal ladder       */
    uint64_t omp_gram_signals;     /* ... of omp_batch_signals, those certified by the Gram form (csrc/ompbatch.hip: the path on the 448-column subset
                                      with its Gram matrix gathered from G = A^T A, every state checked against all columns by the MFMA pass
                                      over the rows of G at the signal's support)                                                        */
    /* ABI version 7, added with the IRLS batch */
    uint64_t irls_batch_signals;   /* IRLS batches (ss_hip_irls_solve_batch_*): signals solved (each also counts in solves, its iterations in iterations) */
    uint64_t irls_batch_rounds;    /* ... lock-step Newton rounds run by the blocked batch form (n >= 96), one host read of the live-slot count each */
} ss_hip_stats;

/* ---- IRLS: the reference's second solver (src/solvers/irls-cpu.cpp:63-124) ----------------------
 *
 * Replaces construction of solver<T, irls_policy>'s state — irls_state(A) = qr_decomposition<T>(A)
 * (include/ss/policies.h:77-85, src/lib.cpp:51-57, src/linalg/qr_decomposition.h:93-139) — and
 * solve_irls::op<mode, T> (src/solvers/irls.h:27-38).  Requires m >= n (the reference asserts it).
 * create: uploads A like ss_hip_homotopy_create_*, factorises it on the device (Householder QR,
 * thin Q, R, Q^T Q).  solve: outputs are irls_report{iter, solution_error, spd_failure}
 * (policies.h:58-72); x is normalised to sum 1 like the reference's (irls-cpu.cpp:121).
 * An IRLS context is not a Homotopy context: each family of entry points rejects the other's. */
ss_hip_ctx* ss_hip_irls_create_f32(const float* A, size_t m, size_t n, ptrdiff_t stride_row, ptrdiff_t stride_col,
                                   int device, char* err, size_t errlen);
ss_hip_ctx* ss_hip_irls_create_f64(const double* A, size_t m, size_t n, ptrdiff_t stride_row, ptrdiff_t stride_col,
                                   int device, char* err, size_t errlen);
int ss_hip_irls_solve_f32(ss_hip_ctx* ctx, const float* y, ptrdiff_t incy, float tolerance, uint32_t max_iterations,
                          float* x, ptrdiff_t incx, uint32_t* iter_out, double* solution_error_out,
                          int* spd_failure_out, char* err, size_t errlen);
int ss_hip_irls_solve_f64(ss_hip_ctx* ctx, const double* y, ptrdiff_t incy, double tolerance, uint32_t max_iterations,
                          double* x, ptrdiff_t incx, uint32_t* iter_out, double* solution_error_out,
                          int* spd_failure_out, char* err, size_t errlen);
/*
 * IRLS batch (added under ABI version 7): B signals against the context's factorised matrix.  Signal b is
 * Y[b*y_stride + i*incy], its solution X[b*x_stride + j*incx]; Y and X may be host or device pointers.  iter_out,
 * solution_error_out and spd_failure_out (each [B], may be NULL) receive every signal's irls_report.  Validation is the
 * single solve's: SS_HIP_EINVAL for a Homotopy context, a null Y or X, max_iterations == 0 or non-positive increments;
 * SS_HIP_ETYPE on a dtype mismatch; B == 0 returns SS_HIP_OK and touches nothing.
 * CONTRACT: signal b's x, iter, solution_error and spd_failure are BIT FOR BIT what ss_hip_irls_solve_* returns for it alone
 * on the same context — for every B, every chunking (option "irls_batch_max"), both dtypes and whatever the context did
 * before: the batch kernels (csrc/irlsbatch.hip) run the single solve's statements in its order per signal.
 * Forms: the single solve's choice for this n — n < 96 (or SS_HIP_IRLS_FUSED): one workgroup per signal, one launch per
 * chunk; otherwise the blocked chain with every launch covering the chunk's live signals and one host read per Newton round
 * (ss_hip_stats::irls_batch_rounds).  A batch adds B to ss_hip_stats::solves and its iterations to iterations, as a loop of
 * single solves would, and B to irls_batch_signals.
 */
int ss_hip_irls_solve_batch_f32(ss_hip_ctx* ctx, const float* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy,
                                float tolerance, uint32_t max_iterations, float* X, ptrdiff_t x_stride, ptrdiff_t incx,
                                uint32_t* iter_out, double* solution_error_out, int* spd_failure_out, char* err, size_t errlen);
int ss_hip_irls_solve_batch_f64(ss_hip_ctx* ctx, const double* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy,
                                double tolerance, uint32_t max_iterations, double* X, ptrdiff_t x_stride, ptrdiff_t incx,
                                uint32_t* iter_out, double* solution_error_out, int* spd_failure_out, char* err, size_t errlen);
void ss_hip_irls_destroy(ss_hip_ctx* ctx);

/* ---- one signal over a COLUMN-SHARDED dictionary (csrc/colshard.hip) -------------------------------
 *
 * For dictionaries beyond one GPU's memory (or n >> 10^6): every rank — one process per GPU — owns the columns
 * [col_lo, col_lo + n_local) of the m x n_total sensing matrix; the reference's iteration (homotopy-cpu.cpp:236-272)
 * runs with the O(m n) work local to the shard (the correlation sweep of the shard's own context) and its reductions
 * over all columns as device-side collectives: one (value, index) all-reduce for lambda = ||A^T r||_inf and the
 * left-most arg-max (homotopy-cpu.cpp:32-37), one for the smallest step length and its left-most column (:122-163),
 * and one all-reduce of m + kcap floats that carries the entering column from its owner to everyone.  The active
 * set (support, (A_S^T A_S)^-1, x_S, the active columns) is replicated: every rank performs the same update.
 * Results equal the single-GPU residual form (option "engine" = 0) to rounding; sharded and unsharded runs of THIS
 * entry point agree bit for bit.
 *
 * Transport: RCCL (librccl.so is opened at run time) — rank 0 calls ss_hip_comm_unique_id, distributes the 128 bytes
 * out of band (MPI, torch.distributed, a file) and every rank passes them to create, which calls ncclCommInitRank —
 * or, with comm_id == NULL, a table of HOST collectives (in-place all-reduces on host memory, called by every rank in
 * the same order; tests and other transports).  world == 1 needs neither.
 * x_local receives the shard's n_local coefficients; iter_out / err_out as ss_hip_homotopy_solve_f32.  Options
 * "strict_sign", "tie_guard", "zero_on_removal", "trace" apply; destroy with ss_hip_homotopy_destroy. */
#define SS_HIP_COMM_ID_BYTES 128
typedef struct ss_hip_collectives {
    void* user;
    int (*allreduce_max_u64)(void* user, uint64_t* buf, size_t count);   /* 0 on success */
    int (*allreduce_min_u64)(void* user, uint64_t* buf, size_t count);
    int (*allreduce_sum_f32)(void* user, float* buf, size_t count);
} ss_hip_collectives;
int ss_hip_comm_unique_id(unsigned char* id /* SS_HIP_COMM_ID_BYTES */, char* err, size_t errlen);
ss_hip_ctx* ss_hip_homotopy_colshard_create_f32(const float* A_local, size_t m, size_t n_local,
                                                ptrdiff_t stride_row, ptrdiff_t stride_col,
                                                size_t col_lo, size_t n_total, int device,
                                                const unsigned char* comm_id, int rank, int world,
                                                const ss_hip_collectives* host_collectives,
                                                char* err, size_t errlen);
int ss_hip_homotopy_colshard_solve_f32(ss_hip_ctx* ctx, const float* y, ptrdiff_t incy, float tol, uint32_t max_iter,
                                       float* x_local, ptrdiff_t incx, uint32_t* iter_out, double* err_out,
                                       char* err, size_t errlen);
/* The same in fp64 (round 4).  A double and its column index do not share one 64-bit word, so the two (value, index)
 * reductions of an iteration travel as a [world][2] table of 64-bit words — every rank fills its own pair, zeros elsewhere —
 * gathered by ONE exact MAX all-reduce each and reduced by every rank in the same order (largest value, then smallest global
 * index): still three collectives per iteration (2 x 16 * world bytes, (m + kcap) * 8 bytes), at most 64 ranks.  The host
 * table therefore needs two entries only.  Sharded and unsharded runs agree bit for bit, like in fp32. */
typedef struct ss_hip_collectives_f64 {
    void* user;
    int (*allreduce_max_u64)(void* user, uint64_t* buf, size_t count);   /* 0 on success */
    int (*allreduce_sum_f64)(void* user, double* buf, size_t count);
} ss_hip_collectives_f64;
ss_hip_ctx* ss_hip_homotopy_colshard_create_f64(const double* A_local, size_t m, size_t n_local,
                                                ptrdiff_t stride_row, ptrdiff_t stride_col,
                                                size_t col_lo, size_t n_total, int device,
                                                const unsigned char* comm_id, int rank, int world,
                                                const ss_hip_collectives_f64* host_collectives,
                                                char* err, size_t errlen);
int ss_hip_homotopy_colshard_solve_f64(ss_hip_ctx* ctx, const double* y, ptrdiff_t incy, double tol, uint32_t max_iter,
                                       double* x_local, ptrdiff_t incx, uint32_t* iter_out, double* err_out,
                                       char* err, size_t errlen);

/* profiling != 0: bracket every sweep launch with HIP events on the context's stream. */
int ss_hip_set_profiling(ss_hip_ctx* ctx, int profiling);
int ss_hip_get_stats(ss_hip_ctx* ctx, ss_hip_stats* out);
int ss_hip_reset_stats(ss_hip_ctx* ctx);

/*
 * Tuning knobs (integers), for benchmarks only; unknown keys return SS_HIP_EINVAL.
 *   "sweep_variant"  kernel variant of the sweep (see csrc/sweep.hip)
 *   "lookahead"      iterations the host enqueues ahead of the device's done flag
 *   "strict_sign"    1 = seed the first direction with sign(c[idx]) instead of the
 *                    reference's sign(|c[idx]|) (homotopy-cpu.cpp:223-227); default 0
 *   "trace"          1 = record the homotopy path of each solve (ss_hip_get_trace)
 *   "engine"         single-signal Homotopy: 1 (default) = lookahead engine — Gram
 *                    columns A^T a_j of active columns are cached and A is swept (32 right-hand
 *                    sides per pass) only when an uncached column enters — unless the tolerance
 *                    is below 2^-14 (fp32) / 2^-42 (fp64) * ||A^T y||_inf, too tight for Gram-form
 *                    correlations: such a solve runs as 0; 2 = lookahead engine unconditionally;
 *                    0 = one fused 2-RHS sweep per iteration (residual form);
 *                    3 = reference-order engine (csrc/reforder.hip): the reference's values statement for statement
 *                    — c = A^T(y - A x) re-computed, the direction formed from the signs of THAT c —
 *                    with every reduction in ONE documented order (8 partial sums, term r to partial r & 7, combined
 *                    ((0+1)+(2+3))+((4+5)+(6+7)), products and sums separately rounded): the path is reproducible bit
 *                    for bit by any implementation that states the same order.  One pass over A per iteration (2 GiB
 *                    at 8192 x 65536, 0.84 of the HBM peak); batches run up to 4 signals per pass; the arbiter of
 *                    "tie_rerun".
 *   "batch_screen"   1 (default) = fp32 batches of at least 4 signals on a context without G = A^T A (see "batch_gram_min"), on dictionaries
 *                    the screened form applies to ("screen_single"), run in that form chunk by chunk (64 signals): c0 of the chunk
 *                    by the batch GEMM, every signal solved by one workgroup on its subset's own Gram matrix, one screening launch
 *                    over the fp16 copy of A for the whole chunk (four signals per workgroup); a signal it hands back is solved by
 *                    the default single-signal engine.  Results agree with solve() to rounding, not bit for bit; 0 = the column
 *                    form ("batch_cols_min") or one solve per signal as before
 *   "batch_subset"   1 (default) = batches that run in Gram form on the full G = A^T A use the SUBSET form
 *                    (csrc/subbatch.hip): every signal is solved by one workgroup on the 448 columns with the largest
 *                    |A^T y| and every breakpoint is then checked against all columns by the same chain of fmas; a signal
 *                    the form declines (left its common path) or whose check fails is solved again in the lock-step
 *                    form (ss_hip_stats::subset_signals / subset_redone); 0 = the lock-step form for all
 *   "screen_single"  1 (default) = single fp32 signals on dictionaries of >= 16 Mi entries and >= 8192 columns take the
 *                    SCREENED form (csrc/screen.hip): c0 = A^T y in fp32, the whole path by one workgroup on the 448 columns
 *                    with the largest |c0| (their Gram matrix formed from A), then ONE pass over an fp16 copy of A (kept by
 *                    the context: half of A's bytes again) that certifies every state of the path against all columns —
 *                    |c~| + eps <= 7/8 lambda with eps = 2^-9 ||a_i|| ||r_k|| + flush terms, a rigorous bound.  Nothing
 *                    reported comes from that pass; a signal it cannot certify, or whose path leaves the subset form's
 *                    common path, is solved again by the default engine (ss_hip_stats::screen_signals / screen_redone).
 *                    fp64 contexts (>= 32768 columns, >= 64 Mi entries): the same certificate around the fp64 engine, which
 *                    solves the path on a sub-dictionary of the 2048 columns with the largest |c0| (a context of its own).
 *                    2 = on every shape the form can run on (tests); 0 = never.  Initial value: environment variable
 *                    SS_HIP_SCREEN_SINGLE when set.  Stands in for the default speculative engine only ("la_fused" = 3,
 *                    "early_solo" = 1); with G = A^T A in HBM the subset form on G ("gram_single") is used instead only where the
 *                    half-precision first pass ("screen_first16") does not apply — with it the screened form is the faster one.
 *   "screen_first16" 1 (default) = the screened form of one fp32 signal reads the fp16 copy for its FIRST pass too (row counts padded to
 *                    a multiple of 512, at most 15872): c~0 = A16^T y ranks the columns, the exact fp32 c0 of the 448 chosen ones
 *                    is formed beside their Gram matrix (lambda_0, the first pick and the path come from those), and state 0 is
 *                    certified like every other state: T + eps_0 <= 7/8 lambda_0 with T above every |c~0| left out and
 *                    eps_0 = 2^-9 max ||a_i|| ||y|| + the flush term.  No fp32 pass over A is left in a certified solve
 *                    (ss_hip_stats::first16_*); 0 = c0 = A^T y by the fp32 sweep
 *   "screen_first8"  1 (default) = where the padded row count is a multiple of 1024 that first pass reads an FP8 (OCP e4m3) copy of A instead of the
 *                    fp16 copy (a quarter of A's bytes again, made on the first such solve): the pass only RANKS the columns and bounds what it
 *                    left out — eps_0 = 2^-4 x 1.02 max ||a_i|| ||y|| + its flush term, sixteen times the fp16 pass's, written by the pass
 *                    itself for the state-0 certificate; nothing it computes is reported.  fp32 and fp64 contexts; 0 = the fp16 copy
 *                    (no fp8 copy is made); an allocation that does not fit does the same by itself
 *   "screen_resident" 1 (default) = the path of the screened form runs in the one-workgroup resident kernel (csrc/resident.hip; fp32: 448 columns,
 *                    72 positions; fp64: 256 columns, 136 positions — the fp64 resident tier); 0 = fp32: k_sub_solve, fp64: the sub-dictionary
 *                    tier only.  OMP takes the screened form only with 1
 *   "screen_rescue"  1 (default) = a single fp32 signal the screened form declined because its path ran out of positions or an outside column beat
 *                    a state is scanned for the columns the ranking missed (the certificate pass over the declined solve's early states) and
 *                    solved once more in the same form with those columns in the subset (ss_hip_stats::screen_rescued); 0 = it goes back
 *   "screen_recheck" 1 (default) = columns the half-precision certificate cannot clear are decided exactly from A in the solve's precision
 *                    (k_scr_recheck) and a last step an outside column stops early is repaired (k_scr_repair); 0 = such signals go back
 *   "gram_reserve"   1 (default) = the memory of G = A^T A is reserved on a helper thread when the first batch of >= 4 signals arrives, so that
 *                    the batch that forms G does not wait for the allocation; 0 = allocated on first use
 *   "solo_full_gram" tests: 1 = the speculative form may run with G = A^T A as its cache too (default 0: it does not — gathers of scattered entries)
 *   "pass_dbg_ptr"   developer aid: a device buffer (1 + 4 x 4096 u64) that receives a per-workgroup trace of the early form's passes (tools/probe_pass_trace.py)
 *   "colshard_fail_prepare" test aid: 1 = the next column-sharded solve fails on this rank while it prepares (the ranks must all leave)
 *   "ro_slots"       1..8 (default 8; fp64 contexts use at most 4): signals the reference-order engine runs in lock-step per pass over A (batches in
 *                    engine 3, a batch's tie re-runs); every signal's words are those of its own solve
 *   "ro_staged"      1 (default) = its sweep stages the dictionary through LDS (coalesced loads); 0 = direct 16-byte
 *                    loads (one signal per pass; the same bits at 0.35 of the HBM peak): A/B aid
 *   "ro_force_resweep" developer aid: 1 = every iteration of engine 3 takes its second sweep (the check of the
 *                    speculated signs is treated as failed): a schedule, not arithmetic — the same bits
 *   "la_fused"       form of the lookahead engine's iterations: 3 (default, fp32) = speculative resident form:
 *                    one workgroup iterates on a 256-column subset and every breakpoint is re-derived over
 *                    all columns, bit for bit, before anything is committed; 2 = one resident launch on all
 *                    CUs (k_la_persist, fp32; same results as 3; fp64 runs as 1), 1 = one launch per
 *                    iteration, 0 = separate kernels
 *   "solo_subset"    columns beyond the support a speculative launch may hold (default 256; tests use small
 *                    values to provoke failed verifications)
 *   "sweep32_variant" tiling of the 32-RHS lookahead sweep (0 default; 1-7 measured alternatives, same results)
 *   "first_sweep_cols" 32 (default) / 64: 64 = the first lookahead pass of a fp32 solve (plain speculative form)
 *                    fetches the entering column and the 63 largest |A^T y| in ONE pass over A (2*64*m*n flops:
 *                    MFMA-bound, 0.61 ms at 8192 x 65536) instead of 32; measured no faster end to end
 *   "early_solo"     1 (default) = early form of the speculative engine (fp32, n > 16384): the first speculative
 *                    launch iterates on the 256 x 256 Gram matrix of its column subset (csrc/subgram.hip, the
 *                    pass's own arithmetic) while two 32-column passes over A run beside it on a second stream;
 *                    the passes' columns are what the verification then needs.  Same results, bit for bit, as 0
 *                    (= the passes first, then the launch)
 *   "early_pass"     tiling of the early form's two passes: 2 (default) = 128-column LDS-staged tiles, three 256-thread
 *                    workgroups per CU (all 512 tiles of 8192 x 65536 resident on the 255 CUs the speculative launch
 *                    leaves: 0.49 ms per pass beside it); 0 = one 32-column tile per single-wave workgroup (0.52 ms).
 *                    Same results bit for bit
 *   "early_se"       (3 = the same dealing-out for ANY tile count: 7u tiles per shader engine in the main launch, the
 *                    workgroups dealt out by SE come back until their SE has had u more — measured no faster than one launch per
 *                    pass beyond 65536 columns, kept as an option)
 *                    1 (default) = the early form's two passes are dealt out around the speculative workgroup: the
 *                    hardware gives every shader engine the same number of workgroups of a grid, and the SE of that
 *                    workgroup has 7 CUs for its share — so the main launch takes 14 tiles per SE, a second launch puts
 *                    two more workgroups on every SE, which pick their tile by where they run and leave at once on that
 *                    SE, and the last two tiles are formed by a VALU kernel: every other CU carries exactly two tiles
 *                    (0.37-0.38 ms per pass instead of 0.47-0.49; 256-CU parts, 57345..65536 columns); 0 = one launch
 *                    per pass.  Same results bit for bit
 *   "early_adapt"    1 (default) = the early form's second pass takes its 32 columns from the speculative launch's
 *                    progress when the first pass has finished (columns that have entered its support, then those
 *                    closest to entering); 0 = from the |c0| ranking.  Decides which Gram columns are fetched when,
 *                    never a result
 *   "cache_mib"      memory budget of the lookahead engine's Gram-column cache (default 2048)
 *   "batch_min"      smallest fp32 batch that takes the lock-step MFMA path (default 192: below
 *                    that, one lookahead solve per signal is faster)
 *   "batch_chunk"    signals processed together by the batched path (default 4096)
 *   "irls_batch_max" IRLS contexts: most signals one chunk of ss_hip_irls_solve_batch_* holds (default 256; 1..65535); chunks are
 *                    also bounded by 1 GiB of per-signal state (n^2 + 5 n + 2 ldm elements each).  Never changes a result
 *   "dl_chunk_max"   test aid: most signals whose residuals ss_hip_homotopy_atom_update_* holds at once (default 0 = a byte budget
 *                    alone; at most 32768); chunks are taken in ascending order with g carried between them: never changes a result
 *   "tc_chunk_max"   test aid: most signals whose residuals and dots ss_hip_top_correlations_* holds at once (default 0 = a byte budget
 *                    alone; at most 32768); every signal's row is formed on its own: never changes a result
 *   "batch_gram_min" (where the screened batch form applies — "batch_screen" — G pays later and is formed for a batch of at
 *                    least max(batch_gram_min, 1536) signals, or once the context has received 3072 signals in batches)
 *                    smallest lock-step batch that forms G = A^T A (n^2 fp32, 2 m n^2 flops once) and then
 *                    takes every signal's correlations from rows of G instead of two GEMMs per round
 *                    (default 512; once G exists every lock-step batch uses it; 0 = never)
 *   "batch_cols_min" fp32 batches of at least batch_cols_min signals (default 24) with no G at hand — below
 *                    batch_gram_min, or G switched off or too large — run in lock-step in the column form: per round ONE pass over A per 64 signals forms the Gram columns
 *                    of the columns that enter (a single solve spends three passes on one signal), and correlations
 *                    come from those cached columns as in the Gram form; chunks of at most 448 signals; smaller
 *                    batches run one solve per signal; batch_cols_min = 0: never (round-1 behaviour: one solve per
 *                    signal below batch_min, two GEMMs per round from there on)
 *   "batch_fused_scan" 1 (default) = the lock-step Gram forms scan inside the Gram-form pass (k_la_cqs: c and q of a
 *                    workgroup's columns stay in registers while the signal's workgroups meet for lambda = ||c||_inf);
 *                    0 = two kernels (k_la_cq writes c and q, k_scansel reads them back).  Same results bit for bit.
 *                    (A workgroup of 256 threads reads runs of 4096 columns of each of its signal's K rows of G, two rows in
 *                    flight per thread: 16 KiB runs stream at 82 % of the HBM peak where 4 KiB runs reached 64 %.)
 *   "gram_full_gib"  largest G — and largest column cache of the column form — that may be allocated
 *                    (default 64 GiB; 0 = never form G)
 *   "gram_full_after" opt-in (default 0 = never): single-signal solves (fp32) after which the context forms G
 *                    for them as well: with G in HBM every Gram column is at hand and a solve needs no pass over
 *                    A beyond A^T y — at the price of n^2 fp32 of HBM (17 GiB at 8192 x 65536) and one GEMM;
 *                    1 = from the first solve
 *   "gram_single"    1 (default) = once G exists (a large batch formed it, or gram_full_after) single-signal
 *                    solves use it as their Gram-column cache; 0 = they keep their own 32-column sweeps
 *   "gram_symmetric" 1 (default) = G is formed from the GEMM tiles on and above the diagonal, each stored to both
 *                    sides (half the flops, G exactly symmetric); 0 = the full product
 *   "profile_every"  with profiling on, bracket only every k-th fused sweep with events
 *   "profile_solve_every" with profiling on, only every k-th solve carries events at all (each event costs stream time)
 *   "tie_guard"      0 (default) = the reference's strict `t > 0` (homotopy-cpu.cpp:135,145,151): an
 *                    off-support column that attains max|c| exactly (it tied with an inserted column
 *                    within an ulp) is skipped for good and such a solve runs to max_iterations, as the
 *                    reference's does; 1 = opt-in fix: that column enters by a zero-length step
 *   "tie_rerun"      1 (default) = a solve (or a signal of a batch) whose step-length scan met an EXACT tie — an
 *                    off-support column that attains max|c|, candidate t == 0 — is solved again in the
 *                    reference-order engine (engine 3) and that result is returned: after such a tie the reference's
 *                    strict t > 0 decides by rounding whether the path derails, so the fast engines (other summation
 *                    orders) do not guess; ss_hip_stats::tie_reruns counts them.  0 = keep the fast engine's path
 *                    (with "tie_guard" = 1 the tie is resolved by the guard and nothing is re-run)
 *   "zero_on_removal" 0 (default) = a coefficient whose column leaves the support keeps the reference's
 *                    x + gamma*d rounding residue (homotopy-cpu.cpp:246-252; 0 or an ulp, and a
 *                    re-inserted column may bounce out again); 1 = opt-in fix: it is set to exactly 0.
 *                    Both fixes are restated in the CPU oracle (SS_ORACLE_TIE_GUARD,
 *                    SS_ORACLE_ZERO_ON_REMOVAL) so that the opt-in modes are checked too.
 */
int ss_hip_set_option(ss_hip_ctx* ctx, const char* key, long value);
int ss_hip_get_option(ss_hip_ctx* ctx, const char* key, long* value);

/*
 * The homotopy path of the LAST solve when option "trace" is on: entry 0 is the initial
 * pick, entry t the column toggled by iteration t (added = 1 insert / 0 remove), the step
 * length gamma taken and lambda = ||c||_inf at the start of that iteration.  OMP
 * (ss_hip_omp_solve_*) has no initial pick: its entry 0 is all zeros and entry t is the
 * column picked by iteration t.  Writes up to `capacity` entries into each non-NULL array;
 * *count receives the number available.
 */
int ss_hip_get_trace(ss_hip_ctx* ctx, uint32_t capacity, uint32_t* idx, uint8_t* added,
                     double* gamma, double* c_inf, uint32_t* count);

/* Shape / placement queries. */
int ss_hip_ctx_info(const ss_hip_ctx* ctx, size_t* m, size_t* n, int* is_f64, int* device);

#ifdef __cplusplus
}
#endif
#endif /* SS_HIP_H */
