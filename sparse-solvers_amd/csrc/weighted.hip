// weighted.hip — coding under a non-negative weight per row and signal, min sum_k w_kb (y_b - A x)_k^2 (include/ss_hip.h):
//   ss_hip_weighted_top_correlations_*, ss_hip_weighted_refit_records_*, ss_hip_weighted_class_residuals_*.
//
// A 0/1 mask of observed rows (occlusion, inpainting) is the special case; robust coders supply the weights from the previous
// residual (robust.hip makes them on the device).  A is shared by the batch and the weights are not: the atom norms become d(i, b) = sum_k w_kb a_ki^2, one per atom and
// signal, and the normal equations A_S^T W_b A_S — neither comes out of scaling Y beforehand.
//
// WEIGHTS, common to the three calls: row b of W at W[b * w_stride + k], k < m; w_stride == 0 is one vector shared by all signals.  A
// host caller's W is staged once per call (weights_on_device: [B][m], or [m] for the shared vector); k_w_check then finds the first
// weight that is negative or not finite — the smallest (signal, row) — before anything is written.  Rows m .. ldm - 1 weigh 0.
//
// LAYOUT of the selection: TWO PASSES of topcorr.hip's tile kernel, the second with its squaring flag (k_tc_tile<T, true>) — not one
// kernel with both accumulator sets.  Each pass keeps k_tc_tile's registers (64 accumulators a thread in fp32), its two workgroups a
// CU and its chain, so dot(i, b) here is bit for bit the dot the unweighted call forms from the same block, and the unflagged
// instantiation is untouched.  The compiler's resource report shows no scratch for either instantiation in either precision.
// The refit and the class residuals are refit.hip's and classify.hip's kernels with a weight flag (k_rf_gram<T, NT, true>: ONE
// operand scaled by w_k, not both by sqrt(w_k); k_cls_residual<T, false, true>), reached through refit_weighted /
// class_residuals_weighted: their checks, their order, their status codes.  Kernels of this unit, per chunk of signals:
//
//   k_w_check    grid-stride over the batch's weights: the first offender by atomicMin on (signal * m + row), an integer.
//   k_w_apply    one workgroup per signal: Wb[b][k] = w_kb (0 from row m on), R[b][k] = w_kb * r_kb in place — one multiplication in
//                T — and wmax_b = max_k w_kb (a maximum: any order gives the same word).
//   k_tc_tile    twice (tc_launch_dots, tc_launch_weight_dots): D = A^T (w o r), D2 = (A o A)^T w, both [chunk][n_pad] in T.
// THE SELECTION's host side is the driver of the top correlations (tc_driver.h) and its kernel is k_tc_select (tc_select.h).  This
// unit supplies the variant: a second residual-sized block (Wb), a second dot block (D2) and wmax to carve; d_i instead of rn_i from
// the norms kernel (coh_launch_norms with its flag: 0 for an excluded column — d_i zero or not finite, or i >= n — the visible share
// needs d_i, not rn_i); per chunk the three launches above; and the scorer WtScorer: a candidate's key formed in double from the
// stored words.
//
// ORDER (build flag -ffp-contract=off: outside the MFMA products and sums are rounded separately):
//   r_b          tc_launch_residual_block's words (top_correlations' residual); rw_b = w_b o r_b, one multiplication in T.
//   dot(i, b)    k_tc_tile's chain over rw_b: one accumulator from 0, the K-steps ascending (topcorr.hip, ORDER).
//   d(i, b)      the same chain with the operands (w_b, a_i o a_i): a_ki * a_ki rounded once to T where A is staged.
//   v(i, b)      = d(i, b) / (wmax_b * d_i) in double: the product first, then one division.
//   s(i, b)      = |dot| / sqrt(d(i, b)) in double: the square root, then one division.
//   coef         = (T)((double)dot / (double)d(i, b)): one division, one rounding to T.
//   candidates   i < n, not stored in record b, d_i finite and non-zero, d(i, b) > 0, v(i, b) > min_visible, s not NaN — by index
//                mask and comparison, never by arithmetic.  All weights zero: wmax_b = 0, d(i, b) = 0, no candidates.
// BOUND: |s - s_float64| <= (2 gamma_{m+1} + 1e-12) ||r_b||_w, ||r||_w = sqrt(sum w r^2): |fl(dot) - dot| <= gamma_m sum |a||w r| <=
// gamma_m sqrt(d(i, b)) ||r||_w (weighted Cauchy-Schwarz); fl(d) = d (1 + delta), |delta| <= gamma_{m+1} (non-negative terms, one more
// rounding for the square); s <= ||r||_w.
// No floating-point atomics.  Row b of the outputs is a function of (A, y_b, w_b, record b, k, min_visible) alone: nothing depends on
// B, on the chunking, on the launch geometry, on where the pointers live, on w_stride == 0 against repeated rows, or on what the
// context did before.
#include "ss_hip_internal.h"
#include "tc_driver.h"

#include <algorithm>
#include <cmath>
#include <limits>

namespace sship {

namespace {

constexpr unsigned long long kWtNoBad = ~0ull;

struct WeightedState {
    Holdings own;
    unsigned char* wbuf = nullptr;     // per call: the first-offender word, then a host caller's weights
    size_t wbuf_bytes = 0;
};

WeightedState* state_of(ss_hip_ctx* ctx)
{
    return &part<WeightedState>(ctx->wt);
}

// ---- kernels -------------------------------------------------------------------------------------------------------------------

// total = rows * m weights, row r of them at W[r * w_stride + k]; bad: the smallest r * m + k whose weight is negative or not finite
template <typename T>
__global__ __launch_bounds__(256)
void k_w_check(const T* __restrict__ W, long long w_stride, uint32_t m, unsigned long long total, unsigned long long* __restrict__ bad)
{
    for (unsigned long long e = (unsigned long long)blockIdx.x * 256u + threadIdx.x; e < total; e += (unsigned long long)gridDim.x * 256u) {
        const unsigned long long r = e / m, k = e - r * m;
        const T w = W[(long long)r * w_stride + (long long)k];
        if (!(w >= T(0) && w <= std::numeric_limits<T>::max())) atomicMin(bad, e);
    }
}

// R, Wb: [chunk][ldm]; W: the chunk's weights (row b at W[b * w_stride])
template <typename T>
__global__ __launch_bounds__(256)
void k_w_apply(const T* __restrict__ W, long long w_stride, uint32_t m, uint32_t ldm, T* __restrict__ R, T* __restrict__ Wb,
               double* __restrict__ wmax)
{
    __shared__ T s_mx[4];
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    const T* w = W + (long long)b * w_stride;
    T* r = R + (size_t)b * ldm;
    T* wb = Wb + (size_t)b * ldm;
    T mx = T(0);
    for (uint32_t k = tid; k < ldm; k += 256u) {
        const T wk = k < m ? w[k] : T(0);
        wb[k] = wk;
        r[k] = wk * r[k];
        mx = wk > mx ? wk : mx;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const T ov = __shfl_xor(mx, o); mx = ov > mx ? ov : mx; }
    if ((tid & 63u) == 0u) s_mx[tid >> 6] = mx;
    __syncthreads();
    if (tid == 0) {
        for (uint32_t v = 1; v < 4u; ++v) mx = s_mx[v] > mx ? s_mx[v] : mx;
        wmax[b] = (double)mx;
    }
}

// the weighted scorer for k_tc_select (tc_select.h).  D2: the chunk's second dot block, dn: d_i, wmax: the chunk's wmax_b
template <typename T> struct WtScorer {
    const T* __restrict__ D2;
    const double* __restrict__ dn;
    const double* __restrict__ wmax;
    double min_visible;
    struct Row {
        const T* d2;
        const double* dn;
        double wm, min_visible;
        __device__ bool key(const T* d, uint32_t i, unsigned long long& key) const
        {
            const double di = dn[i];
            if (di == 0.0) return false;
            const double dw = (double)d2[i];
            if (!(dw > 0.0)) return false;
            if (!(dw / (wm * di) > min_visible)) return false;
            const double s = fabs((double)d[i]) / sqrt(dw);
            if (!(s == s)) return false;
            key = (unsigned long long)__double_as_longlong(s);
            return true;
        }
        __device__ T coef(const T* d, uint32_t i) const { return (T)((double)d[i] / (double)d2[i]); }
    };
    __device__ Row row(uint32_t b, uint32_t n_pad) const { return { D2 + (size_t)b * n_pad, dn, wmax[b], min_visible }; }
};

// ---- host side -----------------------------------------------------------------------------------------------------------------

// the variant of the driver (tc_driver.h): a second residual-sized and a second dot-sized block and wmax; d_i for the norms; per
// chunk the weights applied, both products and the selection
template <typename T> struct WeightedVariant {
    const T* Wd;                       // the batch's weights on the device, row pitch wsd (weights_on_device)
    long long wsd;
    double min_visible;
    T* Wb = nullptr;
    T* D2 = nullptr;
    double* wmax = nullptr;

    void carve(const ss_hip_ctx* ctx, Carver& cv, size_t max_sig, size_t sig_pad, size_t)
    {
        Wb = cv.take<T>(sig_pad * ctx->ldm);
        D2 = cv.take<T>(sig_pad * ctx->n_pad);
        wmax = cv.take<double>(max_sig);
    }
    hipError_t prepare(ss_hip_ctx* ctx, double* dn) { return coh_launch_norms<T, true>(ctx, dn); }
    void chunk(ss_hip_ctx* ctx, const TcCall<T>& c, const TcChunk& ch, const TcWork<T>& w)
    {
        hipStream_t st = ctx->stream;
        const uint32_t Bc = ch.Bc, ldm = ctx->ldm, btiles = (Bc + kTcTile - 1u) / kTcTile;
        // (the rows behind the chunk's last signal, up to a whole tile, weigh zero as R's are zero: their dots are never read)
        if (btiles * kTcTile != Bc) HIPCHK(hipMemsetAsync(Wb + (size_t)Bc * ldm, 0, (size_t)(btiles * kTcTile - Bc) * ldm * sizeof(T), st));
        hipLaunchKernelGGL((k_w_apply<T>), dim3(Bc), dim3(256), 0, st, Wd + (ptrdiff_t)ch.b0 * wsd, wsd, (uint32_t)ctx->m, ldm, w.R, Wb, wmax);
        HIPCHK(hipGetLastError());
        HIPCHK(tc_launch_dots<T>(ctx, w.R, Bc, w.D));
        HIPCHK(tc_launch_weight_dots<T>(ctx, Wb, Bc, D2));
        tc_launch_select(ctx, c, ch, w, WtScorer<T>{ D2, w.norms, wmax, min_visible });
    }
};

// top_correlations' checks in its order, then the weights' and min_visible's
template <typename T>
int wtop_entry(ss_hip_ctx* ctx, const TcCall<T>& c, const T* W, ptrdiff_t w_stride, double min_visible)
{
    int rc = tc_check_call<T>(ctx, c);
    if (rc != SS_HIP_OK) return rc;
    if ((rc = weights_check_args(ctx, c.who, W, w_stride, c.err, c.errlen)) != SS_HIP_OK) return rc;
    if (!(min_visible >= 0.0 && min_visible < 1.0)) { set_err(c.err, c.errlen, "weighted_top_correlations: min_visible must lie in [0, 1)"); return SS_HIP_EINVAL; }
    return tc_run(c, [&] {
        HIPCHK(hipSetDevice(ctx->device));
        WeightedVariant<T> v{ nullptr, 0, min_visible };
        const int rw = weights_on_device<T>(ctx, c.who, W, c.B, w_stride, &v.Wd, &v.wsd, c.err, c.errlen);
        if (rw != SS_HIP_OK) return rw;
        // (two blocks of each kind, and wmax)
        const bool y_dev = on_device(c.Y);
        return tc_drive<T>(ctx, c, y_dev, c.B, tc_uniform_chunks(ctx, c.B, tc_signal_bytes<T>(ctx, y_dev, 2) + sizeof(double)), v);
    });
}

}  // namespace

// ---- what the three weighted calls share (ss_hip_internal.h) -----------------------------------------------------------------------

int weights_check_args(const ss_hip_ctx* ctx, const char* who, const void* W, ptrdiff_t w_stride, char* err, size_t errlen)
{
    if (!W) { set_err(err, errlen, std::string(who) + ": W must not be null"); return SS_HIP_EINVAL; }
    if (w_stride < 0 || (w_stride != 0 && (size_t)w_stride < ctx->m)) {
        set_err(err, errlen, std::string(who) + ": w_stride must be 0 (one shared weight vector) or at least m");
        return SS_HIP_EINVAL;
    }
    return SS_HIP_OK;
}

template <typename T>
int weights_on_device(ss_hip_ctx* ctx, const char* who, const T* W, size_t B, ptrdiff_t w_stride, const T** Wd, long long* wsd, char* err,
                      size_t errlen)
{
    HIPCHK(hipSetDevice(ctx->device));
    WeightedState* ws = state_of(ctx);
    hipStream_t st = ctx->stream;
    const size_t m = ctx->m, rows = w_stride == 0 ? 1 : B;
    const bool w_dev = on_device(W);
    grow(ws->own, ws->wbuf, ws->wbuf_bytes, 256 + (w_dev ? 0 : rows * m * sizeof(T)), "hipMalloc(weights)");
    unsigned long long* bad = reinterpret_cast<unsigned long long*>(ws->wbuf);
    const T* wd = W;
    long long pitch = (long long)w_stride;
    if (!w_dev) {
        T* dst = reinterpret_cast<T*>(ws->wbuf + 256);
        if (rows == 1) HIPCHK(hipMemcpyAsync(dst, W, m * sizeof(T), hipMemcpyHostToDevice, st));
        else HIPCHK(hipMemcpy2DAsync(dst, m * sizeof(T), W, (size_t)w_stride * sizeof(T), m * sizeof(T), rows, hipMemcpyHostToDevice, st));
        wd = dst;
        pitch = rows == 1 ? 0 : (long long)m;
    }
    flag_arm(reinterpret_cast<uint32_t*>(bad), st, 2);     // (one 64-bit word)
    const unsigned long long total = (unsigned long long)rows * m;
    const uint32_t blocks = (uint32_t)std::min<unsigned long long>((total + 255u) / 256u, 4096u);
    hipLaunchKernelGGL((k_w_check<T>), dim3(blocks), dim3(256), 0, st, wd, pitch, (uint32_t)m, total, bad);
    HIPCHK(hipGetLastError());
    unsigned long long first_bad;
    flag_fetch(reinterpret_cast<uint32_t*>(&first_bad), reinterpret_cast<const uint32_t*>(bad), st, 2);   // (nothing has been written when a weight is invalid)
    if (first_bad != kWtNoBad) {
        set_err(err, errlen, std::string(who) + ": the weight of signal " + std::to_string(first_bad / m) + ", row " + std::to_string(first_bad % m) +
                                 " is negative or not finite");
        return SS_HIP_EINVAL;
    }
    *Wd = wd;
    *wsd = pitch;
    return SS_HIP_OK;
}

template int weights_on_device<float>(ss_hip_ctx*, const char*, const float*, size_t, ptrdiff_t, const float**, long long*, char*, size_t);
template int weights_on_device<double>(ss_hip_ctx*, const char*, const double*, size_t, ptrdiff_t, const double**, long long*, char*, size_t);

}  // namespace sship

using namespace sship;

extern "C" {

int ss_hip_weighted_top_correlations_f32(ss_hip_ctx* ctx, const float* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const float* W,
                                         ptrdiff_t w_stride, const void* records, uint32_t kmax, double min_visible, uint32_t k, uint32_t* idx,
                                         float* coef, double* score, char* err, size_t errlen)
{
    return wtop_entry<float>(ctx, { "weighted_top_correlations", Y, B, y_stride, incy, records, kmax, k, idx, coef, score, err, errlen }, W, w_stride,
                             min_visible);
}
int ss_hip_weighted_top_correlations_f64(ss_hip_ctx* ctx, const double* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const double* W,
                                         ptrdiff_t w_stride, const void* records, uint32_t kmax, double min_visible, uint32_t k, uint32_t* idx,
                                         double* coef, double* score, char* err, size_t errlen)
{
    return wtop_entry<double>(ctx, { "weighted_top_correlations", Y, B, y_stride, incy, records, kmax, k, idx, coef, score, err, errlen }, W, w_stride,
                              min_visible);
}

int ss_hip_weighted_refit_records_f32(ss_hip_ctx* ctx, const float* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const float* W,
                                      ptrdiff_t w_stride, const void* records, uint32_t kmax, void* records_out, double* resnorm,
                                      uint32_t* status, char* err, size_t errlen)
{
    return refit_weighted<float>(ctx, Y, B, y_stride, incy, W, w_stride, records, kmax, records_out, resnorm, status, err, errlen);
}
int ss_hip_weighted_refit_records_f64(ss_hip_ctx* ctx, const double* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const double* W,
                                      ptrdiff_t w_stride, const void* records, uint32_t kmax, void* records_out, double* resnorm,
                                      uint32_t* status, char* err, size_t errlen)
{
    return refit_weighted<double>(ctx, Y, B, y_stride, incy, W, w_stride, records, kmax, records_out, resnorm, status, err, errlen);
}

int ss_hip_weighted_class_residuals_f32(ss_hip_ctx* ctx, const float* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const float* W,
                                        ptrdiff_t w_stride, const void* records, uint32_t kmax, float* R, ptrdiff_t r_stride, uint32_t* best,
                                        double* sci, char* err, size_t errlen)
{
    return class_residuals_weighted<float>(ctx, Y, B, y_stride, incy, W, w_stride, records, kmax, R, r_stride, best, sci, err, errlen);
}
int ss_hip_weighted_class_residuals_f64(ss_hip_ctx* ctx, const double* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const double* W,
                                        ptrdiff_t w_stride, const void* records, uint32_t kmax, double* R, ptrdiff_t r_stride, uint32_t* best,
                                        double* sci, char* err, size_t errlen)
{
    return class_residuals_weighted<double>(ctx, Y, B, y_stride, incy, W, w_stride, records, kmax, R, r_stride, best, sci, err, errlen);
}

}  // extern "C"
