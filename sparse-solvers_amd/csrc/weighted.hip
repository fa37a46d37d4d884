// weighted.hip — coding under a non-negative weight per row and signal, min sum_k w_kb (y_b - A x)_k^2 (include/ss_hip.h):
//   ss_hip_weighted_top_correlations_*, ss_hip_weighted_refit_records_*, ss_hip_weighted_class_residuals_*.
//
// A 0/1 mask of observed rows (occlusion, inpainting) is the special case; robust coders supply the weights from the previous
// residual.  A is shared by the batch and the weights are not: the atom norms become d(i, b) = sum_k w_kb a_ki^2, one per atom and
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
//   k_w_norms    one wave per column: d_i = sum_k a_ki^2 in double — k_coh_norms' statements and words (coherence.hip), stored as
//                d_i itself (0 for an excluded column: d_i zero or not finite, or i >= n): the visible share needs d_i, not rn_i.
//   k_w_apply    one workgroup per signal: Wb[b][k] = w_kb (0 from row m on), R[b][k] = w_kb * r_kb in place — one multiplication in
//                T — and wmax_b = max_k w_kb (a maximum: any order gives the same word).
//   k_tc_tile    twice (tc_launch_dots, tc_launch_weight_dots): D = A^T (w o r), D2 = (A o A)^T w, both [chunk][n_pad] in T.
//   k_w_select   one workgroup per signal: the record's columns struck out by index, the key of a candidate formed in double from
//                the stored words, tc_select.h's selection.
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
#include "record_common.h"
#include "tc_select.h"

#include <algorithm>
#include <cmath>
#include <limits>

namespace sship {

namespace {

constexpr unsigned long long kWtNoBad = ~0ull;

struct WeightedState {
    unsigned char* wbuf = nullptr;     // per call: the first-offender word, then a host caller's weights
    size_t wbuf_bytes = 0;
    unsigned char* buf = nullptr;      // top correlations — per call: d_i, staged records and outputs; per chunk: residuals, weights, both dot blocks
    size_t bytes = 0;
};

WeightedState* state_of(ss_hip_ctx* ctx)
{
    if (!ctx->wt) ctx->wt = new WeightedState();
    return static_cast<WeightedState*>(ctx->wt);
}

__device__ inline float wt_nan(float) { return __int_as_float(0x7fc00000); }
__device__ inline double wt_nan(double) { return __longlong_as_double(0x7ff8000000000000ll); }

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

// k_coh_norms' statements (coherence.hip), the sum stored instead of its inverse root
template <typename T>
__global__ __launch_bounds__(256)
void k_w_norms(const T* __restrict__ At, uint32_t ldm, uint32_t m, uint32_t n, uint32_t n_pad, double* __restrict__ dn)
{
    const uint32_t lane = threadIdx.x & 63u, i = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (i >= n_pad) return;
    double s = 0.0;
    if (i < n) {
        const T* a = At + (size_t)i * ldm;
        for (uint32_t k = lane; k < m; k += 64u) { const double v = (double)a[k]; s = s + v * v; }
    }
    s = wave_sum(s);
    if (lane == 0) dn[i] = (i < n && s > 0.0 && s <= 1.7976931348623157e308) ? s : 0.0;
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

// D, D2: the chunk's two dot blocks, row b of D is this workgroup's to strike columns out of; rec == nullptr: no records
template <typename T>
__global__ __launch_bounds__(256)
void k_w_select(T* __restrict__ D, const T* __restrict__ D2, uint32_t n, uint32_t n_pad, const double* __restrict__ dn,
                const double* __restrict__ wmax, double min_visible, const unsigned char* __restrict__ rec, size_t rb, uint32_t kmax, uint32_t k,
                uint32_t* __restrict__ oidx, T* __restrict__ ocoef, double* __restrict__ oscore)
{
    __shared__ TcSelectLds lds;
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    T* d = D + (size_t)b * n_pad;
    const T* d2 = D2 + (size_t)b * n_pad;
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
        for (uint32_t e = tid; e < K; e += 256u) d[idx[e]] = wt_nan(T(0));        // (idx < n: tc_launch_record_check)
        __threadfence_block();
        __syncthreads();
    }
    const double wm = wmax[b];
    auto keyof = [&](uint32_t i, unsigned long long& key) -> bool {
        const double di = dn[i];
        if (di == 0.0) return false;
        const double dw = (double)d2[i];
        if (!(dw > 0.0)) return false;
        if (!(dw / (wm * di) > min_visible)) return false;
        const double s = fabs((double)d[i]) / sqrt(dw);
        if (!(s == s)) return false;
        key = (unsigned long long)__double_as_longlong(s);
        return true;
    };
    const uint32_t L = tc_select_sorted(lds, n, k, keyof);
    for (uint32_t t = tid; t < k; t += 256u) {
        if (t < L) {
            const uint32_t i = lds.lidx[t];
            oidx[t] = i;
            ocoef[t] = (T)((double)d[i] / (double)d2[i]);
            oscore[t] = __longlong_as_double((long long)lds.lkey[t]);
        } else {
            oidx[t] = kTcNone;
            ocoef[t] = T(0);
            oscore[t] = 0.0;
        }
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------

bool wt_grow(WeightedState* ws, size_t need, const char* who, char* err, size_t errlen)
{
    try {
        grow(ws->buf, ws->bytes, need, "hipMalloc(weighted top correlations workspace)");
    } catch (const HipFail& f) {
        if (f.code != hipErrorOutOfMemory) throw;
        (void)hipGetLastError();
        set_err(err, errlen, std::string(who) + ": no device memory for a workspace of " + std::to_string(need) + " bytes");
        return false;
    }
    return true;
}

template <typename T>
int wtop_impl(ss_hip_ctx* ctx, const T* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const T* W, ptrdiff_t w_stride, const void* records,
              uint32_t kmax, double min_visible, uint32_t k, uint32_t* idx, T* coef, double* score, char* err, size_t errlen)
{
    static const char* who = "weighted_top_correlations";
    HIPCHK(hipSetDevice(ctx->device));
    WeightedState* ws = state_of(ctx);
    hipStream_t st = ctx->stream;
    const size_t m = ctx->m, rb = records ? record_bytes(kmax, sizeof(T)) : 0;
    const uint32_t ldm = ctx->ldm, n = (uint32_t)ctx->n, n_pad = ctx->n_pad, Bu = (uint32_t)B;
    const uint32_t rtiles = (uint32_t)((m + kClsTileRows - 1) / kClsTileRows);
    const bool rec_dev = records && on_device(records), y_dev = on_device(Y);

    const T* Wd = nullptr;
    long long wsd = 0;
    const int rw = weights_on_device<T>(ctx, who, W, B, w_stride, &Wd, &wsd, err, errlen);
    if (rw != SS_HIP_OK) return rw;

    // the chunk: whole signal tiles under top_correlations' byte budget (two blocks of each kind)
    const size_t per = 2 * (size_t)ldm * sizeof(T) + 2 * (size_t)n_pad * sizeof(T) + (size_t)rtiles * 4u * sizeof(double) + sizeof(double) +
                       (y_dev ? 0 : m * sizeof(T));
    size_t chunk = std::max<size_t>(kTcTile, std::min<size_t>(kTcChunkMax, kTcChunkBytes / per) / kTcTile * kTcTile);
    if (ctx->tc_chunk_max > 0) chunk = std::min<size_t>(chunk, (size_t)ctx->tc_chunk_max);
    chunk = std::min(chunk, B);
    const size_t chunk_pad = (chunk + kTcTile - 1) / kTcTile * kTcTile;

    auto carve = [&](unsigned char* base, auto&& use) {
        Carver cv(base);
        double* dn = cv.take<double>(n_pad);
        uint32_t* bad = cv.take<uint32_t>(1);
        unsigned char* stage = (records && !rec_dev) ? cv.take<unsigned char>(B * rb) : nullptr;
        uint32_t* oi = cv.take<uint32_t>(B * k);
        T* oc = cv.take<T>(B * k);
        double* os = cv.take<double>(B * k);
        T* R = cv.take<T>(chunk_pad * ldm);
        T* Wb = cv.take<T>(chunk_pad * ldm);
        T* D = cv.take<T>(chunk_pad * n_pad);
        T* D2 = cv.take<T>(chunk_pad * n_pad);
        double* wmax = cv.take<double>(chunk);
        double* part = cv.take<double>(chunk * rtiles * 4u);
        T* ybuf = y_dev ? nullptr : cv.take<T>(chunk * m);
        use(dn, bad, stage, oi, oc, os, R, Wb, D, D2, wmax, part, ybuf);
        return cv.off;
    };
    if (!wt_grow(ws, carve(nullptr, [](auto...) {}), who, err, errlen)) return SS_HIP_ENOMEM;

    int rc = SS_HIP_OK;
    carve(ws->buf, [&](double* dn, uint32_t* bad, unsigned char* stage, uint32_t* oi, T* oc, double* os, T* R, T* Wb, T* D, T* D2, double* wmax,
                       double* part, T* ybuf) {
        const unsigned char* din = static_cast<const unsigned char*>(records);
        if (records) {
            if (!rec_dev) { HIPCHK(hipMemcpyAsync(stage, records, B * rb, hipMemcpyHostToDevice, st)); din = stage; }
            HIPCHK(tc_launch_record_check(ctx, din, rb, kmax, Bu, bad));
            uint32_t first_bad = kTcNone;
            HIPCHK(hipMemcpyAsync(&first_bad, bad, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));            // (nothing has been written when a record is invalid)
            if (first_bad != kTcNone) { rc = bad_index(first_bad, who, err, errlen); return; }
        }
        hipLaunchKernelGGL((k_w_norms<T>), dim3(n_pad / 4u), dim3(256), 0, st, static_cast<const T*>(ctx->At), ldm, (uint32_t)m, n, n_pad, dn);
        HIPCHK(hipGetLastError());
        std::vector<T> tmp;
        for (size_t b0 = 0; b0 < B; b0 += chunk) {
            const uint32_t Bc = (uint32_t)std::min(chunk, B - b0), btiles = (Bc + kTcTile - 1u) / kTcTile;
            const T* yd = Y + (ptrdiff_t)b0 * y_stride;
            long long ys = y_stride, yi = incy;
            if (!y_dev) { upload_rows<T>(ctx, ybuf, Y, y_stride, incy, b0, Bc, tmp); yd = ybuf; ys = (long long)m; yi = 1; }
            HIPCHK(tc_launch_residual_block<T>(ctx, yd, ys, yi, records ? din + b0 * rb : nullptr, rb, kmax, Bc, R, part));
            // (the rows behind the chunk's last signal, up to a whole tile, weigh zero as R's are zero: their dots are never read)
            if (btiles * kTcTile != Bc) HIPCHK(hipMemsetAsync(Wb + (size_t)Bc * ldm, 0, (size_t)(btiles * kTcTile - Bc) * ldm * sizeof(T), st));
            hipLaunchKernelGGL((k_w_apply<T>), dim3(Bc), dim3(256), 0, st, Wd + (ptrdiff_t)b0 * wsd, wsd, (uint32_t)m, ldm, R, Wb, wmax);
            HIPCHK(hipGetLastError());
            HIPCHK(tc_launch_dots<T>(ctx, R, Bc, D));
            HIPCHK(tc_launch_weight_dots<T>(ctx, Wb, Bc, D2));
            hipLaunchKernelGGL((k_w_select<T>), dim3(Bc), dim3(256), 0, st, D, (const T*)D2, n, n_pad, (const double*)dn, (const double*)wmax,
                               min_visible, records ? din + b0 * rb : nullptr, rb, kmax, k, oi + b0 * k, oc + b0 * k, os + b0 * k);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipMemcpyAsync(idx, oi, B * k * sizeof(uint32_t), hipMemcpyDefault, st));
        if (coef) HIPCHK(hipMemcpyAsync(coef, oc, B * k * sizeof(T), hipMemcpyDefault, st));
        if (score) HIPCHK(hipMemcpyAsync(score, os, B * k * sizeof(double), hipMemcpyDefault, st));
        HIPCHK(hipStreamSynchronize(st));
    });
    return rc;
}

// top_correlations' checks in its order, then the weights' and min_visible's
template <typename T>
int wtop_entry(ss_hip_ctx* ctx, const T* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const T* W, ptrdiff_t w_stride, const void* records,
               uint32_t kmax, double min_visible, uint32_t k, uint32_t* idx, T* coef, double* score, char* err, size_t errlen)
{
    static const char* who = "weighted_top_correlations";
    // (without records kmax is ignored: the checks see a capacity that passes)
    int rc = check_common<T>(ctx, who, records, false, records ? kmax : 1u, err, errlen);
    if (rc != SS_HIP_OK) return rc;
    if (!Y || !idx) { set_err(err, errlen, "weighted_top_correlations: Y and idx must not be null"); return SS_HIP_EINVAL; }
    if (k == 0 || k > (uint32_t)SS_HIP_TOPCORR_KMAX) {
        set_err(err, errlen, std::string(who) + ": k must be 1.." + std::to_string(SS_HIP_TOPCORR_KMAX));
        return SS_HIP_EINVAL;
    }
    if (incy <= 0 || y_stride <= 0) { set_err(err, errlen, "weighted_top_correlations: increments and strides must be positive"); return SS_HIP_EINVAL; }
    if ((rc = weights_check_args(ctx, who, W, w_stride, err, errlen)) != SS_HIP_OK) return rc;
    if (!(min_visible >= 0.0 && min_visible < 1.0)) { set_err(err, errlen, "weighted_top_correlations: min_visible must lie in [0, 1)"); return SS_HIP_EINVAL; }
    if (B == 0) return SS_HIP_OK;                             // (every argument above was checked all the same)
    if (B >= 0x80000000ull) { set_err(err, errlen, "weighted_top_correlations: B must stay below 2^31"); return SS_HIP_EINVAL; }
    return guarded(err, errlen, who, [&] {
        return wtop_impl<T>(ctx, Y, B, y_stride, incy, W, w_stride, records, kmax, min_visible, k, idx, coef, score, err, errlen);
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
    grow(ws->wbuf, ws->wbuf_bytes, 256 + (w_dev ? 0 : rows * m * sizeof(T)), "hipMalloc(weights)");
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
    HIPCHK(hipMemsetAsync(bad, 0xff, sizeof(unsigned long long), st));
    const unsigned long long total = (unsigned long long)rows * m;
    const uint32_t blocks = (uint32_t)std::min<unsigned long long>((total + 255u) / 256u, 4096u);
    hipLaunchKernelGGL((k_w_check<T>), dim3(blocks), dim3(256), 0, st, wd, pitch, (uint32_t)m, total, bad);
    HIPCHK(hipGetLastError());
    unsigned long long first_bad = kWtNoBad;
    HIPCHK(hipMemcpyAsync(&first_bad, bad, sizeof(first_bad), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));                    // (nothing has been written when a weight is invalid)
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

void weighted_free(ss_hip_ctx* ctx)
{
    WeightedState* ws = static_cast<WeightedState*>(ctx->wt);
    if (!ws) return;
    if (ws->wbuf) (void)hipFree(ws->wbuf);
    if (ws->buf) (void)hipFree(ws->buf);
    delete ws;
    ctx->wt = nullptr;
}

}  // namespace sship

using namespace sship;

extern "C" {

int ss_hip_weighted_top_correlations_f32(ss_hip_ctx* ctx, const float* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const float* W,
                                         ptrdiff_t w_stride, const void* records, uint32_t kmax, double min_visible, uint32_t k, uint32_t* idx,
                                         float* coef, double* score, char* err, size_t errlen)
{
    return wtop_entry<float>(ctx, Y, B, y_stride, incy, W, w_stride, records, kmax, min_visible, k, idx, coef, score, err, errlen);
}
int ss_hip_weighted_top_correlations_f64(ss_hip_ctx* ctx, const double* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const double* W,
                                         ptrdiff_t w_stride, const void* records, uint32_t kmax, double min_visible, uint32_t k, uint32_t* idx,
                                         double* coef, double* score, char* err, size_t errlen)
{
    return wtop_entry<double>(ctx, Y, B, y_stride, incy, W, w_stride, records, kmax, min_visible, k, idx, coef, score, err, errlen);
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
