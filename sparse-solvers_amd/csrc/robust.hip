// robust.hip — row weights from record residuals, the step between two codings of a robust (IRLS-style) coder (include/ss_hip.h):
//   ss_hip_robust_weights_*.
//
// The weighted calls (weighted.hip, wdictlearn.hip) take a weight per row and signal; this call makes them on the device from what a
// coding left over: r_b = y_b - A x_b from the records, a scale per signal from the median of |r_b| (the MAD about zero), and a
// loss's weight factor per row, times the caller's PRIOR weights (a known mask, a confidence).  A stays on the device and only the
// records' columns are read.  The host side is the driver of the top correlations (tc_driver.h) with a variant that selects nothing
// (k == 0: no dot block, no idx / coef / score): the record check, the residual block, the chunking and the arena are that driver's.
// Kernels, per chunk of signals:
//
//   (tc_launch_residual_block, by the driver)   R[b][0 .. ldm) = the residual of ss_hip_top_correlations_*, word for word.
//   k_rb_weights  one workgroup of 256 threads per signal.  A truncated record (K > kmax) leaves first: its row of R was not written.
//                 The VISIBLE rows — prior weight > 0 and r finite, k < m — are counted; the element of rank (v - 1) / 2 of |r| over
//                 them is found by a radix selection on the bits of |r| (non-negative IEEE words order as integers): eight bits a
//                 pass from the top, an LDS histogram of integer counts, the bin that holds the rank by a prefix sum over the 256
//                 bins — four passes in fp32, eight in fp64, no arithmetic on the values, so the median is a stored word.  One pass
//                 then writes W_out, resid and scale.  REG (ldm <= 256 * 32): a thread keeps the words of its rows — the bits of |r|,
//                 or the word that marks a row as not visible — in registers across the passes; above that every pass reads the
//                 block again, which was just written.  Caller rows (W, W_out, resid) are read and written as scalars: their
//                 strides need not be 16-byte aligned.
//
// ORDER (build flag -ffp-contract=off: products and sums are rounded separately):
//   r_kb         tc_launch_residual_block's words; rows m .. ldm - 1 take no part anywhere.
//   med_b        the word of rank (v - 1) / 2, 0-based and ascending, of |r_kb| over the visible rows; 0 for v == 0.
//   sigma_b      = max(1.4826022185056018 * (double)med_b, sigma_min): one multiplication, one comparison.  t = tuning * sigma_b.
//   f            with a = |(double)r_kb|, by comparisons first: 0 for a row that is not visible; Huber: a <= t -> 1, else (T)(t / a);
//                Tukey: a == 0 -> 1, a < t -> u = a / t, q = 1 - u * u, (T)(q * q), else 0; cutoff: a <= t -> 1, else 0.
//   W_out        = f * prior, one multiplication in T; f itself without a prior.
// No floating-point atomics: the histogram's counts are integers and commute.  Row b of the outputs is a function of (A, y_b,
// prior_b, record b, loss, tuning, sigma_min) alone: nothing depends on B, on the chunking, on where the pointers live, on w_stride
// == 0 against repeated rows, or on what the context did before.  The unit keeps no buffer of its own: the workspace is the top
// correlations' arena, a host caller's prior is staged where the weighted calls stage theirs.
#include "ss_hip_internal.h"
#include "tc_driver.h"

#include <cmath>
#include <limits>

namespace sship {

namespace {

constexpr uint32_t kRbRegs = 32;                         // rows a thread keeps in registers: ldm <= 256 * kRbRegs
constexpr double kRbMad = 1.4826022185056018;            // 1 / Phi^-1(3/4): the MAD of a normal sample -> its sigma

// the bits of |v| as an unsigned integer; kNone: the word of a row that is not visible (no |v| has it: a NaN with every bit set)
template <typename T> struct RbWord;
template <> struct RbWord<float> {
    typedef uint32_t U;
    static constexpr int kTop = 24;
    static constexpr U kInf = 0x7f800000u, kNone = 0xffffffffu;
    __device__ static U abs_bits(float v) { return __float_as_uint(v) & 0x7fffffffu; }
    __device__ static float value(U u) { return __uint_as_float(u); }
};
template <> struct RbWord<double> {
    typedef unsigned long long U;
    static constexpr int kTop = 56;
    static constexpr U kInf = 0x7ff0000000000000ull, kNone = 0xffffffffffffffffull;
    __device__ static U abs_bits(double v) { return (U)__double_as_longlong(v) & 0x7fffffffffffffffull; }
    __device__ static double value(U u) { return __longlong_as_double((long long)u); }
};

// ---- kernel --------------------------------------------------------------------------------------------------------------------

// R: [chunk][ldm]; rec: the chunk's first record (nullptr: none); W: the chunk's prior weights (row b at W[b * w_stride]; nullptr:
// every weight 1); Wout / resid / scale: the chunk's rows of the outputs (resid, scale may be nullptr)
template <typename T, bool REG>
__global__ __launch_bounds__(256)
void k_rb_weights(const T* __restrict__ R, uint32_t m, uint32_t ldm, const unsigned char* __restrict__ rec, size_t rb, uint32_t kmax, const T* W,
                  long long w_stride, uint32_t loss, double tuning, double sigma_min, T* Wout, long long wo_stride, T* resid, long long r_stride,
                  double* __restrict__ scale)
{
    typedef RbWord<T> X;
    typedef typename X::U U;
    __shared__ uint32_t s_hist[256];
    __shared__ uint32_t s_wave[4];
    __shared__ uint32_t s_pick[2];
    const uint32_t b = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const T* r = R + (size_t)b * ldm;
    const T* w = W ? W + (long long)b * w_stride : nullptr;
    T* wo = Wout + (long long)b * wo_stride;
    T* ro = resid ? resid + (long long)b * r_stride : nullptr;

    if (rec && *reinterpret_cast<const uint32_t*>(rec + (size_t)b * rb) > kmax) {
        // a truncated record does not hold its support, and its row of R holds what the workspace held: the prior passes through
        for (uint32_t k = tid; k < m; k += 256u) {
            wo[k] = w ? w[k] : T(1);
            if (ro) ro[k] = T(0);
        }
        if (tid == 0 && scale) scale[b] = std::numeric_limits<double>::quiet_NaN();
        return;
    }

    // the word of row k: the bits of |r|, kNone for a row that is not visible
    auto word = [&](uint32_t k) -> U {
        const U a = X::abs_bits(r[k]);
        const bool visible = a < X::kInf && (!w || w[k] > T(0));
        return visible ? a : X::kNone;
    };
    U key[REG ? kRbRegs : 1u];
    uint32_t cnt = 0;
    if constexpr (REG) {
#pragma unroll
        for (uint32_t j = 0; j < kRbRegs; ++j) {
            const uint32_t k = tid + 256u * j;
            key[j] = k < m ? word(k) : X::kNone;
            cnt += key[j] != X::kNone ? 1u : 0u;
        }
    } else {
        key[0] = X::kNone;
        for (uint32_t k = tid; k < m; k += 256u) cnt += word(k) != X::kNone ? 1u : 0u;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane == 0) s_wave[wave] = cnt;
    __syncthreads();
    const uint32_t v = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];

    // ---- radix selection: P = the bits above `shift` of the word of rank q as far as they are known; q counts within P's rows ----
    U P = 0;
    uint32_t q = v ? (v - 1u) >> 1 : 0u;
    if (v) {
        for (int shift = X::kTop; shift >= 0; shift -= 8) {
            s_hist[tid] = 0u;
            __syncthreads();
            auto vote = [&](U a) {
                if (a != X::kNone && (shift == X::kTop || (a >> (shift + 8)) == P)) atomicAdd(&s_hist[(uint32_t)(a >> shift) & 255u], 1u);
            };
            if constexpr (REG) {
#pragma unroll
                for (uint32_t j = 0; j < kRbRegs; ++j) vote(key[j]);
            } else {
                for (uint32_t k = tid; k < m; k += 256u) vote(word(k));
            }
            __syncthreads();
            // the bin that holds rank q: the one whose rows begin at or before q and end behind it (inclusive prefix sums of the counts)
            const uint32_t c = s_hist[tid];
            uint32_t inc = c;
#pragma unroll
            for (uint32_t o = 1; o < 64u; o <<= 1) {
                const uint32_t t = __shfl_up(inc, o);
                if (lane >= o) inc += t;
            }
            if (lane == 63u) s_wave[wave] = inc;
            __syncthreads();
            for (uint32_t x = 0; x < wave; ++x) inc += s_wave[x];
            if (inc - c <= q && q < inc) { s_pick[0] = tid; s_pick[1] = inc - c; }
            __syncthreads();
            P = (P << 8) | (U)s_pick[0];
            q -= s_pick[1];
        }
    }
    const double sm = kRbMad * (double)X::value(P);
    const double sigma = sm > sigma_min ? sm : sigma_min;
    const double t = tuning * sigma;

    // ---- the weights ----
    auto emit = [&](uint32_t k, U a_bits) {
        T f = T(0);
        if (a_bits != X::kNone) {
            const double a = (double)X::value(a_bits);
            if (loss == SS_HIP_ROBUST_HUBER) f = a <= t ? T(1) : (T)(t / a);
            else if (loss == SS_HIP_ROBUST_TUKEY) {
                if (a == 0.0) f = T(1);
                else if (a < t) {
                    const double u = a / t, s = 1.0 - u * u;
                    f = (T)(s * s);
                }
            } else f = a <= t ? T(1) : T(0);
        }
        wo[k] = w ? f * w[k] : f;
        if (ro) ro[k] = r[k];
    };
    if constexpr (REG) {
#pragma unroll
        for (uint32_t j = 0; j < kRbRegs; ++j) {
            const uint32_t k = tid + 256u * j;
            if (k < m) emit(k, key[j]);
        }
    } else {
        for (uint32_t k = tid; k < m; k += 256u) emit(k, word(k));
    }
    if (tid == 0 && scale) scale[b] = sigma;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------

// the variant of the driver (tc_driver.h): nothing is selected; per chunk the one launch behind the residual block, into the
// caller's rows on the device or into a staging of the chunk's rows that is copied to a host caller
template <typename T> struct RobustVariant {
    const T* Wd;                       // the prior on the device, row pitch wsd (weights_on_device); nullptr: none
    long long wsd;
    uint32_t loss;
    double tuning, sigma_min;
    T* W_out;
    ptrdiff_t wo_stride;
    T* resid;
    ptrdiff_t r_stride;
    double* scale;
    bool wo_dev = false, r_dev = false, s_dev = false;
    T* swo = nullptr;
    T* sr = nullptr;
    double* ss = nullptr;

    // the bytes a signal of a chunk takes: one residual block and no dot block, the partial sums, a host caller's signal and outputs
    size_t signal_bytes(const ss_hip_ctx* ctx, bool y_dev) const
    {
        return tc_signal_bytes<T>(ctx, y_dev, 1, 0) + ((wo_dev ? 0 : 1) + (resid && !r_dev ? 1 : 0)) * ctx->m * sizeof(T) + sizeof(double);
    }
    void carve(const ss_hip_ctx* ctx, Carver& cv, size_t max_sig, size_t, size_t)
    {
        if (!wo_dev) swo = cv.take<T>(max_sig * ctx->m);
        if (resid && !r_dev) sr = cv.take<T>(max_sig * ctx->m);
        if (scale && !s_dev) ss = cv.take<double>(max_sig);
    }
    hipError_t prepare(ss_hip_ctx*, double*) { return hipSuccess; }
    void chunk(ss_hip_ctx* ctx, const TcCall<T>& c, const TcChunk& ch, const TcWork<T>& w)
    {
        hipStream_t st = ctx->stream;
        const size_t m = ctx->m;
        const ptrdiff_t b0 = (ptrdiff_t)ch.b0;
        T* wo = wo_dev ? W_out + b0 * wo_stride : swo;
        T* ro = !resid ? nullptr : r_dev ? resid + b0 * r_stride : sr;
        double* so = !scale ? nullptr : s_dev ? scale + b0 : ss;
        const long long wos = wo_dev ? (long long)wo_stride : (long long)m, rs = r_dev ? (long long)r_stride : (long long)m;
        const T* wd = Wd ? Wd + b0 * wsd : nullptr;
        if (ctx->ldm <= 256u * kRbRegs)
            hipLaunchKernelGGL((k_rb_weights<T, true>), dim3(ch.Bc), dim3(256), 0, st, w.R, (uint32_t)m, ctx->ldm, w.recs, w.rb, c.kmax, wd, wsd, loss,
                               tuning, sigma_min, wo, wos, ro, rs, so);
        else
            hipLaunchKernelGGL((k_rb_weights<T, false>), dim3(ch.Bc), dim3(256), 0, st, w.R, (uint32_t)m, ctx->ldm, w.recs, w.rb, c.kmax, wd, wsd, loss,
                               tuning, sigma_min, wo, wos, ro, rs, so);
        HIPCHK(hipGetLastError());
        if (!wo_dev)
            HIPCHK(hipMemcpy2DAsync(W_out + b0 * wo_stride, (size_t)wo_stride * sizeof(T), swo, m * sizeof(T), m * sizeof(T), ch.Bc, hipMemcpyDeviceToHost, st));
        if (resid && !r_dev)
            HIPCHK(hipMemcpy2DAsync(resid + b0 * r_stride, (size_t)r_stride * sizeof(T), sr, m * sizeof(T), m * sizeof(T), ch.Bc, hipMemcpyDeviceToHost, st));
        if (scale && !s_dev) HIPCHK(hipMemcpyAsync(scale + b0, ss, ch.Bc * sizeof(double), hipMemcpyDeviceToHost, st));
    }
};

template <typename T>
int robust_entry(ss_hip_ctx* ctx, const T* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const T* W, ptrdiff_t w_stride, const void* records,
                 uint32_t kmax, uint32_t loss, double tuning, double sigma_min, T* W_out, ptrdiff_t wo_stride, T* resid, ptrdiff_t r_stride,
                 double* scale, char* err, size_t errlen)
{
    const char* who = "robust_weights";
    // (without records kmax is ignored: the checks see a capacity that passes)
    int rc = check_common<T>(ctx, who, records, false, records ? kmax : 1u, err, errlen);
    if (rc != SS_HIP_OK) return rc;
    if ((rc = clause(!Y || !W_out, who, "Y and W_out must not be null", err, errlen))) return rc;
    if ((rc = clause(incy <= 0 || y_stride <= 0, who, "increments and strides must be positive", err, errlen))) return rc;
    if ((rc = clause(wo_stride < (ptrdiff_t)ctx->m || (resid && r_stride < (ptrdiff_t)ctx->m), who, "wo_stride and r_stride must be at least m", err, errlen)))
        return rc;
    if (W && (rc = weights_check_args(ctx, who, W, w_stride, err, errlen)) != SS_HIP_OK) return rc;
    if ((rc = clause(loss > SS_HIP_ROBUST_CUTOFF, who, "loss must be SS_HIP_ROBUST_HUBER, _TUKEY or _CUTOFF", err, errlen))) return rc;
    if ((rc = clause(!(tuning > 0.0 && std::isfinite(tuning)), who, "tuning must be finite and > 0", err, errlen))) return rc;
    if ((rc = clause(!(sigma_min >= 0.0 && std::isfinite(sigma_min)), who, "sigma_min must be finite and >= 0", err, errlen))) return rc;
    if ((rc = clause(W != nullptr && W == W_out, who, "W_out must not be W", err, errlen))) return rc;
    const TcCall<T> c{ who, Y, B, y_stride, incy, records, kmax, 0u, nullptr, nullptr, nullptr, err, errlen };
    return tc_run(c, [&] {
        HIPCHK(hipSetDevice(ctx->device));
        RobustVariant<T> v{ nullptr, 0, loss, tuning, sigma_min, W_out, wo_stride, resid, r_stride, scale };
        if (W) {
            const int rw = weights_on_device<T>(ctx, who, W, B, w_stride, &v.Wd, &v.wsd, err, errlen);
            if (rw != SS_HIP_OK) return rw;
        }
        v.wo_dev = on_device(W_out);
        v.r_dev = resid && on_device(resid);
        v.s_dev = scale && on_device(scale);
        const bool y_dev = on_device(Y);
        return tc_drive<T>(ctx, c, y_dev, B, tc_uniform_chunks(ctx, B, v.signal_bytes(ctx, y_dev)), v);
    });
}

}  // namespace

}  // namespace sship

using namespace sship;

extern "C" {

int ss_hip_robust_weights_f32(ss_hip_ctx* ctx, const float* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const float* W, ptrdiff_t w_stride,
                              const void* records, uint32_t kmax, uint32_t loss, double tuning, double sigma_min, float* W_out, ptrdiff_t wo_stride,
                              float* resid, ptrdiff_t r_stride, double* scale, char* err, size_t errlen)
{
    return robust_entry<float>(ctx, Y, B, y_stride, incy, W, w_stride, records, kmax, loss, tuning, sigma_min, W_out, wo_stride, resid, r_stride, scale, err,
                               errlen);
}
int ss_hip_robust_weights_f64(ss_hip_ctx* ctx, const double* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const double* W, ptrdiff_t w_stride,
                              const void* records, uint32_t kmax, uint32_t loss, double tuning, double sigma_min, double* W_out, ptrdiff_t wo_stride,
                              double* resid, ptrdiff_t r_stride, double* scale, char* err, size_t errlen)
{
    return robust_entry<double>(ctx, Y, B, y_stride, incy, W, w_stride, records, kmax, loss, tuning, sigma_min, W_out, wo_stride, resid, r_stride, scale,
                                err, errlen);
}

}  // extern "C"
