// blockcode.hip — block-sparse coding: the class top correlations (include/ss_hip.h): ss_hip_class_top_correlations_*.
//
// A query in the span of one subject's training atoms is block-sparse: few classes, many atoms of each.  The call scores a whole
// CLASS of the context's labels (ss_hip_set_classes) by the l2 norm of its atoms' scores against the residual (block OMP, Eldar,
// Kuppinger and Boelcskei 2010; structured SRC, Elhamifar and Vidal 2011), ranks the classes and emits the best ones whole — every
// candidate atom of a class, or none — into rows ss_hip_extend_records_* takes.  It is the transpose of joint.hip: there the norm runs
// over the signals of a group, here over the atoms of a class.  The host side is the driver of the top correlations (tc_driver.h: its
// record check, residual block, norms and the copies of the class rows; the MFMA tile through tc_launch_dots).  This unit supplies the
// variant — a row a signal (tc_uniform_chunks), a class-score row and the atom rows to carve, what runs on a chunk behind the dots and
// the copies of the atom rows — and the inverted index of the labels.  What runs behind the dots (256 threads each):
//
//   k_bc_scores   grid = (block of 256 classes, signal).  The record's index list goes into LDS; a column is tested against it by index
//                 (binary search: a record's list ascends; a caller's list that does not is searched linearly).  A lane owns a class and
//                 walks that class's columns in ascending order — the serial chain is the definition; the lanes of a wave own
//                 consecutive classes, so with contiguous classes a wave's reads cover one contiguous span of the signal's row of D
//                 and hit in L1 / L2.  It writes the class-score row [num_classes] in double, a NaN word for a class without a
//                 candidate atom.  D is not struck into.  A very large class is a long chain on one lane.
//   (selection)   one workgroup per signal: tc_select.h's selection (tc_select_sorted: its total order, list, tie branch and prefix
//                 property) over the stored class scores.  That is joint.hip's k_js_select word for word — a row of stored scores in
//                 double, a NaN word for no candidate — so it is launched (js_launch_select), not stated again: two kernels select.
//   k_bc_emit     one workgroup per signal: the emission rule — integer logic on the ranked classes — and coef from D and rn.
//
// ORDER (stated once; build flag -ffp-contract=off: products and sums are rounded separately):
//   r_b, dot(i, b), d_i, rn_i   topcorr.hip's words (its ORDER block): the same kernels on the same rows.
//   t(i, b)      = |dot(i, b)| * rn_i, dot widened to double: one multiplication — topcorr.hip's score word.
//   candidates   of signal b: the columns i < n with d_i finite and non-zero that record b does not store (by index, never by a
//                multiplication by zero or by the value of a dot); a truncated record (K > kmax) has none.
//   q(c, b)      = sum t(i, b) * t(i, b) over the candidate atoms of class c: one accumulator, started at 0, the columns in ascending
//                index; each product and each sum rounded on its own.  s(c, b) = sqrt(q(c, b)): one square root.
//   selection    the classes with at least one candidate atom whose score is not a NaN, a maximum under a total order (score
//                descending, class ascending): tc_select.h.  No floating-point atomics.
//   emission     room = width (with records: min(width, kmax - K)); the ranked classes in order, a class whole — its candidate atoms in
//                ascending index — while they fit what is left of the room; the first class that does not fit ends the row (no later,
//                smaller class jumps the queue); taken = the classes emitted.
//   coef         = (T)((double)dot * (rn_i * rn_i)): topcorr.hip's coef of that column and signal.
//   A CLASS OF ONE atom has s = sqrt(fl(t * t)) = t in binary round-to-nearest as long as t * t neither underflows nor overflows (t
//   between 2^-511 and 2^511 is safe): with every class a single atom the call returns top_correlations' words.
// A signal's rows depend on A, the labels, its own signal and record, k and width: not on B, on the chunking (a row of D and a row of
// class scores are functions of their own signal), on where the pointers live or on what the context did before.
#include "ss_hip_internal.h"
#include "tc_driver.h"

#include <algorithm>
#include <cmath>

namespace sship {

namespace {

// The inverted index of the labels (ss_hip_ctx::bc): off [C + 1], cols [n] — the columns of class c, ascending, at cols[off[c] ..
// off[c + 1]).  Its content is a function of the labels alone.  Built once after each ss_hip_set_classes (classify_generation), by a
// counting sort on a host copy of the labels; its memory is the state's own, released with the context
struct ClassIndex {
    Holdings own;
    uint32_t* off = nullptr;
    uint32_t* cols = nullptr;
    uint32_t C = 0;
    uint64_t generation = 0;           // of the labels it was built from; 0: none
};

const ClassIndex& class_index(ss_hip_ctx* ctx)
{
    ClassIndex& ix = part<ClassIndex>(ctx->bc);
    const uint64_t gen = classify_generation(ctx);
    if (ix.generation == gen && ix.off) return ix;
    hipStream_t st = ctx->stream;
    const size_t n = ctx->n;
    const uint32_t C = classify_num_classes(ctx);
    std::vector<uint32_t> lab(n), hoff((size_t)C + 1, 0u), hcols(n);
    HIPCHK(hipMemcpyAsync(lab.data(), classify_labels(ctx), n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (size_t i = 0; i < n; ++i) hoff[(size_t)lab[i] + 1] += 1u;               // (labels < C: ss_hip_set_classes)
    for (size_t c = 0; c < C; ++c) hoff[c + 1] += hoff[c];
    std::vector<uint32_t> next(hoff.begin(), hoff.end() - 1);
    for (size_t i = 0; i < n; ++i) hcols[next[lab[i]]++] = (uint32_t)i;          // (ascending i: every class's columns ascend)
    ix.generation = 0;
    HIPCHK(ix.own.drop(ix.off));
    HIPCHK(ix.own.drop(ix.cols));
    HELD(ix.own, hipMalloc, &ix.off, ((size_t)C + 1) * sizeof(uint32_t));
    HELD(ix.own, hipMalloc, &ix.cols, n * sizeof(uint32_t));
    HIPCHK(hipMemcpyAsync(ix.off, hoff.data(), ((size_t)C + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ix.cols, hcols.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    ix.C = C;
    ix.generation = gen;
    return ix;
}

// ---- kernels -------------------------------------------------------------------------------------------------------------------

// The record of signal b, staged by the whole workgroup (256): s_idx [K] its stored columns, *s_unsorted != 0 when the list does
// not ascend strictly.  -> K (0 without records); trunc: a truncated record (nothing is staged).  Every condition is uniform
__device__ inline uint32_t bc_stage_record(const unsigned char* __restrict__ rec, size_t rb, uint32_t kmax, uint32_t b, uint32_t* s_idx,
                                           uint32_t* s_unsorted, bool& trunc)
{
    const uint32_t tid = threadIdx.x;
    trunc = false;
    if (tid == 0) *s_unsorted = 0u;
    if (!rec) { __syncthreads(); return 0u; }
    const unsigned char* r = rec + (size_t)b * rb;
    const uint32_t K = *reinterpret_cast<const uint32_t*>(r);
    if (K > kmax) { trunc = true; __syncthreads(); return 0u; }
    const uint32_t* idx = reinterpret_cast<const uint32_t*>(r + 16);
    for (uint32_t e = tid; e < K; e += 256u) s_idx[e] = idx[e];
    __syncthreads();
    for (uint32_t e = tid; e + 1u < K; e += 256u)
        if (s_idx[e] >= s_idx[e + 1u]) *s_unsorted = 1u;         // (every thread that writes writes the same word)
    __syncthreads();
    return K;
}

// does the staged record store column i?  By index alone
__device__ inline bool bc_stored(const uint32_t* s_idx, uint32_t K, bool sorted, uint32_t i)
{
    if (sorted) {
        uint32_t lo = 0, hi = K;
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (s_idx[mid] < i) lo = mid + 1u; else hi = mid;
        }
        return lo < K && s_idx[lo] == i;
    }
    for (uint32_t e = 0; e < K; ++e)
        if (s_idx[e] == i) return true;
    return false;
}

// D: the chunk's dots; rec: the chunk's first record, nullptr: no records; S: the chunk's class-score rows [signals][C]
template <typename T>
__global__ __launch_bounds__(256)
void k_bc_scores(const T* __restrict__ D, uint32_t n_pad, const double* __restrict__ rinv, const unsigned char* __restrict__ rec, size_t rb,
                 uint32_t kmax, const uint32_t* __restrict__ off, const uint32_t* __restrict__ cols, uint32_t C, double* __restrict__ S)
{
    extern __shared__ uint32_t s_bc_idx[];                      // [kmax] with records
    __shared__ uint32_t s_unsorted;
    const uint32_t b = blockIdx.y, c = blockIdx.x * 256u + threadIdx.x;
    bool trunc;
    const uint32_t K = bc_stage_record(rec, rb, kmax, b, s_bc_idx, &s_unsorted, trunc);
    if (c >= C) return;
    const bool sorted = s_unsorted == 0u;
    double s = tc_nan(0.0);
    if (!trunc) {
        const T* d = D + (size_t)b * n_pad;
        const uint32_t hi = off[c + 1u];
        uint32_t j = off[c], cnt = 0u;
        double q = 0.0;
        // a candidate atom's term enters the one accumulator; an excluded or stored column is passed over by index
        auto add = [&](uint32_t i, double r, T x) {
            if (r != 0.0 && !bc_stored(s_bc_idx, K, sorted, i)) {
                const double t = fabs((double)x) * r;
                q += t * t;
                cnt += 1u;
            }
        };
        for (; j + 4u <= hi; j += 4u) {                          // four columns' loads in flight, added in ascending order
            const uint32_t i0 = cols[j], i1 = cols[j + 1u], i2 = cols[j + 2u], i3 = cols[j + 3u];
            const double r0 = rinv[i0], r1 = rinv[i1], r2 = rinv[i2], r3 = rinv[i3];
            const T x0 = d[i0], x1 = d[i1], x2 = d[i2], x3 = d[i3];
            add(i0, r0, x0);
            add(i1, r1, x1);
            add(i2, r2, x2);
            add(i3, r3, x3);
        }
        for (; j < hi; ++j) {
            const uint32_t i = cols[j];
            add(i, rinv[i], d[i]);
        }
        if (cnt != 0u) s = sqrt(q);
    }
    S[(size_t)b * C + c] = s;
}

// ocls: the chunk's ranked classes [signals][k]; oidx / ocoef: the chunk's atom rows [signals][width]; otaken [signals]
template <typename T>
__global__ __launch_bounds__(256)
void k_bc_emit(const T* __restrict__ D, uint32_t n_pad, const double* __restrict__ rinv, const unsigned char* __restrict__ rec, size_t rb,
               uint32_t kmax, const uint32_t* __restrict__ off, const uint32_t* __restrict__ cols, uint32_t k, uint32_t width,
               const uint32_t* __restrict__ ocls, uint32_t* __restrict__ oidx, T* __restrict__ ocoef, uint32_t* __restrict__ otaken)
{
    extern __shared__ uint32_t s_bc_idx[];
    __shared__ uint32_t s_unsorted, s_wcnt[4];
    const uint32_t b = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    bool trunc;
    const uint32_t K = bc_stage_record(rec, rb, kmax, b, s_bc_idx, &s_unsorted, trunc);
    const bool sorted = s_unsorted == 0u;
    const T* d = D + (size_t)b * n_pad;
    ocls += (size_t)b * k;
    oidx += (size_t)b * width;
    ocoef += (size_t)b * width;
    uint32_t room = width;
    if (rec) room = trunc ? 0u : (kmax - K < width ? kmax - K : width);

    // One pass over a class's columns, cols[lo .. hi), in ascending blocks of 256 -> the number of its candidate atoms; with `write` they
    // are entered from position `at` on, in ascending index.  Every thread of the workgroup calls it and receives the same count
    auto pass = [&](uint32_t lo, uint32_t hi, bool write, uint32_t at) -> uint32_t {
        uint32_t total = 0u;
        for (uint32_t base = lo; base < hi; base += 256u) {
            const uint32_t j = base + tid;
            uint32_t i = 0u;
            double r = 0.0;
            bool mine = false;
            if (j < hi) {
                i = cols[j];
                r = rinv[i];
                mine = r != 0.0 && !bc_stored(s_bc_idx, K, sorted, i);
            }
            const unsigned long long mask = __ballot(mine);
            if (lane == 0u) s_wcnt[wave] = (uint32_t)__popcll(mask);
            __syncthreads();
            uint32_t before = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull)), all = 0u;
            for (uint32_t w = 0; w < 4u; ++w) { if (w < wave) before += s_wcnt[w]; all += s_wcnt[w]; }
            if (write && mine) {
                oidx[at + total + before] = i;                   // (at + the class's candidates <= room <= width: checked by the caller)
                ocoef[at + total + before] = (T)((double)d[i] * (r * r));
            }
            total += all;
            __syncthreads();
        }
        return total;
    };

    uint32_t used = 0u, taken = 0u;
    for (uint32_t t = 0; t < k; ++t) {                           // (every condition below is uniform across the workgroup)
        const uint32_t c = ocls[t];
        if (c == kTcNone) break;
        const uint32_t lo = off[c], hi = off[c + 1u];
        const uint32_t Lc = pass(lo, hi, false, 0u);
        if (Lc > room - used) break;                             // the prefix rule: the first class that does not fit ends the row
        (void)pass(lo, hi, true, used);
        used += Lc;
        taken += 1u;
    }
    for (uint32_t e = used + tid; e < width; e += 256u) { oidx[e] = kTcNone; ocoef[e] = T(0); }
    if (tid == 0) otaken[b] = taken;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------

// the variant of the driver (tc_driver.h): a chunk's rows are its signals; a class-score row a signal and, for a call that emits, the
// atom rows; rn_i; per chunk the dots, the class scores, their selection, the emission and the copies of the atom rows.  The class
// rows (cls, score) are the driver's idx and score rows, which it copies out
template <typename T> struct BlockVariant {
    const ClassIndex& ix;
    uint32_t width;                    // 0: a ranking-only call
    uint32_t* idx;                     // the caller's, each may be null
    T* coef;
    uint32_t* taken;
    double* S = nullptr;
    uint32_t *ai = nullptr, *at = nullptr;
    T* ac = nullptr;

    void carve(const ss_hip_ctx*, Carver& cv, size_t max_sig, size_t, size_t)
    {
        S = cv.take<double>(max_sig * ix.C);
        ai = cv.take<uint32_t>(max_sig * width);
        ac = cv.take<T>(max_sig * width);
        at = cv.take<uint32_t>(width ? max_sig : 0);
    }
    hipError_t prepare(ss_hip_ctx* ctx, double* rinv) { return coh_launch_norms<T>(ctx, rinv); }
    void chunk(ss_hip_ctx* ctx, const TcCall<T>& c, const TcChunk& ch, const TcWork<T>& w)
    {
        hipStream_t st = ctx->stream;
        const uint32_t n_pad = ctx->n_pad, k = c.k, C = ix.C;
        const size_t o = ch.b0 * k, lds = w.recs ? (size_t)c.kmax * sizeof(uint32_t) : 0;
        HIPCHK(tc_launch_dots<T>(ctx, w.R, ch.Bc, w.D));
        hipLaunchKernelGGL((k_bc_scores<T>), dim3((C + 255u) / 256u, ch.Bc), dim3(256), lds, st, (const T*)w.D, n_pad, w.norms, w.recs, w.rb, c.kmax,
                           (const uint32_t*)ix.off, (const uint32_t*)ix.cols, C, S);
        HIPCHK(hipGetLastError());
        HIPCHK(js_launch_select(ctx, S, ch.Bc, C, C, k, w.oi + o, w.os + o));
        if (width == 0) return;
        hipLaunchKernelGGL((k_bc_emit<T>), dim3(ch.Bc), dim3(256), lds, st, (const T*)w.D, n_pad, w.norms, w.recs, w.rb, c.kmax, (const uint32_t*)ix.off,
                           (const uint32_t*)ix.cols, k, width, (const uint32_t*)(w.oi + o), ai, ac, at);
        HIPCHK(hipGetLastError());
        const size_t rows = (size_t)ch.Bc * width;
        HIPCHK(hipMemcpyAsync(idx + ch.b0 * width, ai, rows * sizeof(uint32_t), hipMemcpyDefault, st));
        if (coef) HIPCHK(hipMemcpyAsync(coef + ch.b0 * width, ac, rows * sizeof(T), hipMemcpyDefault, st));
        if (taken) HIPCHK(hipMemcpyAsync(taken + ch.b0, at, (size_t)ch.Bc * sizeof(uint32_t), hipMemcpyDefault, st));
    }
};

// c.idx / c.score: the caller's cls and score (the driver's rows); idx, coef, taken: the caller's atom rows
template <typename T>
int block_topcorr_entry(ss_hip_ctx* ctx, const TcCall<T>& c, uint32_t width, uint32_t* idx, T* coef, uint32_t* taken)
{
    // top_correlations' checks in their order (tc_check_call), with the null clause in this call's words in front of the driver's
    int rc = check_common<T>(ctx, c.who, c.records, false, c.records ? c.kmax : 1u, c.err, c.errlen);
    if (rc != SS_HIP_OK) return rc;
    if ((rc = clause(!c.Y || !c.idx, c.who, "Y and cls must not be null", c.err, c.errlen)) != SS_HIP_OK) return rc;
    if ((rc = tc_check_call<T>(ctx, c)) != SS_HIP_OK) return rc;
    if ((rc = clause(classify_num_classes(ctx) == 0, c.who, "no classes set (ss_hip_set_classes)", c.err, c.errlen)) != SS_HIP_OK) return rc;
    if ((rc = clause(!idx && (coef || taken), c.who, "coef and taken need idx", c.err, c.errlen)) != SS_HIP_OK) return rc;
    if (idx && (width == 0 || width > (uint32_t)SS_HIP_TOPCORR_KMAX)) {
        set_err(c.err, c.errlen, std::string(c.who) + ": width must be 1.." + std::to_string(SS_HIP_TOPCORR_KMAX));
        return SS_HIP_EINVAL;
    }
    return tc_run(c, [&] {
        HIPCHK(hipSetDevice(ctx->device));
        const ClassIndex& ix = class_index(ctx);
        const bool y_dev = on_device(c.Y);
        BlockVariant<T> v{ ix, idx ? width : 0u, idx, coef, taken };
        // §3.13h's bytes a signal plus its class-score row
        const size_t per = tc_signal_bytes<T>(ctx, y_dev, 1) + (size_t)ix.C * sizeof(double);
        return tc_drive<T>(ctx, c, y_dev, c.B, tc_uniform_chunks(ctx, c.B, per), v);
    });
}

}  // namespace

}  // namespace sship

using namespace sship;

extern "C" {

int ss_hip_class_top_correlations_f32(ss_hip_ctx* ctx, const float* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const void* records,
                                      uint32_t kmax, uint32_t k, uint32_t width, uint32_t* cls, double* score, uint32_t* idx, float* coef,
                                      uint32_t* taken, char* err, size_t errlen)
{
    return block_topcorr_entry<float>(ctx, { "class_top_correlations", Y, B, y_stride, incy, records, kmax, k, cls, nullptr, score, err, errlen }, width, idx,
                                      coef, taken);
}
int ss_hip_class_top_correlations_f64(ss_hip_ctx* ctx, const double* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const void* records,
                                      uint32_t kmax, uint32_t k, uint32_t width, uint32_t* cls, double* score, uint32_t* idx, double* coef,
                                      uint32_t* taken, char* err, size_t errlen)
{
    return block_topcorr_entry<double>(ctx, { "class_top_correlations", Y, B, y_stride, incy, records, kmax, k, cls, nullptr, score, err, errlen }, width,
                                       idx, coef, taken);
}

}  // extern "C"
