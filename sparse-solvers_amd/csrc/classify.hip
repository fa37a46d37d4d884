// classify.hip — sparse-representation classification on the device, from compact records (include/ss_hip.h):
//   ss_hip_set_classes, ss_hip_reconstruct_records_*, ss_hip_class_residuals_*, ss_hip_homotopy_classify_batch_*.
//
// A record (ss_hip_homotopy_solve_batch_compact_*) holds the K non-zero coefficients of a solution as (column, value) pairs.  The
// class residual r_c(y) = ||y - A delta_c(x)||_2 needs only the record's columns of class c, and A is stored column-contiguous
// (ctx->At, [n_pad][ldm]): every such column is one contiguous run of ldm elements.  Three kernels per chunk of signals:
//
//   k_cls_prepare   one workgroup per signal.  Reads K, idx[], val[] and each column's class, orders the entries by
//                   (class, position in the record) — a stable counting rank, a function of the record alone — writes the segment
//                   list (class, first entry, count) and, in double from the record's values, the per-class ||delta_c x||_1,
//                   ||x||_1 and the sparsity concentration index.  A column index >= n marks the signal invalid; it is never used
//                   as an address.
//   k_cls_residual  grid = (row tile, signal).  A workgroup of 256 threads holds a tile of 1024 rows of y in registers (thread t:
//                   fp32 rows 4t .. 4t+3 of the tile, fp64 rows 2t, 2t+1 and 512+2t, 512+2t+1: 16-byte loads along a column; rows
//                   m .. ldm-1 of At are zero).  For each segment it forms acc_i = sum_k v_k * A[i][col_k] over the segment's
//                   entries in the prepared order, eight columns' loads in flight, then sums (y_i - acc_i)^2 over the tile.  With
//                   STORE it runs one segment over all entries and stores acc: ss_hip_reconstruct_records_*.
//   k_cls_finish    one workgroup per signal: the tile partials per segment added up, square roots, the row of R, the arg-min.
//
// SUMMATION ORDER (the tests' tolerances follow from it; build flag -ffp-contract=off: products and sums are rounded separately):
//   acc_i      starts at 0 and takes v_k * A[i][col_k] one entry after the other in the prepared order, in the context's precision;
//   d_i        = y_i - acc_i in the context's precision; its square and every sum of squares in double;
//   a thread   adds its four squares in ascending row order;
//   a wave     adds its 64 thread sums by the butterfly lane ^ 32, ^ 16, ^ 8, ^ 4, ^ 2, ^ 1 (every lane ends with the same word);
//   a segment  = the wave sums taken one after the other: tiles ascending, inside a tile waves 0, 1, 2, 3;
//   ||y||_2    the same way from y_i^2;
//   ||delta_c x||_1 = |v| of the segment's entries one after the other in the prepared order; ||x||_1 = those sums one after the other
//              in ascending class order.
// No floating-point atomics; nothing depends on B, on the chunking or on the launch geometry: a signal's words are a function of its
// record, its y, the labels and A.
// The weighted class residuals (ss_hip_weighted_class_residuals_*, weighted.hip) are this unit with a flag: class_residuals_weighted is
// class_residuals_entry with the weights checked and brought to the device, k_cls_residual<T, false, true> multiplies every square
// by (double)w_i before the sums above.  The unflagged instantiations are the code they were.
#include "ss_hip_internal.h"
#include "record_common.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

namespace sship {

namespace {

constexpr uint32_t kClsChunkMax = 1024;                  // most signals per internal chunk ...
constexpr size_t kClsChunkBytes = (size_t)64 << 20;      // ... and the byte budget of a chunk's workspace (never changes a result)
constexpr uint32_t kClsTruncated = 1u, kClsInvalid = 2u; // per-signal flags
constexpr uint32_t kSigWords = 4;                        // per-signal header: K stored, segments, flags, unused

struct ClassifyState {
    Holdings own;                      // the labels
    uint32_t* labels = nullptr;        // [n_pad] class of every column (padding columns: 0)
    uint32_t num_classes = 0;
    uint64_t generation = 0;           // ss_hip_set_classes calls that succeeded: what a derived index was built from (classify_generation)
    WorkArena arena;                   // the workspace of one chunk, carved per call
    WorkArena y_all;                   // classify: the batch's signals, uploaded once (a host Y)
    WorkArena rec_all;                 // classify: the batch's records (the caller's are on the host, or not asked for)
};

ClassifyState* state_of(ss_hip_ctx* ctx)
{
    return &part<ClassifyState>(ctx->cls);
}

// ---- kernels -------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256)
void k_cls_check_labels(const uint32_t* __restrict__ labels, uint32_t n, uint32_t C, uint32_t* __restrict__ bad)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j < n && labels[j] >= C) atomicMin(bad, j);
}

// labels == nullptr: every column in one class (the record's own order: reconstruct_records)
template <typename T>
__global__ __launch_bounds__(256)
void k_cls_prepare(const unsigned char* __restrict__ rec, size_t rb, uint32_t kmax, uint32_t n, const uint32_t* __restrict__ labels,
                   uint32_t C, uint32_t segcap, uint32_t* __restrict__ ord_idx, T* __restrict__ ord_val, uint32_t* __restrict__ seg,
                   double* __restrict__ seg_l1, uint32_t* __restrict__ sig, double* __restrict__ sci, uint32_t* __restrict__ bad,
                   uint32_t b0)
{
    extern __shared__ uint32_t s_mem[];
    uint32_t* s_cls = s_mem;               // [kmax] class of entry e
    uint32_t* s_sorted = s_mem + kmax;     // [kmax] class at prepared position p
    __shared__ uint32_t s_bad, s_nseg;
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    const unsigned char* r = rec + (size_t)b * rb;
    const uint32_t Krec = *reinterpret_cast<const uint32_t*>(r);
    const uint32_t K = Krec < kmax ? Krec : kmax;
    const uint32_t* idx = reinterpret_cast<const uint32_t*>(r + 16);
    const unsigned char* valp = r + 16 + (size_t)kmax * 4;
    ord_idx += (size_t)b * kmax;
    ord_val += (size_t)b * kmax;
    seg += (size_t)b * segcap * 3;
    seg_l1 += (size_t)b * segcap;
    sig += (size_t)b * kSigWords;
    if (tid == 0) { s_bad = 0u; s_nseg = 0u; }
    __syncthreads();
    for (uint32_t e = tid; e < K; e += 256u) {
        const uint32_t col = idx[e];
        uint32_t c = 0u;
        if (col >= n) s_bad = 1u;
        else if (labels) c = labels[col];
        s_cls[e] = c;
    }
    __syncthreads();
    if (s_bad != 0u) {
        if (tid == 0) {
            sig[0] = 0u; sig[1] = 0u; sig[2] = kClsInvalid; sig[3] = 0u;
            sci[b] = __longlong_as_double(0x7ff8000000000000ll);
            atomicMin(bad, b0 + b);
        }
        return;
    }
    // stable rank: entries of a smaller class first, then earlier entries of the same class
    for (uint32_t e = tid; e < K; e += 256u) {
        const uint32_t c = s_cls[e];
        uint32_t pos = 0;
        for (uint32_t j = 0; j < K; ++j) {
            const uint32_t cj = s_cls[j];
            pos += (cj < c || (cj == c && j < e)) ? 1u : 0u;
        }
        s_sorted[pos] = c;
        ord_idx[pos] = idx[e];
        ord_val[pos] = load_val(valp, e, T(0));
    }
    __threadfence_block();
    __syncthreads();
    // segments: the thread of a segment's first position writes it and adds up its |v| in order
    for (uint32_t p = tid; p < K; p += 256u) {
        const uint32_t c = s_sorted[p];
        if (p != 0u && s_sorted[p - 1u] == c) continue;
        uint32_t si = 0;
        for (uint32_t j = 1; j <= p; ++j) si += s_sorted[j] != s_sorted[j - 1u] ? 1u : 0u;
        uint32_t cnt = 1;
        while (p + cnt < K && s_sorted[p + cnt] == c) ++cnt;
        double l1 = 0.0;
        for (uint32_t q = p; q < p + cnt; ++q) l1 += fabs((double)ord_val[q]);
        seg[3u * si] = c; seg[3u * si + 1u] = p; seg[3u * si + 2u] = cnt;
        seg_l1[si] = l1;
        if (p + cnt == K) s_nseg = si + 1u;
    }
    __threadfence_block();
    __syncthreads();
    if (tid == 0) {
        const uint32_t nseg = s_nseg;
        double total = 0.0, mx = 0.0;
        for (uint32_t s = 0; s < nseg; ++s) { const double l = seg_l1[s]; total += l; mx = l > mx ? l : mx; }
        double v;
        if (Krec > kmax) v = __longlong_as_double(0x7ff8000000000000ll);
        else if (!(total > 0.0)) v = 0.0;
        else if (C <= 1u) v = 1.0;
        else v = ((double)C * mx / total - 1.0) / (double)(C - 1u);
        sci[b] = v;
        sig[0] = K; sig[1] = nseg; sig[2] = Krec > kmax ? kClsTruncated : 0u; sig[3] = 0u;
    }
}

// STORE: acc of ONE segment over all stored entries goes to yhat ([signals][ldm]); otherwise the tile's partial sums of squares
// of every segment go to part ([signal][tile][segcap][4 waves]) and those of y to party ([signal][tile][4]).
// WGT (the weighted class residuals, weighted.hip): every square, formed in double as before, is multiplied by (double)w_i — row i of
// the signal's weights Wt[b * w_stride + i], 0 for the rows from m on — before it enters the same sums: sqrt(sum_i w_i d_i^2), and
// ||y||_w for a class without entries.  With w_i == 1 the product is the square itself: the unweighted words.  A class none of
// whose rows is visible reads 0 like any other.  Without WGT nothing is added and Wt is not read.
template <typename T, bool STORE, bool WGT = false>
__global__ __launch_bounds__(256)
void k_cls_residual(const T* __restrict__ At, uint32_t ldm, uint32_t m, const T* __restrict__ Y, long long y_stride, long long incy,
                    const uint32_t* __restrict__ ord_idx, const T* __restrict__ ord_val, uint32_t kmax,
                    const uint32_t* __restrict__ seg, uint32_t segcap, const uint32_t* __restrict__ sig,
                    double* __restrict__ part, double* __restrict__ party, T* __restrict__ yhat, const T* __restrict__ Wt = nullptr,
                    long long w_stride = 0)
{
    typedef typename ClsVec<T>::type V;
    constexpr uint32_t W = ClsVec<T>::W, L = ClsVec<T>::L, U = kClsInFlight;
    const uint32_t tile = blockIdx.x, b = blockIdx.y, ntiles = gridDim.x;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t K = sig[(size_t)b * kSigWords], nseg = sig[(size_t)b * kSigWords + 1u], flags = sig[(size_t)b * kSigWords + 2u];
    ord_idx += (size_t)b * kmax;
    ord_val += (size_t)b * kmax;
    seg += (size_t)b * segcap * 3;
    uint32_t row0[L];
#pragma unroll
    for (uint32_t j = 0; j < L; ++j) row0[j] = tile * kClsTileRows + j * (256u * W) + tid * W;

    T yv[L][W];
    double wv[WGT ? L : 1u][W];
    if (!STORE) {
        const T* y = Y + (long long)b * y_stride;
        double s = 0.0;
#pragma unroll
        for (uint32_t j = 0; j < L; ++j)
#pragma unroll
            for (uint32_t e = 0; e < W; ++e) {
                const uint32_t row = row0[j] + e;
                yv[j][e] = row < m ? y[(long long)row * incy] : T(0);
                if constexpr (WGT) {
                    wv[j][e] = row < m ? (double)Wt[(long long)b * w_stride + row] : 0.0;
                    s += ((double)yv[j][e] * (double)yv[j][e]) * wv[j][e];
                } else {
                    s += (double)yv[j][e] * (double)yv[j][e];
                }
            }
        s = wave_sum(s);
        if (lane == 0u) party[((size_t)b * ntiles + tile) * 4u + wave] = s;
        if (flags != 0u) return;                       // truncated or invalid: k_cls_finish writes NaN
    }
    const uint32_t nsegs = STORE ? (flags & kClsInvalid ? 0u : 1u) : nseg;
    for (uint32_t s = 0; s < nsegs; ++s) {
        const uint32_t first = STORE ? 0u : seg[3u * s + 1u], cnt = STORE ? K : seg[3u * s + 2u];
        T acc[L][W];
#pragma unroll
        for (uint32_t j = 0; j < L; ++j)
#pragma unroll
            for (uint32_t e = 0; e < W; ++e) acc[j][e] = T(0);
        uint32_t k = 0;
        for (; k + U <= cnt; k += U) {                  // U columns' loads in flight, added in order
            V a[U][L];
            T v[U];
#pragma unroll
            for (uint32_t u = 0; u < U; ++u) {
                const T* colp = At + (size_t)ord_idx[first + k + u] * ldm;
                v[u] = ord_val[first + k + u];
#pragma unroll
                for (uint32_t j = 0; j < L; ++j) a[u][j] = row0[j] < ldm ? *reinterpret_cast<const V*>(colp + row0[j]) : V{};
            }
#pragma unroll
            for (uint32_t u = 0; u < U; ++u)
#pragma unroll
                for (uint32_t j = 0; j < L; ++j)
#pragma unroll
                    for (uint32_t e = 0; e < W; ++e) acc[j][e] = acc[j][e] + v[u] * vget(a[u][j], e);
        }
        for (; k < cnt; ++k) {
            const T* colp = At + (size_t)ord_idx[first + k] * ldm;
            const T v = ord_val[first + k];
#pragma unroll
            for (uint32_t j = 0; j < L; ++j) {
                const V a = row0[j] < ldm ? *reinterpret_cast<const V*>(colp + row0[j]) : V{};
#pragma unroll
                for (uint32_t e = 0; e < W; ++e) acc[j][e] = acc[j][e] + v * vget(a, e);
            }
        }
        if (STORE) {
#pragma unroll
            for (uint32_t j = 0; j < L; ++j)
#pragma unroll
                for (uint32_t e = 0; e < W; ++e)
                    if (row0[j] + e < ldm) yhat[(size_t)b * ldm + row0[j] + e] = acc[j][e];
        } else {
            double q = 0.0;
#pragma unroll
            for (uint32_t j = 0; j < L; ++j)
#pragma unroll
                for (uint32_t e = 0; e < W; ++e) {
                    const T d = yv[j][e] - acc[j][e];
                    if constexpr (WGT) q += ((double)d * (double)d) * wv[j][e];
                    else q += (double)d * (double)d;
                }
            q = wave_sum(q);
            if (lane == 0u) part[(((size_t)b * ntiles + tile) * segcap + s) * 4u + wave] = q;
        }
    }
    if (STORE && nsegs == 0u) {
#pragma unroll
        for (uint32_t j = 0; j < L; ++j)
#pragma unroll
            for (uint32_t e = 0; e < W; ++e)
                if (row0[j] + e < ldm) yhat[(size_t)b * ldm + row0[j] + e] = T(0);
    }
}

template <typename T> __device__ inline T cls_nan();
template <> __device__ inline float cls_nan<float>() { return __uint_as_float(0x7fc00000u); }
template <> __device__ inline double cls_nan<double>() { return __longlong_as_double(0x7ff8000000000000ll); }

template <typename T>
__global__ __launch_bounds__(256)
void k_cls_finish(const uint32_t* __restrict__ seg, uint32_t segcap, const uint32_t* __restrict__ sig, const double* __restrict__ part,
                  const double* __restrict__ party, uint32_t ntiles, uint32_t C, T* __restrict__ Rb, uint32_t* __restrict__ best)
{
    __shared__ T s_yn;
    __shared__ T s_v[4];
    __shared__ uint32_t s_c[4];
    const uint32_t b = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t nseg = sig[(size_t)b * kSigWords + 1u], flags = sig[(size_t)b * kSigWords + 2u];
    T* R = Rb + (size_t)b * C;
    seg += (size_t)b * segcap * 3;
    if (flags != 0u) {
        for (uint32_t c = tid; c < C; c += 256u) R[c] = cls_nan<T>();
        if (tid == 0) best[b] = 0xffffffffu;
        return;
    }
    if (tid == 0) {
        double s = 0.0;
        for (uint32_t t = 0; t < ntiles * 4u; ++t) s += party[(size_t)b * ntiles * 4u + t];
        s_yn = (T)sqrt(s);
    }
    __syncthreads();
    const T yn = s_yn;
    for (uint32_t c = tid; c < C; c += 256u) R[c] = yn;
    __threadfence_block();
    __syncthreads();
    for (uint32_t s = tid; s < nseg; s += 256u) {
        double q = 0.0;
        for (uint32_t t = 0; t < ntiles; ++t)
            for (uint32_t w = 0; w < 4u; ++w) q += part[(((size_t)b * ntiles + t) * segcap + s) * 4u + w];
        R[seg[3u * s]] = (T)sqrt(q);
    }
    __threadfence_block();
    __syncthreads();
    // left-most arg-min of the row as stored (a NaN is never smaller)
    T bv = R[0];
    uint32_t bc = 0u;
    for (uint32_t c = tid; c < C; c += 256u) {
        const T v = R[c];
        if (c != 0u && (v < bv || (v == bv && c < bc) || (bv != bv && v == v))) { bv = v; bc = c; }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const T ov = __shfl_xor(bv, o);
        const uint32_t oc = (uint32_t)__shfl_xor((int)bc, o);
        if (ov < bv || (ov == bv && oc < bc) || (bv != bv && ov == ov)) { bv = ov; bc = oc; }
    }
    if (lane == 0u) { s_v[wave] = bv; s_c[wave] = bc; }
    __syncthreads();
    if (tid == 0) {
        for (uint32_t w = 1; w < 4u; ++w) {
            const T ov = s_v[w];
            const uint32_t oc = s_c[w];
            if (ov < bv || (ov == bv && oc < bc) || (bv != bv && ov == ov)) { bv = ov; bc = oc; }
        }
        best[b] = bc;
    }
}

// dst[b * d_stride + i * d_inc] = src[b * ld + i] (a device Yhat whose rows a 2-D copy cannot describe)
template <typename T>
__global__ __launch_bounds__(256)
void k_cls_scatter(const T* __restrict__ src, uint32_t ld, uint32_t m, T* __restrict__ dst, long long d_stride, long long d_inc)
{
    const uint32_t b = blockIdx.y;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < m; i += gridDim.x * 256u)
        dst[(long long)b * d_stride + (long long)i * d_inc] = src[(size_t)b * ld + i];
}

// ---- host side -----------------------------------------------------------------------------------------------------------------

int check_classes(const ss_hip_ctx* ctx, const char* who, char* err, size_t errlen)
{
    const ClassifyState* cs = ctx->cls.as<const ClassifyState>();
    if (!cs || !cs->labels) { set_err(err, errlen, std::string(who) + ": no classes set (ss_hip_set_classes)"); return SS_HIP_EINVAL; }
    return SS_HIP_OK;
}

// a chunk's pieces: the residuals', or the reconstruction's (store: one segment, no Y, yh in place of the residuals' outputs)
template <typename T> struct ClsWork {
    size_t rb, m;
    uint32_t kmax, segcap, ntiles, C, ldm;
    bool rec_dev, y_dev, store;
    unsigned char* rec;
    T *ybuf, *ord_val, *Rb, *yh;
    uint32_t *ord_idx, *seg, *sig, *dbest, *bad;
    double *seg_l1, *dsci, *part, *party;
    void carve(Carver& cv, size_t ch)
    {
        rec = rec_dev ? nullptr : cv.take<unsigned char>(ch * rb);
        ybuf = y_dev ? nullptr : cv.take<T>(ch * m);
        ord_idx = cv.take<uint32_t>(ch * kmax);
        ord_val = cv.take<T>(ch * kmax);
        seg = cv.take<uint32_t>(ch * segcap * 3);
        seg_l1 = cv.take<double>(ch * segcap);
        sig = cv.take<uint32_t>(ch * kSigWords);
        dsci = cv.take<double>(ch);
        yh = store ? cv.take<T>(ch * ldm) : nullptr;
        dbest = store ? nullptr : cv.take<uint32_t>(ch);
        part = store ? nullptr : cv.take<double>(ch * ntiles * segcap * 4);
        party = store ? nullptr : cv.take<double>(ch * ntiles * 4);
        Rb = store ? nullptr : cv.take<T>(ch * C);
        bad = cv.take<uint32_t>(1);
    }
    // the most signals a chunk holds under the byte budget; the arena grown to them and carved
    size_t place(WorkArena& arena, size_t B)
    {
        const size_t chunk = std::min<size_t>(B, std::max<size_t>(1, std::min<size_t>(kClsChunkMax, kClsChunkBytes / carve_into(nullptr, *this, 1))));
        grow(arena, carve_into(nullptr, *this, chunk), "hipMalloc(classify workspace)");
        carve_into(arena.buf, *this, chunk);
        return chunk;
    }
};

// labels / C: the classes the residuals are taken by — the context's (class_residuals, classify), or nullptr / 1: every column in
// one class (record_residual_norms).  best may be null then.
template <typename T>
int residuals_impl(ss_hip_ctx* ctx, const char* who, const uint32_t* labels, uint32_t C, const T* Y, size_t B, ptrdiff_t y_stride,
                   ptrdiff_t incy, const void* records, uint32_t kmax, T* R, ptrdiff_t r_stride, uint32_t* best, double* sci, char* err,
                   size_t errlen, const T* Wd = nullptr, long long ws = 0)
{
    HIPCHK(hipSetDevice(ctx->device));
    ClassifyState* cs = state_of(ctx);
    hipStream_t st = ctx->stream;
    const size_t m = ctx->m, rb = record_bytes(kmax, sizeof(T));
    const uint32_t ldm = ctx->ldm, n = (uint32_t)ctx->n;
    const uint32_t ntiles = (uint32_t)((m + kClsTileRows - 1) / kClsTileRows), segcap = std::min(kmax, C);
    const bool rec_dev = on_device(records), y_dev = on_device(Y);

    ClsWork<T> w{ rb, m, kmax, segcap, ntiles, C, ldm, rec_dev, y_dev, false };
    const size_t chunk = w.place(cs->arena, B);

    std::vector<T> tmp;
    flag_arm(w.bad, st);
    for (size_t b0 = 0; b0 < B; b0 += chunk) {
        const uint32_t Bc = (uint32_t)std::min(chunk, B - b0);
        const unsigned char* recs = static_cast<const unsigned char*>(records) + b0 * rb;
        if (!rec_dev) { HIPCHK(hipMemcpyAsync(w.rec, recs, (size_t)Bc * rb, hipMemcpyHostToDevice, st)); recs = w.rec; }
        const ChunkSignals<T> y = chunk_signals<T>(ctx, Y, y_stride, incy, y_dev, w.ybuf, b0, Bc, tmp);
        hipLaunchKernelGGL((k_cls_prepare<T>), dim3(Bc), dim3(kClsThreads), (size_t)kmax * 8, st, recs, rb, kmax, n,
                           labels, C, segcap, w.ord_idx, w.ord_val, w.seg, w.seg_l1, w.sig, w.dsci, w.bad, (uint32_t)b0);
        if (Wd)                                          // (the batch's weights on the device, validated: weights_on_device)
            hipLaunchKernelGGL((k_cls_residual<T, false, true>), dim3(ntiles, Bc), dim3(kClsThreads), 0, st, static_cast<const T*>(ctx->At), ldm,
                               (uint32_t)m, y.yd, y.ys, y.yi, (const uint32_t*)w.ord_idx, (const T*)w.ord_val, kmax, (const uint32_t*)w.seg, segcap,
                               (const uint32_t*)w.sig, w.part, w.party, (T*)nullptr, Wd + (ptrdiff_t)b0 * ws, ws);
        else
            hipLaunchKernelGGL((k_cls_residual<T, false>), dim3(ntiles, Bc), dim3(kClsThreads), 0, st, static_cast<const T*>(ctx->At), ldm,
                               (uint32_t)m, y.yd, y.ys, y.yi, (const uint32_t*)w.ord_idx, (const T*)w.ord_val, kmax, (const uint32_t*)w.seg, segcap,
                               (const uint32_t*)w.sig, w.part, w.party, (T*)nullptr, (const T*)nullptr, 0ll);
        hipLaunchKernelGGL((k_cls_finish<T>), dim3(Bc), dim3(kClsThreads), 0, st, (const uint32_t*)w.seg, segcap, (const uint32_t*)w.sig,
                           (const double*)w.part, (const double*)w.party, ntiles, C, w.Rb, w.dbest);
        HIPCHK(hipGetLastError());
        if (R) HIPCHK(hipMemcpy2DAsync(R + (ptrdiff_t)b0 * r_stride, (size_t)r_stride * sizeof(T), w.Rb, (size_t)C * sizeof(T),
                                       (size_t)C * sizeof(T), Bc, hipMemcpyDefault, st));
        if (best) HIPCHK(hipMemcpyAsync(best + b0, w.dbest, (size_t)Bc * sizeof(uint32_t), hipMemcpyDefault, st));
        if (sci) HIPCHK(hipMemcpyAsync(sci + b0, w.dsci, (size_t)Bc * sizeof(double), hipMemcpyDefault, st));
    }
    return flag_verdict(w.bad, st, who, err, errlen);
}

// weighted: the call carries W / w_stride (ss_hip_weighted_class_residuals_*), checked and brought to the device behind the other checks
template <typename T>
int class_residuals_entry(ss_hip_ctx* ctx, const char* who, const T* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const void* records,
                          uint32_t kmax, T* R, ptrdiff_t r_stride, uint32_t* best, double* sci, bool weighted, const T* W, ptrdiff_t w_stride,
                          char* err, size_t errlen)
{
    const std::string w(who);
    const int rc = check_common<T>(ctx, who, records, true, kmax, err, errlen);
    if (rc != SS_HIP_OK) return rc;
    if (!Y || !best) { set_err(err, errlen, w + ": Y and best must not be null"); return SS_HIP_EINVAL; }
    if (const int rq = check_classes(ctx, who, err, errlen)) return rq;
    if (weighted)
        if (const int rw = weights_check_args(ctx, who, W, w_stride, err, errlen)) return rw;
    if (B == 0) return SS_HIP_OK;
    if (incy <= 0) { set_err(err, errlen, w + ": increments must be positive"); return SS_HIP_EINVAL; }
    if (const int rr = check_r_stride(who, R, r_stride, ctx->cls.as<const ClassifyState>()->num_classes, err, errlen)) return rr;
    return guarded(err, errlen, who, [&]() -> int {
        const ClassifyState* cs = ctx->cls.as<const ClassifyState>();
        const T* Wd = nullptr;
        long long ws = 0;
        if (weighted) {
            const int rw = weights_on_device<T>(ctx, who, W, B, w_stride, &Wd, &ws, err, errlen);
            if (rw != SS_HIP_OK) return rw;
        }
        return residuals_impl<T>(ctx, who, cs->labels, cs->num_classes, Y, B, y_stride, incy, records, kmax, R, r_stride, best, sci, err, errlen,
                                 Wd, ws);
    });
}

template <typename T>
int reconstruct_impl(ss_hip_ctx* ctx, const void* records, size_t B, uint32_t kmax, T* Yhat, ptrdiff_t yh_stride, ptrdiff_t incyh,
                     char* err, size_t errlen)
{
    HIPCHK(hipSetDevice(ctx->device));
    ClassifyState* cs = state_of(ctx);
    hipStream_t st = ctx->stream;
    const size_t m = ctx->m, rb = record_bytes(kmax, sizeof(T));
    const uint32_t ldm = ctx->ldm, n = (uint32_t)ctx->n;
    const uint32_t ntiles = (uint32_t)((m + kClsTileRows - 1) / kClsTileRows);
    const bool rec_dev = on_device(records), out_dev = on_device(Yhat);
    const bool rows2d = incyh == 1 && yh_stride >= (ptrdiff_t)m;

    ClsWork<T> w{ rb, m, kmax, 1u, ntiles, 1u, ldm, rec_dev, true, true };
    const size_t chunk = w.place(cs->arena, B);

    std::vector<T> tmp;
    flag_arm(w.bad, st);
    for (size_t b0 = 0; b0 < B; b0 += chunk) {
        const uint32_t Bc = (uint32_t)std::min(chunk, B - b0);
        const unsigned char* recs = static_cast<const unsigned char*>(records) + b0 * rb;
        if (!rec_dev) { HIPCHK(hipMemcpyAsync(w.rec, recs, (size_t)Bc * rb, hipMemcpyHostToDevice, st)); recs = w.rec; }
        hipLaunchKernelGGL((k_cls_prepare<T>), dim3(Bc), dim3(kClsThreads), (size_t)kmax * 8, st, recs, rb, kmax, n,
                           (const uint32_t*)nullptr, 1u, 1u, w.ord_idx, w.ord_val, w.seg, w.seg_l1, w.sig, w.dsci, w.bad, (uint32_t)b0);
        hipLaunchKernelGGL((k_cls_residual<T, true>), dim3(ntiles, Bc), dim3(kClsThreads), 0, st, static_cast<const T*>(ctx->At), ldm,
                           (uint32_t)m, (const T*)nullptr, 0ll, 1ll, (const uint32_t*)w.ord_idx, (const T*)w.ord_val, kmax,
                           (const uint32_t*)w.seg, 1u, (const uint32_t*)w.sig, (double*)nullptr, (double*)nullptr, w.yh, (const T*)nullptr, 0ll);
        HIPCHK(hipGetLastError());
        T* out = Yhat + (ptrdiff_t)b0 * yh_stride;
        if (rows2d) {
            HIPCHK(hipMemcpy2DAsync(out, (size_t)yh_stride * sizeof(T), w.yh, (size_t)ldm * sizeof(T), m * sizeof(T), Bc, hipMemcpyDefault, st));
        } else if (out_dev) {
            hipLaunchKernelGGL((k_cls_scatter<T>), dim3((uint32_t)std::min<size_t>((m + 255) / 256, 64), Bc), dim3(256), 0, st, (const T*)w.yh, ldm,
                               (uint32_t)m, out, (long long)yh_stride, (long long)incyh);
            HIPCHK(hipGetLastError());
        } else {
            tmp.resize((size_t)Bc * m);
            HIPCHK(hipMemcpy2DAsync(tmp.data(), m * sizeof(T), w.yh, (size_t)ldm * sizeof(T), m * sizeof(T), Bc, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            for (size_t b = 0; b < Bc; ++b)
                for (size_t i = 0; i < m; ++i) out[(ptrdiff_t)b * yh_stride + (ptrdiff_t)i * incyh] = tmp[b * m + i];
        }
    }
    return flag_verdict(w.bad, st, "reconstruct_records", err, errlen);
}

template <typename T>
int reconstruct_entry(ss_hip_ctx* ctx, const void* records, size_t B, uint32_t kmax, T* Yhat, ptrdiff_t yh_stride, ptrdiff_t incyh,
                      char* err, size_t errlen)
{
    static const char* who = "reconstruct_records";
    const int rc = check_common<T>(ctx, who, records, true, kmax, err, errlen);
    if (rc != SS_HIP_OK) return rc;
    if (!Yhat) { set_err(err, errlen, "reconstruct_records: Yhat must not be null"); return SS_HIP_EINVAL; }
    if (B == 0) return SS_HIP_OK;
    if (incyh <= 0) { set_err(err, errlen, "reconstruct_records: increments must be positive"); return SS_HIP_EINVAL; }
    return guarded(err, errlen, who, [&] { return reconstruct_impl<T>(ctx, records, B, kmax, Yhat, yh_stride, incyh, err, errlen); });
}

inline int solve_compact(ss_hip_ctx* ctx, const float* Y, size_t B, ptrdiff_t ys, ptrdiff_t iy, float tol, uint32_t mi, uint32_t kmax, void* rec,
                         char* err, size_t errlen)
{
    return ss_hip_homotopy_solve_batch_compact_f32(ctx, Y, B, ys, iy, tol, mi, kmax, rec, err, errlen);
}
inline int solve_compact(ss_hip_ctx* ctx, const double* Y, size_t B, ptrdiff_t ys, ptrdiff_t iy, double tol, uint32_t mi, uint32_t kmax, void* rec,
                         char* err, size_t errlen)
{
    return ss_hip_homotopy_solve_batch_compact_f64(ctx, Y, B, ys, iy, tol, mi, kmax, rec, err, errlen);
}

template <typename T>
int classify_entry(ss_hip_ctx* ctx, const T* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, T tol, uint32_t max_iter, uint32_t kmax,
                   void* records, T* R, ptrdiff_t r_stride, uint32_t* best, double* sci, char* err, size_t errlen)
{
    static const char* who = "classify_batch";
    const int rc = check_common<T>(ctx, who, records, false, kmax, err, errlen);
    if (rc != SS_HIP_OK) return rc;
    if (!Y || !best) { set_err(err, errlen, "classify_batch: Y and best must not be null"); return SS_HIP_EINVAL; }
    if (const int rq = check_classes(ctx, who, err, errlen)) return rq;
    if (B == 0) return SS_HIP_OK;
    if (incy <= 0) { set_err(err, errlen, "classify_batch: increments must be positive"); return SS_HIP_EINVAL; }
    if (const int rr = check_r_stride(who, R, r_stride, ctx->cls.as<const ClassifyState>()->num_classes, err, errlen)) return rr;
    return guarded(err, errlen, who, [&]() -> int {
        HIPCHK(hipSetDevice(ctx->device));
        ClassifyState* cs = state_of(ctx);
        const size_t m = ctx->m, rb = record_bytes(kmax, sizeof(T));
        // Y once to the device, the records kept there
        const bool y_dev = on_device(Y);
        std::vector<T> tmp;
        if (!y_dev) grow(cs->y_all, B * m * sizeof(T), "hipMalloc(classify signals)");
        const ChunkSignals<T> y = chunk_signals<T>(ctx, Y, y_stride, incy, y_dev, reinterpret_cast<T*>(cs->y_all.buf), 0, B, tmp);
        if (!y_dev) HIPCHK(hipStreamSynchronize(ctx->stream));
        void* rd = records;
        if (!records || !on_device(records)) {
            grow(cs->rec_all, B * rb, "hipMalloc(classify records)");
            rd = cs->rec_all.buf;
        }
        const int rs = solve_compact(ctx, y.yd, B, (ptrdiff_t)y.ys, (ptrdiff_t)y.yi, tol, max_iter, kmax, rd, err, errlen);
        if (rs != SS_HIP_OK) return rs;
        const int rr = residuals_impl<T>(ctx, "class_residuals", cs->labels, cs->num_classes, y.yd, B, (ptrdiff_t)y.ys, (ptrdiff_t)y.yi, rd, kmax, R, r_stride, best, sci, err, errlen);
        if (rr != SS_HIP_OK) return rr;
        if (records && rd != records) HIPCHK(hipMemcpy(records, rd, B * rb, hipMemcpyDeviceToHost));
        return SS_HIP_OK;
    });
}

}  // namespace

// Rn[b] = ||y_b - A x_b||_2 of B compact records: the words ss_hip_class_residuals_* gives in R[b][0] with every column in class 0
// (its kernels, its order; NaN for a truncated record, ||y_b||_2 for K = 0).  The residual path behind the entry point's validation,
// for the refit (refit.hip); needs no classes.  Y, records and Rn on either side.  Throws what HIPCHK throws: call it under guarded.
template <typename T>
int record_residual_norms(ss_hip_ctx* ctx, const char* who, const T* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const void* records,
                          uint32_t kmax, T* Rn, char* err, size_t errlen)
{
    return residuals_impl<T>(ctx, who, nullptr, 1u, Y, B, y_stride, incy, records, kmax, Rn, 1, nullptr, nullptr, err, errlen);
}

template int record_residual_norms<float>(ss_hip_ctx*, const char*, const float*, size_t, ptrdiff_t, ptrdiff_t, const void*, uint32_t, float*, char*, size_t);
template int record_residual_norms<double>(ss_hip_ctx*, const char*, const double*, size_t, ptrdiff_t, ptrdiff_t, const void*, uint32_t, double*, char*, size_t);

// the rows of ss_hip_class_residuals_* under the context's classes, behind the entry point's validation: for the group class residuals
// (joint.hip).  Call it under guarded, with classes set (classify_num_classes != 0)
template <typename T>
int class_residual_rows(ss_hip_ctx* ctx, const char* who, const T* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const void* records,
                        uint32_t kmax, T* R, ptrdiff_t r_stride, uint32_t* best, char* err, size_t errlen)
{
    const ClassifyState* cs = ctx->cls.as<const ClassifyState>();
    return residuals_impl<T>(ctx, who, cs->labels, cs->num_classes, Y, B, y_stride, incy, records, kmax, R, r_stride, best, nullptr, err, errlen);
}

template int class_residual_rows<float>(ss_hip_ctx*, const char*, const float*, size_t, ptrdiff_t, ptrdiff_t, const void*, uint32_t, float*, ptrdiff_t,
                                        uint32_t*, char*, size_t);
template int class_residual_rows<double>(ss_hip_ctx*, const char*, const double*, size_t, ptrdiff_t, ptrdiff_t, const void*, uint32_t, double*,
                                         ptrdiff_t, uint32_t*, char*, size_t);

// the weighted forms (weighted.hip).  weighted_residual_rows: the residual path under weights already on the device and validated —
// by_class: under the context's classes (set), else every column in class 0 (the weighted refit's residual norms).
// class_residuals_weighted: ss_hip_weighted_class_residuals_* whole, the unweighted entry's checks in its order
template <typename T>
int weighted_residual_rows(ss_hip_ctx* ctx, const char* who, bool by_class, const T* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy,
                           const void* records, uint32_t kmax, T* R, ptrdiff_t r_stride, uint32_t* best, double* sci, const T* Wd, long long ws,
                           char* err, size_t errlen)
{
    const ClassifyState* cs = ctx->cls.as<const ClassifyState>();
    return residuals_impl<T>(ctx, who, by_class ? cs->labels : nullptr, by_class ? cs->num_classes : 1u, Y, B, y_stride, incy, records, kmax, R,
                             r_stride, best, sci, err, errlen, Wd, ws);
}
template int weighted_residual_rows<float>(ss_hip_ctx*, const char*, bool, const float*, size_t, ptrdiff_t, ptrdiff_t, const void*, uint32_t, float*,
                                           ptrdiff_t, uint32_t*, double*, const float*, long long, char*, size_t);
template int weighted_residual_rows<double>(ss_hip_ctx*, const char*, bool, const double*, size_t, ptrdiff_t, ptrdiff_t, const void*, uint32_t,
                                            double*, ptrdiff_t, uint32_t*, double*, const double*, long long, char*, size_t);

template <typename T>
int class_residuals_weighted(ss_hip_ctx* ctx, const T* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const T* W, ptrdiff_t w_stride,
                             const void* records, uint32_t kmax, T* R, ptrdiff_t r_stride, uint32_t* best, double* sci, char* err, size_t errlen)
{
    return class_residuals_entry<T>(ctx, "weighted_class_residuals", Y, B, y_stride, incy, records, kmax, R, r_stride, best, sci, true, W, w_stride,
                                    err, errlen);
}
template int class_residuals_weighted<float>(ss_hip_ctx*, const float*, size_t, ptrdiff_t, ptrdiff_t, const float*, ptrdiff_t, const void*, uint32_t,
                                             float*, ptrdiff_t, uint32_t*, double*, char*, size_t);
template int class_residuals_weighted<double>(ss_hip_ctx*, const double*, size_t, ptrdiff_t, ptrdiff_t, const double*, ptrdiff_t, const void*,
                                              uint32_t, double*, ptrdiff_t, uint32_t*, double*, char*, size_t);

uint32_t classify_num_classes(const ss_hip_ctx* ctx)
{
    const ClassifyState* cs = ctx->cls.as<const ClassifyState>();
    return cs && cs->labels ? cs->num_classes : 0u;
}

const uint32_t* classify_labels(const ss_hip_ctx* ctx)
{
    const ClassifyState* cs = ctx->cls.as<const ClassifyState>();
    return cs ? cs->labels : nullptr;
}

uint64_t classify_generation(const ss_hip_ctx* ctx)
{
    const ClassifyState* cs = ctx->cls.as<const ClassifyState>();
    return cs ? cs->generation : 0;
}

}  // namespace sship

using namespace sship;

extern "C" {

int ss_hip_set_classes(ss_hip_ctx* ctx, const uint32_t* labels, uint32_t num_classes, char* err, size_t errlen)
{
    if (!ctx) { set_err(err, errlen, "set_classes: null context"); return SS_HIP_EINVAL; }
    if (ctx->kind != 0) { set_err(err, errlen, "set_classes: this context was created for IRLS"); return SS_HIP_EINVAL; }
    if (ctx->colshard != nullptr) { set_err(err, errlen, "set_classes: not available on a column-sharded context"); return SS_HIP_EINVAL; }
    if (!labels || num_classes == 0) { set_err(err, errlen, "set_classes: labels must not be null and num_classes >= 1"); return SS_HIP_EINVAL; }
    return guarded(err, errlen, "set_classes", [&]() -> int {
        HIPCHK(hipSetDevice(ctx->device));
        ClassifyState* cs = state_of(ctx);
        const uint32_t n = (uint32_t)ctx->n, np = ctx->n_pad;
        uint32_t* fresh = nullptr;
        HELD(cs->own, hipMalloc, reinterpret_cast<void**>(&fresh), ((size_t)np + 1) * sizeof(uint32_t));
        uint32_t bad = 0xffffffffu;
        hipError_t e = hipMemsetAsync(fresh, 0, (size_t)np * sizeof(uint32_t), ctx->stream);
        if (e == hipSuccess) e = hipMemsetAsync(fresh + np, 0xff, sizeof(uint32_t), ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(fresh, labels, (size_t)n * sizeof(uint32_t), hipMemcpyDefault, ctx->stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_cls_check_labels, dim3((n + 255u) / 256u), dim3(256), 0, ctx->stream, (const uint32_t*)fresh, n, num_classes, fresh + np);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(&bad, fresh + np, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) { (void)cs->own.drop(fresh); throw HipFail{ e, "set_classes: upload of the labels" }; }
        if (bad != 0xffffffffu) {
            (void)cs->own.drop(fresh);
            set_err(err, errlen, "set_classes: the label of column " + std::to_string(bad) + " is not below num_classes");
            return SS_HIP_EINVAL;
        }
        HIPCHK(cs->own.drop(cs->labels));
        cs->labels = fresh;
        cs->num_classes = num_classes;
        cs->generation += 1;
        return SS_HIP_OK;
    });
}

int ss_hip_reconstruct_records_f32(ss_hip_ctx* ctx, const void* records, size_t B, uint32_t kmax, float* Yhat, ptrdiff_t yh_stride,
                                   ptrdiff_t incyh, char* err, size_t errlen)
{
    return reconstruct_entry<float>(ctx, records, B, kmax, Yhat, yh_stride, incyh, err, errlen);
}
int ss_hip_reconstruct_records_f64(ss_hip_ctx* ctx, const void* records, size_t B, uint32_t kmax, double* Yhat, ptrdiff_t yh_stride,
                                   ptrdiff_t incyh, char* err, size_t errlen)
{
    return reconstruct_entry<double>(ctx, records, B, kmax, Yhat, yh_stride, incyh, err, errlen);
}

int ss_hip_class_residuals_f32(ss_hip_ctx* ctx, const float* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const void* records,
                               uint32_t kmax, float* R, ptrdiff_t r_stride, uint32_t* best, double* sci, char* err, size_t errlen)
{
    return class_residuals_entry<float>(ctx, "class_residuals", Y, B, y_stride, incy, records, kmax, R, r_stride, best, sci, false, nullptr, 0, err, errlen);
}
int ss_hip_class_residuals_f64(ss_hip_ctx* ctx, const double* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const void* records,
                               uint32_t kmax, double* R, ptrdiff_t r_stride, uint32_t* best, double* sci, char* err, size_t errlen)
{
    return class_residuals_entry<double>(ctx, "class_residuals", Y, B, y_stride, incy, records, kmax, R, r_stride, best, sci, false, nullptr, 0, err, errlen);
}

int ss_hip_homotopy_classify_batch_f32(ss_hip_ctx* ctx, const float* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, float tol,
                                       uint32_t max_iter, uint32_t kmax, void* records, float* R, ptrdiff_t r_stride, uint32_t* best,
                                       double* sci, char* err, size_t errlen)
{
    return classify_entry<float>(ctx, Y, B, y_stride, incy, tol, max_iter, kmax, records, R, r_stride, best, sci, err, errlen);
}
int ss_hip_homotopy_classify_batch_f64(ss_hip_ctx* ctx, const double* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, double tol,
                                       uint32_t max_iter, uint32_t kmax, void* records, double* R, ptrdiff_t r_stride, uint32_t* best,
                                       double* sci, char* err, size_t errlen)
{
    return classify_entry<double>(ctx, Y, B, y_stride, incy, tol, max_iter, kmax, records, R, r_stride, best, sci, err, errlen);
}

}  // extern "C"
