// topcorr.hip — the top correlations of residuals on the matrix cores and the record extension (include/ss_hip.h):
//   ss_hip_top_correlations_*, ss_hip_extend_records_*.
//
// For signal b the first call returns the k atoms that best explain what its record leaves over: the columns i, not stored in the
// record, with the largest s(i, b) = |a_i . r_b| / ||a_i||, r_b = y_b - A x_b.  The second call enters named columns into compact
// records.  Together with the refit (refit.hip) they are one stage of stagewise OMP; one stage alone is the thresholding coder.
// G = A^T A is never read: the product A^T R of a chunk of signals runs on the MFMA units from A.  Kernels:
//
//   k_tc_signals  grid = (row tile, signal): the residual block of a call WITHOUT records — the words of y_b, zero padded to ldm.
//                 With records the block is dictlearn.hip's (dl_launch_residuals: the atom update's and the K-SVD sweep's words).
//   k_tc_check    one workgroup per signal, the whole batch before anything is written: the first record with a column index >= n
//                 (never used as an address).
//   k_tc_tile     grid = (signal tile, column tile), 128 x 128 x 128 bytes of K per step, 256 threads, two workgroups a CU.  The
//                 queries are the rows of the residual block [Bc][ldm], the other operand is At.  Tiling, staging, MFMA instructions
//                 and chain order are coherence.hip's k_coh_tile (its main loop is stated here a second time: the two epilogues share
//                 nothing, and coherence.hip stays the unit its tests pin).  Epilogue: dot in T to the block D [Bc][n_pad].
//   k_tc_select   (tc_select.h) one workgroup per signal.  The record's columns are struck out of the signal's row of D by index (a
//                 NaN word: a NaN score is never selected); the scores are formed in double from the stored dots and rn by this unit's
//                 scorer, TcAbsScorer; the k best by the total order (score descending, index ascending) are found by a radix
//                 selection on the score's bits — eight bits a pass, LDS histogram of integer counts — until the columns that can
//                 still be among the k best fit an LDS list of 1024, which is sorted by the total order (bitonic).  All columns tied
//                 on the k-th score (a zero residual): the smallest indices are taken in ascending blocks.  nonneg.hip and
//                 weighted.hip run the same kernel with their scorers; joint.hip's k_js_select calls the selection behind the key
//                 (tc_select_sorted) with a group's stored score.
//   k_tc_extend_check / k_tc_extend   the record extension: one workgroup per signal, the record in LDS, the entries of the row one
//                 after the other (membership and insertion point across the threads, the move block by block from the top).
//
// ORDER (stated once; build flag -ffp-contract=off: outside the MFMA products and sums are rounded separately):
//   r_b          k_dl_residual's words (dictlearn.hip: the record's columns added in record order, one subtraction in T); rows
//                m .. ldm - 1 are zero.
//   dot(i, b)    one accumulator, started at 0, in the context's precision; the K-steps ascending over the padded rows.  fp32: a
//                K-step holds 32 rows; MFMA (g, t), g = 0 .. 3 outer, t = 0 .. 3 inner, adds the rows 8 g + t and 8 g + 4 + t of the
//                step, in the instruction's order.  fp64: a K-step holds 16 rows; MFMA g = 0 .. 3 adds the rows 4 g .. 4 g + 3.  The
//                chain does not depend on where in a tile the pair sits: dot(i, b) is a function of column i, r_b and m alone.
//   d_i, rn_i    k_coh_norms' words (coherence.hip), per call: rn_i = 1 / sqrt(d_i) in double, 0 for an excluded column.
//   s(i, b)      = |dot(i, b)| * rn_i, dot widened to double: one multiplication.
//   coef         = (T)((double)dot * (rn_i * rn_i)): the square first, one rounding to T at the end.
//   selection    a maximum under a total order: whichever way the comparisons run, the result is the same.  The integer atomics (the
//                histogram's counts, the slots of the unsorted list) cannot change it: counts commute, and the list is sorted by a
//                total order afterwards.  No floating-point atomics.
// Nothing depends on B, on the chunking, on the launch geometry, on where the pointers live or on what the context did before.
// The host side of ss_hip_top_correlations_* is the driver tc_driver.h states once for the four selection calls; this unit owns
// the arena they and the record extension carve (topcorr_arena) and the launches behind the driver (ss_hip_internal.h):
// tc_launch_record_check / tc_launch_residual_block / tc_launch_dots, a chunk's record check, residual block and dot block, and
// tc_launch_weight_dots, k_tc_tile with the squaring flag, weighted.hip's second product.
#include "ss_hip_internal.h"
#include "tc_driver.h"

#include <algorithm>
#include <cmath>

namespace sship {

namespace {

constexpr uint32_t kTcVecs = 8;                          // 16-byte vectors of K per row and step (32 floats / 16 doubles)
constexpr uint32_t kTcPitch = kTcVecs + 1;               // LDS row pitch in vectors (144 B, as in coherence.hip)
// (kTcTile, kTcNone, kTcList, kTcChunkMax, kTcChunkBytes: tc_select.h, shared with joint.hip)

typedef float tc_v4f __attribute__((ext_vector_type(4)));
typedef float tc_v16f __attribute__((ext_vector_type(16)));
typedef double tc_v2d __attribute__((ext_vector_type(2)));
typedef double tc_v4d __attribute__((ext_vector_type(4)));

// the wave's 64 x 64 share of a tile as NI x NI accumulators of WT x WT (coherence.hip: CohMma)
template <typename T> struct TcMma;
template <> struct TcMma<float> {
    typedef tc_v4f Vec;
    typedef tc_v16f Acc;
    static constexpr uint32_t NI = 2, NE = 16, WT = 32, KS = 32;
    // C/D layout of the 32 x 32 MFMA: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    __device__ static uint32_t row(uint32_t e, uint32_t hq) { return (e & 3u) + 8u * (e >> 2) + 4u * hq; }
};
template <> struct TcMma<double> {
    typedef tc_v2d Vec;
    typedef tc_v4d Acc;
    static constexpr uint32_t NI = 4, NE = 4, WT = 16, KS = 16;
    // C/D layout of the fp64 16 x 16 MFMA: col = lane & 15, row = (lane >> 4) + 4 reg
    __device__ static uint32_t row(uint32_t e, uint32_t hq) { return 4u * e + hq; }
};

// ---- kernels -------------------------------------------------------------------------------------------------------------------

// R[b][0 .. ldm) = the words of y_b, rows m .. ldm - 1 zero
template <typename T>
__global__ __launch_bounds__(256)
void k_tc_signals(const T* __restrict__ Y, long long y_stride, long long incy, uint32_t m, uint32_t ldm, T* __restrict__ R)
{
    const uint32_t row = blockIdx.x * 256u + threadIdx.x, b = blockIdx.y;
    if (row >= ldm) return;
    R[(size_t)b * ldm + row] = row < m ? Y[(long long)b * y_stride + (long long)row * incy] : T(0);
}

__global__ __launch_bounds__(64)
void k_tc_check(const unsigned char* __restrict__ rec, size_t rb, uint32_t kmax, uint32_t n, uint32_t* __restrict__ bad)
{
    const uint32_t b = blockIdx.x;
    const unsigned char* r = rec + (size_t)b * rb;
    rec_check_indices(r, *reinterpret_cast<const uint32_t*>(r), kmax, n, b, bad);
}

// R: [signal tiles x 128][ldm]; D: [signal tiles x 128][n_pad].  SQ: every element of At is squared once in T where it is staged
// (one multiplication between the global load and the LDS store): with a block of weights for R the tile is d(i, b) = sum_k
// w_kb a_ki^2 of the weighted top correlations (weighted.hip) — the same tile, the same chain.  Without SQ nothing is added.
template <typename T, bool SQ = false>
__global__ __launch_bounds__(256, 2)
void k_tc_tile(const T* __restrict__ At, uint32_t ldm, const T* __restrict__ R, uint32_t n_pad, T* __restrict__ D)
{
    typedef TcMma<T> M;
    typedef typename M::Vec Vec;
    typedef typename M::Acc Acc;
    constexpr uint32_t NI = M::NI, NE = M::NE, WT = M::WT;
    __shared__ __attribute__((aligned(16))) Vec sA[2][kTcTile][kTcPitch];      // the residuals
    __shared__ __attribute__((aligned(16))) Vec sB[2][kTcTile][kTcPitch];      // the columns

    // signal tiles fastest: concurrently resident workgroups share the same panel of At
    const uint32_t bt = blockIdx.x, bn = blockIdx.y;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t wm = wave & 1u, wn = wave >> 1;
    const uint32_t lc = lane & (WT - 1u), hq = lane / WT;

    // staging map: thread -> (rows srow + 32 j, vector svec of the step)
    const uint32_t srow = tid >> 3, svec = tid & 7u;
    const Vec* gA[4];
    const Vec* gB[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        gA[j] = reinterpret_cast<const Vec*>(R + (size_t)(bt * kTcTile + srow + 32u * (uint32_t)j) * ldm) + svec;
        gB[j] = reinterpret_cast<const Vec*>(At + (size_t)(bn * kTcTile + srow + 32u * (uint32_t)j) * ldm) + svec;
    }

    Acc acc[NI][NI];
#pragma unroll
    for (uint32_t i = 0; i < NI; ++i)
#pragma unroll
        for (uint32_t j = 0; j < NI; ++j)
#pragma unroll
            for (uint32_t e = 0; e < NE; ++e) acc[i][j][e] = T(0);

    Vec stA[4], stB[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { stA[j] = gA[j][0]; stB[j] = gB[j][0]; if constexpr (SQ) stB[j] = stB[j] * stB[j]; }
#pragma unroll
    for (int j = 0; j < 4; ++j) { sA[0][srow + 32 * j][svec] = stA[j]; sB[0][srow + 32 * j][svec] = stB[j]; }
    __syncthreads();

    const uint32_t nk = ldm / M::KS;
    uint32_t cur = 0;
    for (uint32_t kt = 0; kt < nk; ++kt) {
        const bool more = (kt + 1u) < nk;
        if (more) {
            const uint32_t voff = (kt + 1u) * kTcVecs;
#pragma unroll
            for (int j = 0; j < 4; ++j) { stA[j] = gA[j][voff]; stB[j] = gB[j][voff]; if constexpr (SQ) stB[j] = stB[j] * stB[j]; }
        }
        if constexpr (sizeof(T) == 4) {
#pragma unroll
            for (uint32_t g = 0; g < 4; ++g) {
                Vec a[NI], b[NI];
#pragma unroll
                for (uint32_t i = 0; i < NI; ++i) {
                    a[i] = sA[cur][wm * 64u + i * WT + lc][2u * g + hq];
                    b[i] = sB[cur][wn * 64u + i * WT + lc][2u * g + hq];
                }
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (uint32_t i = 0; i < NI; ++i)
#pragma unroll
                        for (uint32_t j = 0; j < NI; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][t], b[j][t], acc[i][j], 0, 0, 0);
            }
        } else {
#pragma unroll
            for (uint32_t g = 0; g < 4; ++g) {
                const uint32_t k = 4u * g + hq;
                double a[NI], b[NI];
#pragma unroll
                for (uint32_t i = 0; i < NI; ++i) {
                    a[i] = reinterpret_cast<const double*>(&sA[cur][wm * 64u + i * WT + lc][0])[k];
                    b[i] = reinterpret_cast<const double*>(&sB[cur][wn * 64u + i * WT + lc][0])[k];
                }
#pragma unroll
                for (uint32_t i = 0; i < NI; ++i)
#pragma unroll
                    for (uint32_t j = 0; j < NI; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
            }
        }
        if (more) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { sA[cur ^ 1u][srow + 32 * j][svec] = stA[j]; sB[cur ^ 1u][srow + 32 * j][svec] = stB[j]; }
        }
        __syncthreads();
        cur ^= 1u;
    }

    // ---- epilogue: the dots as they are; a lane holds column lc of each accumulator, WT lanes write one run of a row ----
    T* d0 = D + (size_t)(bt * kTcTile + wm * 64u) * n_pad + bn * kTcTile + wn * 64u + lc;
#pragma unroll
    for (uint32_t i = 0; i < NI; ++i)
#pragma unroll
        for (uint32_t e = 0; e < NE; ++e) {
            T* dr = d0 + (size_t)(i * WT + M::row(e, hq)) * n_pad;
#pragma unroll
            for (uint32_t j = 0; j < NI; ++j) dr[j * WT] = acc[i][j][e];
        }
}

// top_correlations' scorer for k_tc_select (tc_select.h): every column with a norm is a candidate, s = |dot| * rn_i
template <typename T> struct TcAbsScorer {
    const double* __restrict__ rinv;
    __device__ const TcAbsScorer& row(uint32_t, uint32_t) const { return *this; }
    __device__ bool key(const T* d, uint32_t i, unsigned long long& key) const
    {
        const double r = rinv[i];
        if (r == 0.0) return false;
        const double s = fabs((double)d[i]) * r;
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

// bad[0]: the first record with a column index >= n; bad[1]: the first row of idx with an entry >= n that is not NONE
__global__ __launch_bounds__(64)
void k_tc_extend_check(const unsigned char* __restrict__ rec, size_t rb, uint32_t kmax, uint32_t n, const uint32_t* __restrict__ idx,
                       uint32_t k, uint32_t* __restrict__ bad)
{
    const uint32_t b = blockIdx.x;
    const unsigned char* r = rec + (size_t)b * rb;
    rec_check_indices(r, *reinterpret_cast<const uint32_t*>(r), kmax, n, b, &bad[0]);
    for (uint32_t t = threadIdx.x; t < k; t += 64u) {
        const uint32_t cidx = idx[(size_t)b * k + t];
        if (cidx != kTcNone && cidx >= n) atomicMin(&bad[1], b);
    }
}

// VW: 32-bit words of a value.  rec_in and rec_out: the same records (in place) or disjoint ones.  coef: words, or null
template <uint32_t VW>
__global__ __launch_bounds__(256)
void k_tc_extend(const unsigned char* rec_in, unsigned char* rec_out, size_t rb, uint32_t kmax, const uint32_t* __restrict__ idx,
                 const uint32_t* __restrict__ coef, uint32_t k, uint32_t* __restrict__ added)
{
    extern __shared__ __align__(16) unsigned char s_tc_raw[];
    uint32_t* sidx = reinterpret_cast<uint32_t*>(s_tc_raw);      // [kmax]
    uint32_t* sval = sidx + kmax;                                // [kmax][VW]
    __shared__ uint32_t s_found, s_pos;
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    const uint32_t* wi = reinterpret_cast<const uint32_t*>(rec_in + (size_t)b * rb);
    uint32_t* wo = reinterpret_cast<uint32_t*>(rec_out + (size_t)b * rb);
    const uint32_t words = (uint32_t)(rb / 4), Krec = wi[0];
    if (Krec > kmax) {                                           // a truncated record: unchanged
        if (wi != wo)
            for (uint32_t w = tid; w < words; w += 256u) wo[w] = wi[w];
        if (tid == 0) added[b] = 0u;
        return;
    }
    for (uint32_t e = tid; e < kmax; e += 256u) sidx[e] = wi[4u + e];
    for (uint32_t w = tid; w < kmax * VW; w += 256u) sval[w] = wi[4u + kmax + w];
    uint32_t K = Krec;
    for (uint32_t t = 0; t < k && K < kmax; ++t) {               // (every condition below is uniform across the workgroup)
        const uint32_t cidx = idx[(size_t)b * k + t];
        if (cidx == kTcNone) continue;
        __syncthreads();
        if (tid == 0) { s_found = 0u; s_pos = K; }
        __syncthreads();
        for (uint32_t e = tid; e < K; e += 256u) {
            const uint32_t v = sidx[e];
            if (v == cidx) atomicOr(&s_found, 1u);
            if (v > cidx) atomicMin(&s_pos, e);
        }
        __syncthreads();
        const uint32_t found = s_found, pos = s_pos;
        if (found) continue;
        // the entries pos .. K - 1 move up by one: blocks of 256 from the top, each read whole before it is written
        for (uint32_t hi = K; hi > pos;) {
            const uint32_t lo = hi - pos > 256u ? hi - 256u : pos, e = lo + tid;
            uint32_t vi = 0, vv[VW];
            if (e < hi) {
                vi = sidx[e];
#pragma unroll
                for (uint32_t w = 0; w < VW; ++w) vv[w] = sval[e * VW + w];
            }
            __syncthreads();
            if (e < hi) {
                sidx[e + 1u] = vi;
#pragma unroll
                for (uint32_t w = 0; w < VW; ++w) sval[(e + 1u) * VW + w] = vv[w];
            }
            __syncthreads();
            hi = lo;
        }
        if (tid == 0) {
            sidx[pos] = cidx;
#pragma unroll
            for (uint32_t w = 0; w < VW; ++w) sval[pos * VW + w] = coef ? coef[((size_t)b * k + t) * VW + w] : 0u;
        }
        K += 1u;
    }
    __syncthreads();
    // K, then iter and err word for word, the lists from LDS, the padding behind them
    for (uint32_t w = tid; w < words; w += 256u) {
        const uint32_t v = w == 0u ? K : w < 4u ? wi[w] : w < 4u + kmax ? sidx[w - 4u] : w < 4u + kmax + kmax * VW ? sval[w - 4u - kmax] : wi[w];
        wo[w] = v;
    }
    if (tid == 0) added[b] = K - Krec;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------

// the extension's pieces: the records' staging, a host caller's idx and coef, `added`, the two bad-index words
template <typename T> struct ExtendWork {
    bool idx_dev, coef_dev;
    unsigned char* stage = nullptr;
    uint32_t *di = nullptr, *dadd = nullptr, *bad = nullptr;
    T* dc = nullptr;
    void carve(Carver& cv, const RecordPlace& place, size_t B, uint32_t k)
    {
        stage = place.carve(cv);
        di = idx_dev ? nullptr : cv.take<uint32_t>(B * k);
        dc = coef_dev ? nullptr : cv.take<T>(B * k);
        dadd = cv.take<uint32_t>(B);
        bad = cv.take<uint32_t>(2);
    }
};

template <typename T>
int extend_impl(ss_hip_ctx* ctx, const void* records, size_t B, uint32_t kmax, const uint32_t* idx, const T* coef, uint32_t k, void* records_out,
                uint32_t* added, char* err, size_t errlen)
{
    static const char* who = "extend_records";
    constexpr uint32_t VW = sizeof(T) / 4;
    HIPCHK(hipSetDevice(ctx->device));
    WorkArena& ts = topcorr_arena(ctx);
    hipStream_t st = ctx->stream;
    const size_t rb = record_bytes(kmax, sizeof(T));
    const uint32_t n = (uint32_t)ctx->n, Bu = (uint32_t)B;
    RecordPlace place(records, records_out, B * rb);
    ExtendWork<T> w{ on_device(idx), !coef || on_device(coef) };
    if (!arena_grow(ts, carve_into(nullptr, w, place, B, k), who, err, errlen)) return SS_HIP_ENOMEM;
    carve_into(ts.buf, w, place, B, k);

    place.stage_in(w.stage, st);
    const uint32_t* didx = idx;
    if (!w.idx_dev) { HIPCHK(hipMemcpyAsync(w.di, idx, B * k * sizeof(uint32_t), hipMemcpyHostToDevice, st)); didx = w.di; }
    const T* dcoef = coef;
    if (!w.coef_dev) { HIPCHK(hipMemcpyAsync(w.dc, coef, B * k * sizeof(T), hipMemcpyHostToDevice, st)); dcoef = w.dc; }
    flag_arm(w.bad, st, 2);
    hipLaunchKernelGGL(k_tc_extend_check, dim3(Bu), dim3(64), 0, st, place.din, rb, kmax, n, didx, k, w.bad);
    HIPCHK(hipGetLastError());
    uint32_t first_bad[2];
    flag_fetch(first_bad, w.bad, st, 2);                     // (nothing has been written when a record or a row is invalid)
    if (first_bad[0] != kNoRecord) return bad_index(first_bad[0], who, err, errlen);
    if (first_bad[1] != kNoRecord) {
        set_err(err, errlen, std::string(who) + ": row " + std::to_string(first_bad[1]) + " of idx holds a column index >= n");
        return SS_HIP_EINVAL;
    }
    hipLaunchKernelGGL((k_tc_extend<VW>), dim3(Bu), dim3(256), (size_t)kmax * (1u + VW) * sizeof(uint32_t), st, place.din, place.dout, rb, kmax, didx,
                       reinterpret_cast<const uint32_t*>(dcoef), k, w.dadd);
    HIPCHK(hipGetLastError());
    if (added) HIPCHK(hipMemcpyAsync(added, w.dadd, B * sizeof(uint32_t), hipMemcpyDefault, st));
    place.copy_out(w.stage, st);
    HIPCHK(hipStreamSynchronize(st));
    return SS_HIP_OK;
}

template <typename T>
int extend_entry(ss_hip_ctx* ctx, const void* records, size_t B, uint32_t kmax, const uint32_t* idx, const T* coef, uint32_t k, void* records_out,
                 uint32_t* added, char* err, size_t errlen)
{
    static const char* who = "extend_records";
    int rc = check_common<T>(ctx, who, records, true, kmax, err, errlen);
    if (rc != SS_HIP_OK) return rc;
    if (!idx || !records_out) { set_err(err, errlen, "extend_records: idx and records_out must not be null"); return SS_HIP_EINVAL; }
    if ((rc = check_out_aligned(who, records_out, err, errlen)) != SS_HIP_OK) return rc;
    if ((rc = tc_check_k(who, k, err, errlen)) != SS_HIP_OK) return rc;
    if ((rc = check_batch(who, B, err, errlen)) != SS_HIP_OK) return rc;
    if ((rc = check_overlap(who, records, records_out, B * record_bytes(kmax, sizeof(T)), err, errlen)) != SS_HIP_OK) return rc;
    if (B == 0) return SS_HIP_OK;                             // (every argument above was checked all the same)
    return guarded(err, errlen, who, [&] { return extend_impl<T>(ctx, records, B, kmax, idx, coef, k, records_out, added, err, errlen); });
}

}  // namespace

// ---- the launches behind the driver (ss_hip_internal.h), on the context's stream, every pointer on the device -----------------------

hipError_t tc_launch_record_check(ss_hip_ctx* ctx, const unsigned char* recs, size_t rb, uint32_t kmax, uint32_t B, uint32_t* bad)
{
    hipError_t e = hipMemsetAsync(bad, 0xff, sizeof(uint32_t), ctx->stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_tc_check, dim3(B), dim3(64), 0, ctx->stream, recs, rb, kmax, (uint32_t)ctx->n, bad);
    return hipGetLastError();
}

template <typename T>
hipError_t tc_launch_residual_block(ss_hip_ctx* ctx, const T* yd, long long ys, long long yi, const unsigned char* recs, size_t rb, uint32_t kmax,
                                    uint32_t Bc, T* R, double* part)
{
    const uint32_t ldm = ctx->ldm, btiles = (Bc + kTcTile - 1u) / kTcTile;
    // the rows behind the chunk's last signal, up to a whole tile: zero (their dots are never read).  The row of a truncated record
    // is not written by the residual kernel either and holds what the workspace held: a tile's rows are independent of each
    // other, and the selection leaves such a signal (or its group) before it reads a dot
    if (btiles * kTcTile != Bc) {
        const hipError_t e = hipMemsetAsync(R + (size_t)Bc * ldm, 0, (size_t)(btiles * kTcTile - Bc) * ldm * sizeof(T), ctx->stream);
        if (e != hipSuccess) return e;
    }
    if (recs) return dl_launch_residuals<T>(ctx, yd, ys, yi, recs, rb, kmax, Bc, R, part);
    hipLaunchKernelGGL((k_tc_signals<T>), dim3((ldm + 255u) / 256u, Bc), dim3(256), 0, ctx->stream, yd, ys, yi, (uint32_t)ctx->m, ldm, R);
    return hipGetLastError();
}

template <typename T>
hipError_t tc_launch_dots(ss_hip_ctx* ctx, const T* R, uint32_t Bc, T* D)
{
    const uint32_t btiles = (Bc + kTcTile - 1u) / kTcTile, ctiles = ((uint32_t)ctx->n + kTcTile - 1u) / kTcTile;
    hipLaunchKernelGGL((k_tc_tile<T>), dim3(btiles, ctiles), dim3(256), 0, ctx->stream, static_cast<const T*>(ctx->At), ctx->ldm, R, ctx->n_pad, D);
    return hipGetLastError();
}

template <typename T>
hipError_t tc_launch_weight_dots(ss_hip_ctx* ctx, const T* Wb, uint32_t Bc, T* D2)
{
    const uint32_t btiles = (Bc + kTcTile - 1u) / kTcTile, ctiles = ((uint32_t)ctx->n + kTcTile - 1u) / kTcTile;
    hipLaunchKernelGGL((k_tc_tile<T, true>), dim3(btiles, ctiles), dim3(256), 0, ctx->stream, static_cast<const T*>(ctx->At), ctx->ldm, Wb, ctx->n_pad,
                       D2);
    return hipGetLastError();
}

template hipError_t tc_launch_residual_block<float>(ss_hip_ctx*, const float*, long long, long long, const unsigned char*, size_t, uint32_t, uint32_t,
                                                    float*, double*);
template hipError_t tc_launch_residual_block<double>(ss_hip_ctx*, const double*, long long, long long, const unsigned char*, size_t, uint32_t,
                                                     uint32_t, double*, double*);
template hipError_t tc_launch_dots<float>(ss_hip_ctx*, const float*, uint32_t, float*);
template hipError_t tc_launch_dots<double>(ss_hip_ctx*, const double*, uint32_t, double*);
template hipError_t tc_launch_weight_dots<float>(ss_hip_ctx*, const float*, uint32_t, float*);
template hipError_t tc_launch_weight_dots<double>(ss_hip_ctx*, const double*, uint32_t, double*);

WorkArena& topcorr_arena(ss_hip_ctx* ctx)
{
    return part<WorkArena>(ctx->tc);
}

}  // namespace sship

using namespace sship;

extern "C" {

int ss_hip_top_correlations_f32(ss_hip_ctx* ctx, const float* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const void* records,
                                uint32_t kmax, uint32_t k, uint32_t* idx, float* coef, double* score, char* err, size_t errlen)
{
    return tc_dots_entry<float, TcAbsScorer<float>>(ctx, { "top_correlations", Y, B, y_stride, incy, records, kmax, k, idx, coef, score, err, errlen });
}
int ss_hip_top_correlations_f64(ss_hip_ctx* ctx, const double* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const void* records,
                                uint32_t kmax, uint32_t k, uint32_t* idx, double* coef, double* score, char* err, size_t errlen)
{
    return tc_dots_entry<double, TcAbsScorer<double>>(ctx, { "top_correlations", Y, B, y_stride, incy, records, kmax, k, idx, coef, score, err, errlen });
}

int ss_hip_extend_records_f32(ss_hip_ctx* ctx, const void* records, size_t B, uint32_t kmax, const uint32_t* idx, const float* coef, uint32_t k,
                              void* records_out, uint32_t* added, char* err, size_t errlen)
{
    return extend_entry<float>(ctx, records, B, kmax, idx, coef, k, records_out, added, err, errlen);
}
int ss_hip_extend_records_f64(ss_hip_ctx* ctx, const void* records, size_t B, uint32_t kmax, const uint32_t* idx, const double* coef, uint32_t k,
                              void* records_out, uint32_t* added, char* err, size_t errlen)
{
    return extend_entry<double>(ctx, records, B, kmax, idx, coef, k, records_out, added, err, errlen);
}

}  // extern "C"
