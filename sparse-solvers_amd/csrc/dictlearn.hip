// dictlearn.hip — the atom step of approximate K-SVD on the device, from compact records (include/ss_hip.h):
//   ss_hip_homotopy_atom_update_*.
//
// Given B signals, their compact records and a list of S atoms (columns), every requested atom j gets
//   g_j = sum_{b in U_j} w_b r_b + (sum_{b in U_j} w_b^2) a_j,   v_j = g_j / ||g_j||_2,
// r_b = y_b - A x_b, U_j = the counting signals (K_b <= kmax) whose record holds j, w_b = that record's value for j.  All atoms are
// computed against the SAME old dictionary and the same residuals (a Jacobi sweep).  Only the records' columns of A are read, one
// contiguous run of ldm elements each (ctx->At, [n_pad][ldm]), and then the users' rows of the residual block.
//
//   k_dl_count (counts, then fill) / k_dl_scan / k_dl_sort
//                    the inverted index: atom -> (signal, value) pairs, a CSR transpose of the records restricted to the requested
//                    atoms.  Counts and fill positions by integer atomics; then one wave per atom puts its list in ascending
//                    (signal, position in the record) by a rank sort — the order is a function of the records alone — and adds up
//                    sum w^2.  A column index >= n is found by k_dl_count before anything else runs; it is never used as an address.
//   k_dl_long        the list of a popular atom (more than 512 users, where the rank sort's |U|^2 / 64 steps a lane would start to
//                    show) is not sorted but written in order: one workgroup per such atom walks the records in ascending b, 256 at
//                    a time, every thread looks its record up for the atom, a prefix sum places the hits.  B * K reads per popular
//                    atom, linear in B; the list is the same (signal, position) order, so both ways give the same words.
//   k_dl_residual    grid = (row tile, signal of the chunk).  k_cls_residual's tile (256 threads, 1024 rows in registers, 16-byte
//                    loads along a column, eight columns in flight, rows m .. ldm-1 of At are zero): acc = A x_b over the record's
//                    entries, r = y - acc stored to R[b][0 .. ldm), the tile's sum of squares of r to the objective's partials.
//   k_dl_atoms       grid = (atom, row tile).  The accumulator starts from (sum w^2) a_j (first chunk) or from g as the previous
//                    chunk left it, takes w_b * R[b] of the atom's users in this chunk in list order, eight rows in flight, writes g;
//                    after the last chunk the tile's sum of squares of g goes to the norm's partials.
//   k_dl_finish      one workgroup per atom: ||g||_2 from the partials, changed / unchanged, v = g / ||g|| (or the stored column)
//                    through the caller's strides, usage.
//   k_dl_signal_sums / k_dl_objective   the objective: per signal, then over the signals.
// The residuals of B signals are held for a chunk of signals at a time (a byte budget; option "dl_chunk_max"): chunks in ascending
// order, g carried between them in memory — the chain of an atom is the unchunked one, word for word.
//
// SUMMATION ORDER (the tests' bounds follow from it; build flag -ffp-contract=off: products and sums are rounded separately):
//   acc_i      starts at 0 and takes v_k * A[i][col_k] one entry after the other in the record's order, in the context's precision
//              (ss_hip_reconstruct_records_*'s words);
//   r_b,i      = y_b,i - acc_i in the context's precision;
//   sum w^2    in double: w_b * w_b one user after the other in ascending b, rounded once to the context's precision;
//   g_j,i      starts at (sum w^2) * a_ij (the product in the context's precision) and takes w_b * r_b,i one user after the other
//              in ascending b, in the context's precision — a chain is never split across threads or workgroups;
//   ||g_j||^2, ||r_b||^2   in double, classify.hip's order: a thread adds its four squares in ascending row order, a wave its 64
//              thread sums by the butterfly lane ^ 32, ^ 16, ^ 8, ^ 4, ^ 2, ^ 1, then the wave sums one after the other: tiles
//              ascending, inside a tile waves 0, 1, 2, 3;
//   objective  = those ||r_b||^2 one after the other in ascending b (a truncated record adds +0);
//   v_j,i      = g_j,i / (T) sqrt(||g_j||^2); the atom is left as it is when that divisor is zero or not finite.
// No floating-point atomics; nothing depends on B, on the chunking, on the launch geometry or on which other atoms were requested.
// RANGE: no step has an absolute constant, so the words are an exact function of the units (A 2^a, Y 2^b, record values 2^(b-a): the
// same v_j and usage, the objective times 2^2b) as long as every intermediate is a normal number of its type: sum w^2 (of size
// 2^(2b-2a)) after its rounding to the context's precision, (sum w^2) a_ij and w_b r_b,i (2^(2b-a)) in the context's precision,
// ||g_j||^2 (2^(4b-2a)) and ||r_b||^2 (2^2b) in double.  Below it a sum rounds as a subnormal, above it ||g_j||^2 is infinite and the
// atom is left as it is (include/ss_hip.h states the same range; tests/test_gpu_scaling.py holds the kernels to it).
#include "ss_hip_internal.h"
#include "record_common.h"

#include <algorithm>
#include <cmath>
#include <limits>

namespace sship {

namespace {

constexpr size_t kDlChunkBytes = (size_t)256 << 20;      // byte budget of the residual block of one chunk (never changes a result)
constexpr uint32_t kDlChunkMax = 32768;                  // most signals per chunk (grid.y of k_dl_residual)
constexpr uint32_t kDlNone = 0xffffffffu;
constexpr uint32_t kDlRankMax = 512;                    // longest list one wave rank-sorts (512^2 / 64 steps a lane); longer ones: k_dl_long
constexpr uint32_t kDlLeft = 0x80000000u;                // usage bit: the atom had users but was left as it is

struct DictLearnState {
    unsigned char* index = nullptr;    // records (a host caller's), slot map, counts, offsets, partial sums, usage
    size_t index_bytes = 0;
    unsigned char* work = nullptr;     // the inverted index's lists, g [S][ldm], the residual block of a chunk, a host caller's signals
    size_t work_bytes = 0;
    unsigned char* vc = nullptr;       // apply: the changed atoms, contiguous
    size_t vc_bytes = 0;
};

DictLearnState* state_of(ss_hip_ctx* ctx)
{
    if (!ctx->dl) ctx->dl = new DictLearnState();
    return static_cast<DictLearnState*>(ctx->dl);
}

// ---- kernels -------------------------------------------------------------------------------------------------------------------

// one workgroup per signal.  FILL = false: counts[slot] += 1 for every entry of a counting record whose column is requested, and the
// first record with a column index >= n goes to bad; FILL = true: the entry takes the next free place of its atom's list
template <bool FILL>
__global__ __launch_bounds__(256)
void k_dl_count(const unsigned char* __restrict__ rec, size_t rb, uint32_t kmax, uint32_t n, const uint32_t* __restrict__ slot_of,
                uint32_t* __restrict__ counts, const uint32_t* __restrict__ off, uint32_t* __restrict__ pair_b, uint32_t* __restrict__ pair_e,
                uint32_t* __restrict__ bad)
{
    const uint32_t b = blockIdx.x;
    const unsigned char* r = rec + (size_t)b * rb;
    const uint32_t Krec = *reinterpret_cast<const uint32_t*>(r);
    const uint32_t K = Krec < kmax ? Krec : kmax;
    const uint32_t* idx = reinterpret_cast<const uint32_t*>(r + 16);
    for (uint32_t e = threadIdx.x; e < K; e += 256u) {
        const uint32_t col = idx[e];
        if (col >= n) { if (!FILL) atomicMin(bad, b); continue; }
        if (Krec > kmax) continue;                                     // a truncated record does not count
        const uint32_t s = slot_of ? slot_of[col] : col;
        if (s == kDlNone) continue;
        const uint32_t pos = atomicAdd(&counts[s], 1u);
        if (FILL) { pair_b[off[s] + pos] = b; pair_e[off[s] + pos] = e; }
    }
}

// off[0 .. S] = exclusive prefix sums of counts[0 .. S), off[S + 1] = the largest count (integers: the order is immaterial)
__global__ __launch_bounds__(1024)
void k_dl_scan(const uint32_t* __restrict__ counts, uint32_t S, uint32_t* __restrict__ off)
{
    __shared__ uint32_t s_part[1024];
    __shared__ uint32_t s_max;
    const uint32_t tid = threadIdx.x, per = (S + 1023u) / 1024u;
    const uint32_t lo = tid * per < S ? tid * per : S, hi = lo + per < S ? lo + per : S;
    uint32_t sum = 0, mx = 0;
    if (tid == 0) s_max = 0u;
    for (uint32_t i = lo; i < hi; ++i) { const uint32_t c = counts[i]; sum += c; mx = c > mx ? c : mx; }
    s_part[tid] = sum;
    __syncthreads();
    atomicMax(&s_max, mx);
    __syncthreads();
    if (tid == 0) {
        uint32_t run = 0;
        for (uint32_t t = 0; t < 1024u; ++t) { const uint32_t v = s_part[t]; s_part[t] = run; run += v; }
        off[S] = run;
        off[S + 1u] = s_max;                            // the longest list
    }
    __syncthreads();
    uint32_t run = s_part[tid];
    for (uint32_t i = lo; i < hi; ++i) { off[i] = run; run += counts[i]; }
}

// one wave per atom: its list in ascending (signal, position in the record) with the record's values beside it, then sum w^2
template <typename T>
__global__ __launch_bounds__(256)
void k_dl_sort(const unsigned char* __restrict__ rec, size_t rb, uint32_t kmax, const uint32_t* __restrict__ off, uint32_t S,
               const uint32_t* __restrict__ pair_b, const uint32_t* __restrict__ pair_e, uint32_t* __restrict__ sb, T* __restrict__ sw,
               T* __restrict__ s2)
{
    const uint32_t lane = threadIdx.x & 63u, s = blockIdx.x * 4u + (threadIdx.x >> 6);
    const bool mine = s < S && off[s + 1u] - off[s] <= kDlRankMax;     // (a longer list is k_dl_long's)
    const uint32_t beg = mine ? off[s] : 0u, end = mine ? off[s + 1u] : 0u;
    for (uint32_t i = beg + lane; i < end; i += 64u) {
        const uint32_t bi = pair_b[i], ei = pair_e[i];
        uint32_t rank = 0;
        for (uint32_t j = beg; j < end; ++j) {
            const uint32_t bj = pair_b[j];
            rank += (bj < bi || (bj == bi && pair_e[j] < ei)) ? 1u : 0u;
        }
        sb[beg + rank] = bi;
        sw[beg + rank] = load_val(rec + (size_t)bi * rb + 16 + (size_t)kmax * 4, ei, T(0));
    }
    __threadfence_block();
    __syncthreads();
    if (lane == 0u && mine) {
        double q = 0.0;
        for (uint32_t i = beg; i < end; ++i) { const double w = (double)sw[i]; q += w * w; }
        s2[s] = (T)q;
    }
}

// one workgroup per atom with more than kDlRankMax users: its list written in ascending (signal, position in the record) by a walk
// over the records, 256 signals a step, and sum w^2 (col = the atom's column; the hits are k_dl_count's: counting records only)
template <typename T>
__global__ __launch_bounds__(256)
void k_dl_long(const unsigned char* __restrict__ rec, size_t rb, uint32_t kmax, uint32_t B, const uint32_t* __restrict__ cols,
               const uint32_t* __restrict__ off, uint32_t* __restrict__ sb, T* __restrict__ sw, T* __restrict__ s2)
{
    __shared__ uint32_t s_wave[4];
    const uint32_t s = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t beg = off[s], end = off[s + 1u];
    if (end - beg <= kDlRankMax) return;
    const uint32_t col = cols ? cols[s] : s;
    uint32_t base = beg;
    for (uint32_t b0 = 0; b0 < B; b0 += 256u) {
        const uint32_t b = b0 + tid;
        const unsigned char* r = rec + (size_t)(b < B ? b : 0u) * rb;
        const uint32_t Krec = *reinterpret_cast<const uint32_t*>(r);
        const uint32_t K = (b < B && Krec <= kmax) ? Krec : 0u;
        const uint32_t* idx = reinterpret_cast<const uint32_t*>(r + 16);
        uint32_t cnt = 0;
        for (uint32_t e = 0; e < K; ++e) cnt += idx[e] == col ? 1u : 0u;
        uint32_t inc = cnt;
#pragma unroll
        for (uint32_t o = 1; o < 64u; o <<= 1) { const uint32_t v = (uint32_t)__shfl_up((int)inc, o); if (lane >= o) inc += v; }
        if (lane == 63u) s_wave[wave] = inc;
        __syncthreads();
        uint32_t pos = base + inc - cnt;
        for (uint32_t w = 0; w < wave; ++w) pos += s_wave[w];
        base += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        if (cnt != 0u) {
            const unsigned char* valp = r + 16 + (size_t)kmax * 4;
            for (uint32_t e = 0; e < K; ++e)
                if (idx[e] == col && pos < end) { sb[pos] = b; sw[pos] = load_val(valp, e, T(0)); ++pos; }
        }
        __syncthreads();
    }
    __threadfence_block();
    __syncthreads();
    if (tid == 0) {
        double q = 0.0;
        for (uint32_t i = beg; i < end; ++i) { const double w = (double)sw[i]; q += w * w; }
        s2[s] = (T)q;
    }
}

// R[b][0 .. ldm) = y_b - A x_b for the chunk's counting signals, part[b][tile][wave] = the tile's sums of squares (0 for a
// truncated record: its row of R is not written and nobody reads it)
template <typename T>
__global__ __launch_bounds__(256)
void k_dl_residual(const T* __restrict__ At, uint32_t ldm, uint32_t m, const T* __restrict__ Y, long long y_stride, long long incy,
                   const unsigned char* __restrict__ rec, size_t rb, uint32_t kmax, T* __restrict__ R, double* __restrict__ part)
{
    typedef typename ClsVec<T>::type V;
    constexpr uint32_t W = ClsVec<T>::W, L = ClsVec<T>::L, U = kClsInFlight;
    const uint32_t tile = blockIdx.x, b = blockIdx.y, ntiles = gridDim.x;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const unsigned char* r = rec + (size_t)b * rb;
    const uint32_t K = *reinterpret_cast<const uint32_t*>(r);
    if (K > kmax) {
        if (lane == 0u) part[((size_t)b * ntiles + tile) * 4u + wave] = 0.0;
        return;
    }
    const uint32_t* idx = reinterpret_cast<const uint32_t*>(r + 16);
    const unsigned char* valp = r + 16 + (size_t)kmax * 4;
    uint32_t row0[L];
#pragma unroll
    for (uint32_t j = 0; j < L; ++j) row0[j] = tile * kClsTileRows + j * (256u * W) + tid * W;
    const T* y = Y + (long long)b * y_stride;
    T yv[L][W], acc[L][W];
#pragma unroll
    for (uint32_t j = 0; j < L; ++j)
#pragma unroll
        for (uint32_t e = 0; e < W; ++e) {
            const uint32_t row = row0[j] + e;
            yv[j][e] = row < m ? y[(long long)row * incy] : T(0);
            acc[j][e] = T(0);
        }
    uint32_t k = 0;
    for (; k + U <= K; k += U) {                        // U columns' loads in flight, added in order
        V a[U][L];
        T v[U];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            const T* colp = At + (size_t)idx[k + u] * ldm;
            v[u] = load_val(valp, k + u, T(0));
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
    for (; k < K; ++k) {
        const T* colp = At + (size_t)idx[k] * ldm;
        const T v = load_val(valp, k, T(0));
#pragma unroll
        for (uint32_t j = 0; j < L; ++j) {
            const V a = row0[j] < ldm ? *reinterpret_cast<const V*>(colp + row0[j]) : V{};
#pragma unroll
            for (uint32_t e = 0; e < W; ++e) acc[j][e] = acc[j][e] + v * vget(a, e);
        }
    }
    double q = 0.0;
#pragma unroll
    for (uint32_t j = 0; j < L; ++j) {
        T d[W];
#pragma unroll
        for (uint32_t e = 0; e < W; ++e) {
            d[e] = yv[j][e] - acc[j][e];
            q += (double)d[e] * (double)d[e];
        }
        if (row0[j] < ldm) {
            V out;
            if constexpr (sizeof(T) == 4) out = V{ d[0], d[1], d[2], d[3] };
            else out = V{ d[0], d[1] };
            *reinterpret_cast<V*>(R + (size_t)b * ldm + row0[j]) = out;
        }
    }
    q = wave_sum(q);
    if (lane == 0u) part[((size_t)b * ntiles + tile) * 4u + wave] = q;
}

// first position in sb[lo .. hi) whose signal is >= b (the list is ascending)
__device__ inline uint32_t dl_lower_bound(const uint32_t* __restrict__ sb, uint32_t lo, uint32_t hi, uint32_t b)
{
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (sb[mid] < b) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

// the chunk holds signals b0 .. b1 - 1, R their residuals; cols == nullptr: atom s is column s
template <typename T>
__global__ __launch_bounds__(256)
void k_dl_atoms(const T* __restrict__ At, uint32_t ldm, const uint32_t* __restrict__ cols, const uint32_t* __restrict__ off,
                const uint32_t* __restrict__ sb, const T* __restrict__ sw, const T* __restrict__ s2, const T* __restrict__ R, uint32_t b0,
                uint32_t b1, int first, int last, T* G, double* __restrict__ partg)
{
    typedef typename ClsVec<T>::type V;
    constexpr uint32_t W = ClsVec<T>::W, L = ClsVec<T>::L, U = kClsInFlight;
    const uint32_t s = blockIdx.x, tile = blockIdx.y, ntiles = gridDim.y;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t beg = off[s], end = off[s + 1u];
    if (beg == end) return;                             // no user: k_dl_finish hands the stored column back
    uint32_t row0[L];
#pragma unroll
    for (uint32_t j = 0; j < L; ++j) row0[j] = tile * kClsTileRows + j * (256u * W) + tid * W;
    T* g = G + (size_t)s * ldm;
    T acc[L][W];
    if (first) {
        const T q = s2[s];
        const T* colp = At + (size_t)(cols ? cols[s] : s) * ldm;
#pragma unroll
        for (uint32_t j = 0; j < L; ++j) {
            const V a = row0[j] < ldm ? *reinterpret_cast<const V*>(colp + row0[j]) : V{};
#pragma unroll
            for (uint32_t e = 0; e < W; ++e) acc[j][e] = q * vget(a, e);
        }
    } else {
#pragma unroll
        for (uint32_t j = 0; j < L; ++j) {
            const V a = row0[j] < ldm ? *reinterpret_cast<const V*>(g + row0[j]) : V{};
#pragma unroll
            for (uint32_t e = 0; e < W; ++e) acc[j][e] = vget(a, e);
        }
    }
    const uint32_t lo = dl_lower_bound(sb, beg, end, b0), hi = dl_lower_bound(sb, lo, end, b1);
    uint32_t k = lo;
    for (; k + U <= hi; k += U) {                       // U users' rows in flight, added in order
        V a[U][L];
        T w[U];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            const T* rowp = R + (size_t)(sb[k + u] - b0) * ldm;
            w[u] = sw[k + u];
#pragma unroll
            for (uint32_t j = 0; j < L; ++j) a[u][j] = row0[j] < ldm ? *reinterpret_cast<const V*>(rowp + row0[j]) : V{};
        }
#pragma unroll
        for (uint32_t u = 0; u < U; ++u)
#pragma unroll
            for (uint32_t j = 0; j < L; ++j)
#pragma unroll
                for (uint32_t e = 0; e < W; ++e) acc[j][e] = acc[j][e] + w[u] * vget(a[u][j], e);
    }
    for (; k < hi; ++k) {
        const T* rowp = R + (size_t)(sb[k] - b0) * ldm;
        const T w = sw[k];
#pragma unroll
        for (uint32_t j = 0; j < L; ++j) {
            const V a = row0[j] < ldm ? *reinterpret_cast<const V*>(rowp + row0[j]) : V{};
#pragma unroll
            for (uint32_t e = 0; e < W; ++e) acc[j][e] = acc[j][e] + w * vget(a, e);
        }
    }
    double q = 0.0;
#pragma unroll
    for (uint32_t j = 0; j < L; ++j) {
#pragma unroll
        for (uint32_t e = 0; e < W; ++e) q += (double)acc[j][e] * (double)acc[j][e];
        if (row0[j] < ldm) {
            V out;
            if constexpr (sizeof(T) == 4) out = V{ acc[j][0], acc[j][1], acc[j][2], acc[j][3] };
            else out = V{ acc[j][0], acc[j][1] };
            *reinterpret_cast<V*>(g + row0[j]) = out;
        }
    }
    if (last) {
        q = wave_sum(q);
        if (lane == 0u) partg[((size_t)s * ntiles + tile) * 4u + wave] = q;
    }
}

// one workgroup per atom: out(i, s) = out[i * ors + s * ocs] = g / ||g|| or the stored column; out may be G itself (ors 1, ocs ldm)
template <typename T>
__global__ __launch_bounds__(256)
void k_dl_finish(const T* __restrict__ At, uint32_t ldm, uint32_t m, const uint32_t* __restrict__ cols, const uint32_t* __restrict__ off,
                 const T* G, const double* __restrict__ partg, uint32_t ntiles, T* out, long long ors, long long ocs,
                 uint32_t* __restrict__ usage)
{
    __shared__ T s_norm;
    __shared__ uint32_t s_ok;
    const uint32_t s = blockIdx.x, tid = threadIdx.x;
    const uint32_t cnt = off[s + 1u] - off[s];
    if (tid == 0) {
        uint32_t ok = 0u;
        T nrm = T(0);
        if (cnt != 0u) {
            double q = 0.0;
            for (uint32_t t = 0; t < ntiles * 4u; ++t) q += partg[(size_t)s * ntiles * 4u + t];
            nrm = (T)sqrt(q);
            ok = (nrm > T(0) && nrm <= std::numeric_limits<T>::max()) ? 1u : 0u;
        }
        s_norm = nrm;
        s_ok = ok;
        usage[s] = cnt != 0u && ok == 0u ? (cnt | kDlLeft) : cnt;
    }
    __syncthreads();
    const T nrm = s_norm;
    const bool ok = s_ok != 0u;
    const T* g = G + (size_t)s * ldm;
    const T* colp = At + (size_t)(cols ? cols[s] : s) * ldm;
    for (uint32_t i = tid; i < m; i += 256u) out[(long long)i * ors + (long long)s * ocs] = ok ? g[i] / nrm : colp[i];
}

// sig[b] = ||r_b||^2: the tile partials one after the other; then the objective: the signals one after the other
__global__ __launch_bounds__(256)
void k_dl_signal_sums(const double* __restrict__ part, uint32_t per, uint32_t B, double* __restrict__ sig)
{
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= B) return;
    double q = 0.0;
    for (uint32_t t = 0; t < per; ++t) q += part[(size_t)b * per + t];
    sig[b] = q;
}

__global__ __launch_bounds__(64)
void k_dl_objective(const double* __restrict__ sig, uint32_t B, double* __restrict__ obj)
{
    if (threadIdx.x != 0) return;
    double q = 0.0;
    for (uint32_t b = 0; b < B; ++b) q += sig[b];
    obj[0] = q;
}

// Vc[p][0 .. m) = column sel[p] of out (the changed atoms, contiguous, for the column replacement)
template <typename T>
__global__ __launch_bounds__(256)
void k_dl_gather(const T* __restrict__ out, long long ors, long long ocs, const uint32_t* __restrict__ sel, uint32_t m, T* __restrict__ Vc)
{
    const uint32_t p = blockIdx.x;
    const T* src = out + (long long)sel[p] * ocs;
    for (uint32_t i = threadIdx.x; i < m; i += 256u) Vc[(size_t)p * m + i] = src[(long long)i * ors];
}

// ---- host side -----------------------------------------------------------------------------------------------------------------

template <typename T>
int atom_update_impl(ss_hip_ctx* ctx, const T* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const void* records, uint32_t kmax,
                     const uint32_t* cols, size_t S, T* Vout, ptrdiff_t rs, ptrdiff_t cs, uint32_t* usage, double* objective, bool apply,
                     char* err, size_t errlen)
{
    static const char* who = "atom_update";
    HIPCHK(hipSetDevice(ctx->device));
    DictLearnState* ds = state_of(ctx);
    hipStream_t st = ctx->stream;
    const size_t m = ctx->m, n = ctx->n, rb = record_bytes(kmax, sizeof(T));
    const uint32_t ldm = ctx->ldm, ntiles = (uint32_t)((m + kClsTileRows - 1) / kClsTileRows), per = ntiles * 4u;
    const T* At = static_cast<const T*>(ctx->At);

    // ---- the list of atoms, on a host copy: nothing has been written when it fails ----
    std::vector<uint32_t> hc;
    if (cols) {
        hc.resize(S);
        if (on_device(cols)) HIPCHK(hipMemcpy(hc.data(), cols, S * sizeof(uint32_t), hipMemcpyDeviceToHost));
        else std::memcpy(hc.data(), cols, S * sizeof(uint32_t));
        std::vector<uint32_t> sorted(hc);
        std::sort(sorted.begin(), sorted.end());
        if (sorted.back() >= n) { set_err(err, errlen, "atom_update: column index out of range"); return SS_HIP_EINVAL; }
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) { set_err(err, errlen, "atom_update: a column is named twice"); return SS_HIP_EINVAL; }
    } else {
        S = n;
    }
    const uint32_t Su = (uint32_t)S, Bu = (uint32_t)B;
    const bool rec_dev = on_device(records), y_dev = on_device(Y), v_dev = Vout != nullptr && on_device(Vout);

    // ---- the index's fixed-size part ----
    auto carve_index = [&](unsigned char* base, auto&& use) {
        Carver cv(base);
        unsigned char* rec = rec_dev ? nullptr : cv.take<unsigned char>(B * rb);
        uint32_t* slot_of = cols ? cv.take<uint32_t>(n) : nullptr;
        uint32_t* dcols = cols ? cv.take<uint32_t>(S) : nullptr;
        uint32_t* counts = cv.take<uint32_t>(S);
        uint32_t* off = cv.take<uint32_t>(S + 2);         // (+ the total, + the longest list)
        uint32_t* bad = cv.take<uint32_t>(1);
        double* part = cv.take<double>(B * per);
        double* sig = cv.take<double>(B);
        double* obj = cv.take<double>(1);
        T* s2 = cv.take<T>(S);
        double* partg = cv.take<double>(S * per);
        uint32_t* dusage = cv.take<uint32_t>(S);
        uint32_t* sel = cv.take<uint32_t>(2 * S);         // apply: positions of the changed atoms, then their columns
        use(rec, slot_of, dcols, counts, off, bad, part, sig, obj, s2, partg, dusage, sel);
        return cv.off;
    };
    grow(ds->index, ds->index_bytes, carve_index(nullptr, [](auto...) {}), "hipMalloc(atom update index)");

    int rc = SS_HIP_OK;
    carve_index(ds->index, [&](unsigned char* rec, uint32_t* slot_of, uint32_t* dcols, uint32_t* counts, uint32_t* off, uint32_t* bad,
                               double* part, double* sig, double* obj, T* s2, double* partg, uint32_t* dusage, uint32_t* sel) {
        const unsigned char* recs = static_cast<const unsigned char*>(records);
        if (!rec_dev) { HIPCHK(hipMemcpyAsync(rec, recs, B * rb, hipMemcpyHostToDevice, st)); recs = rec; }
        std::vector<uint32_t> slots;
        if (cols) {
            slots.assign(n, kDlNone);
            for (size_t s = 0; s < S; ++s) slots[hc[s]] = (uint32_t)s;
            HIPCHK(hipMemcpyAsync(slot_of, slots.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(dcols, hc.data(), S * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        }
        HIPCHK(hipMemsetAsync(counts, 0, S * sizeof(uint32_t), st));
        HIPCHK(hipMemsetAsync(bad, 0xff, sizeof(uint32_t), st));
        hipLaunchKernelGGL((k_dl_count<false>), dim3(Bu), dim3(256), 0, st, recs, rb, kmax, (uint32_t)n, (const uint32_t*)slot_of, counts,
                           (const uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, bad);
        hipLaunchKernelGGL(k_dl_scan, dim3(1), dim3(1024), 0, st, (const uint32_t*)counts, Su, off);
        HIPCHK(hipGetLastError());
        uint32_t first_bad = kDlNone, tail[2] = { 0u, 0u };
        HIPCHK(hipMemcpyAsync(&first_bad, bad, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(tail, off + S, sizeof(tail), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));                // (the first host read: is a record invalid; how long are the lists)
        const uint32_t total = tail[0], longest = tail[1];
        if (first_bad != kDlNone) { rc = bad_index(first_bad, who, err, errlen); return; }

        // ---- the lists, g, the residual block of a chunk ----
        size_t chunk = std::max<size_t>(1, std::min<size_t>(kDlChunkMax, kDlChunkBytes / ((size_t)ldm * sizeof(T))));
        if (ctx->dl_chunk_max > 0) chunk = std::min<size_t>(chunk, (size_t)ctx->dl_chunk_max);
        chunk = std::min(chunk, B);
        auto carve_work = [&](unsigned char* base, auto&& use) {
            Carver cv(base);
            uint32_t* pair_b = cv.take<uint32_t>(total);
            uint32_t* pair_e = cv.take<uint32_t>(total);
            uint32_t* sb = cv.take<uint32_t>(total);
            T* sw = cv.take<T>(total);
            T* G = cv.take<T>(S * ldm);
            T* R = cv.take<T>(chunk * ldm);
            T* ybuf = y_dev ? nullptr : cv.take<T>(chunk * m);
            use(pair_b, pair_e, sb, sw, G, R, ybuf);
            return cv.off;
        };
        grow(ds->work, ds->work_bytes, carve_work(nullptr, [](auto...) {}), "hipMalloc(atom update workspace)");
        carve_work(ds->work, [&](uint32_t* pair_b, uint32_t* pair_e, uint32_t* sb, T* sw, T* G, T* R, T* ybuf) {
            if (total != 0u) {
                HIPCHK(hipMemsetAsync(counts, 0, S * sizeof(uint32_t), st));
                hipLaunchKernelGGL((k_dl_count<true>), dim3(Bu), dim3(256), 0, st, recs, rb, kmax, (uint32_t)n, (const uint32_t*)slot_of, counts,
                                   (const uint32_t*)off, pair_b, pair_e, bad);
                hipLaunchKernelGGL((k_dl_sort<T>), dim3((Su + 3u) / 4u), dim3(256), 0, st, recs, rb, kmax, (const uint32_t*)off, Su,
                                   (const uint32_t*)pair_b, (const uint32_t*)pair_e, sb, sw, s2);
                if (longest > kDlRankMax)
                    hipLaunchKernelGGL((k_dl_long<T>), dim3(Su), dim3(256), 0, st, recs, rb, kmax, Bu, (const uint32_t*)dcols, (const uint32_t*)off,
                                       sb, sw, s2);
                HIPCHK(hipGetLastError());
            }
            std::vector<T> tmp;
            if (total != 0u || objective) {
                for (size_t b0 = 0; b0 < B; b0 += chunk) {
                    const uint32_t Bc = (uint32_t)std::min(chunk, B - b0);
                    const T* yd = Y + (ptrdiff_t)b0 * y_stride;
                    long long ys = y_stride, yi = incy;
                    if (!y_dev) { upload_rows<T>(ctx, ybuf, Y, y_stride, incy, b0, Bc, tmp); yd = ybuf; ys = (long long)m; yi = 1; }
                    hipLaunchKernelGGL((k_dl_residual<T>), dim3(ntiles, Bc), dim3(kClsThreads), 0, st, At, ldm, (uint32_t)m, yd, ys, yi,
                                       recs + b0 * rb, rb, kmax, R, part + b0 * per);
                    if (total != 0u)
                        hipLaunchKernelGGL((k_dl_atoms<T>), dim3(Su, ntiles), dim3(kClsThreads), 0, st, At, ldm, (const uint32_t*)dcols,
                                           (const uint32_t*)off, (const uint32_t*)sb, (const T*)sw, (const T*)s2, (const T*)R, (uint32_t)b0,
                                           (uint32_t)b0 + Bc, b0 == 0 ? 1 : 0, b0 + Bc >= B ? 1 : 0, G, partg);
                    HIPCHK(hipGetLastError());
                }
            }
            if (objective) {
                hipLaunchKernelGGL(k_dl_signal_sums, dim3((Bu + 255u) / 256u), dim3(256), 0, st, (const double*)part, per, Bu, sig);
                hipLaunchKernelGGL(k_dl_objective, dim3(1), dim3(64), 0, st, (const double*)sig, Bu, obj);
                HIPCHK(hipGetLastError());
            }
            // ---- norms, changed / unchanged, V: straight into a device V, else in place over g ([S][ldm]) ----
            T* out = v_dev ? Vout : G;
            const long long ors = v_dev ? (long long)rs : 1ll, ocs = v_dev ? (long long)cs : (long long)ldm;
            hipLaunchKernelGGL((k_dl_finish<T>), dim3(Su), dim3(256), 0, st, At, ldm, (uint32_t)m, (const uint32_t*)dcols, (const uint32_t*)off,
                               (const T*)G, (const double*)partg, ntiles, out, ors, ocs, dusage);
            HIPCHK(hipGetLastError());
            if (objective) HIPCHK(hipMemcpyAsync(objective, obj, sizeof(double), hipMemcpyDefault, st));
            if (usage) HIPCHK(hipMemcpyAsync(usage, dusage, S * sizeof(uint32_t), hipMemcpyDefault, st));
            std::vector<uint32_t> hus;
            if (apply) {
                hus.resize(S);
                HIPCHK(hipMemcpyAsync(hus.data(), dusage, S * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            }
            if (Vout && !v_dev) {
                tmp.resize(S * m);
                HIPCHK(hipMemcpy2DAsync(tmp.data(), m * sizeof(T), G, (size_t)ldm * sizeof(T), m * sizeof(T), S, hipMemcpyDeviceToHost, st));
                HIPCHK(hipStreamSynchronize(st));
                for (size_t s = 0; s < S; ++s)
                    for (size_t i = 0; i < m; ++i) Vout[(ptrdiff_t)i * rs + (ptrdiff_t)s * cs] = tmp[s * m + i];
            }
            HIPCHK(hipStreamSynchronize(st));
            if (!apply) return;
            // ---- apply: the changed atoms as a device column list + a contiguous device V, through the column replacement ----
            std::vector<uint32_t> pos, ccols;
            for (size_t s = 0; s < S; ++s)
                if (hus[s] != 0u && (hus[s] & kDlLeft) == 0u) { pos.push_back((uint32_t)s); ccols.push_back(cols ? hc[s] : (uint32_t)s); }
            if (pos.empty()) return;
            const size_t nc = pos.size();
            grow(ds->vc, ds->vc_bytes, nc * m * sizeof(T), "hipMalloc(atom update: changed atoms)");
            T* Vc = reinterpret_cast<T*>(ds->vc);
            HIPCHK(hipMemcpyAsync(sel, pos.data(), nc * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(sel + S, ccols.data(), nc * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL((k_dl_gather<T>), dim3((uint32_t)nc), dim3(256), 0, st, (const T*)out, ors, ocs, (const uint32_t*)sel, (uint32_t)m, Vc);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(st));
            rc = replace_columns_device<T>(ctx, sel + S, ccols, Vc, 1ll, (long long)m, err, errlen);
        });
    });
    return rc;
}

template <typename T>
int atom_update_entry(ss_hip_ctx* ctx, const T* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const void* records, uint32_t kmax,
                      const uint32_t* cols, size_t S, T* V, ptrdiff_t rs, ptrdiff_t cs, uint32_t* usage, double* objective, uint32_t apply,
                      char* err, size_t errlen)
{
    static const char* who = "atom_update";
    const int rc = check_common<T>(ctx, who, records, true, kmax, err, errlen);
    if (rc != SS_HIP_OK) return rc;
    if (!Y) { set_err(err, errlen, "atom_update: Y must not be null"); return SS_HIP_EINVAL; }
    if (!V && apply == 0) { set_err(err, errlen, "atom_update: V must not be null unless the atoms are applied"); return SS_HIP_EINVAL; }
    if (incy <= 0 || y_stride <= 0 || (V && (rs <= 0 || cs <= 0))) { set_err(err, errlen, "atom_update: increments and strides must be positive"); return SS_HIP_EINVAL; }
    if (B == 0 || (cols && S == 0)) return SS_HIP_OK;         // (every argument above was checked all the same)
    if (cols && S > ctx->n) { set_err(err, errlen, "atom_update: more columns than the dictionary has (a column is named twice)"); return SS_HIP_EINVAL; }
    if (B >= 0x80000000ull || (unsigned long long)B * kmax >= 0xffffffffull) { set_err(err, errlen, "atom_update: B * kmax must stay below 2^32"); return SS_HIP_EINVAL; }
    return guarded(err, errlen, who, [&] {
        return atom_update_impl<T>(ctx, Y, B, y_stride, incy, records, kmax, cols, S, V, rs, cs, usage, objective, apply != 0, err, errlen);
    });
}

}  // namespace

// ---- the index and the residuals for the K-SVD sweep (ksvd.hip): the launches above on the context's stream, nothing else ----

hipError_t dl_launch_count(ss_hip_ctx* ctx, const unsigned char* recs, size_t rb, uint32_t kmax, uint32_t B, const uint32_t* slot_of, uint32_t S,
                           uint32_t* counts, uint32_t* off, uint32_t* bad)
{
    hipStream_t st = ctx->stream;
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)S * sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(bad, 0xff, sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_dl_count<false>), dim3(B), dim3(256), 0, st, recs, rb, kmax, (uint32_t)ctx->n, slot_of, counts, (const uint32_t*)nullptr,
                       (uint32_t*)nullptr, (uint32_t*)nullptr, bad);
    hipLaunchKernelGGL(k_dl_scan, dim3(1), dim3(1024), 0, st, (const uint32_t*)counts, S, off);
    return hipGetLastError();
}

template <typename T>
hipError_t dl_launch_lists(ss_hip_ctx* ctx, const unsigned char* recs, size_t rb, uint32_t kmax, uint32_t B, const uint32_t* slot_of,
                           const uint32_t* dcols, uint32_t S, uint32_t* counts, const uint32_t* off, uint32_t longest, uint32_t* pair_b,
                           uint32_t* pair_e, uint32_t* sb, T* sw, T* s2, uint32_t* bad)
{
    hipStream_t st = ctx->stream;
    const hipError_t e = hipMemsetAsync(counts, 0, (size_t)S * sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_dl_count<true>), dim3(B), dim3(256), 0, st, recs, rb, kmax, (uint32_t)ctx->n, slot_of, counts, off, pair_b, pair_e, bad);
    hipLaunchKernelGGL((k_dl_sort<T>), dim3((S + 3u) / 4u), dim3(256), 0, st, recs, rb, kmax, off, S, (const uint32_t*)pair_b,
                       (const uint32_t*)pair_e, sb, sw, s2);
    if (longest > kDlRankMax)
        hipLaunchKernelGGL((k_dl_long<T>), dim3(S), dim3(256), 0, st, recs, rb, kmax, B, dcols, off, sb, sw, s2);
    return hipGetLastError();
}

template <typename T>
hipError_t dl_launch_residuals(ss_hip_ctx* ctx, const T* yd, long long ys, long long yi, const unsigned char* recs, size_t rb, uint32_t kmax,
                               uint32_t Bc, T* R, double* part)
{
    const uint32_t ntiles = (uint32_t)((ctx->m + kClsTileRows - 1) / kClsTileRows);
    hipLaunchKernelGGL((k_dl_residual<T>), dim3(ntiles, Bc), dim3(kClsThreads), 0, ctx->stream, static_cast<const T*>(ctx->At), ctx->ldm,
                       (uint32_t)ctx->m, yd, ys, yi, recs, rb, kmax, R, part);
    return hipGetLastError();
}

hipError_t dl_launch_objective(ss_hip_ctx* ctx, const double* part, uint32_t per, uint32_t B, double* sig, double* obj)
{
    hipLaunchKernelGGL(k_dl_signal_sums, dim3((B + 255u) / 256u), dim3(256), 0, ctx->stream, part, per, B, sig);
    hipLaunchKernelGGL(k_dl_objective, dim3(1), dim3(64), 0, ctx->stream, (const double*)sig, B, obj);
    return hipGetLastError();
}

template <typename T>
hipError_t dl_launch_gather(ss_hip_ctx* ctx, const T* out, long long ors, long long ocs, const uint32_t* sel, uint32_t nc, T* Vc)
{
    hipLaunchKernelGGL((k_dl_gather<T>), dim3(nc), dim3(256), 0, ctx->stream, out, ors, ocs, sel, (uint32_t)ctx->m, Vc);
    return hipGetLastError();
}

template hipError_t dl_launch_gather<float>(ss_hip_ctx*, const float*, long long, long long, const uint32_t*, uint32_t, float*);
template hipError_t dl_launch_gather<double>(ss_hip_ctx*, const double*, long long, long long, const uint32_t*, uint32_t, double*);
template hipError_t dl_launch_lists<float>(ss_hip_ctx*, const unsigned char*, size_t, uint32_t, uint32_t, const uint32_t*, const uint32_t*, uint32_t,
                                           uint32_t*, const uint32_t*, uint32_t, uint32_t*, uint32_t*, uint32_t*, float*, float*, uint32_t*);
template hipError_t dl_launch_lists<double>(ss_hip_ctx*, const unsigned char*, size_t, uint32_t, uint32_t, const uint32_t*, const uint32_t*, uint32_t,
                                            uint32_t*, const uint32_t*, uint32_t, uint32_t*, uint32_t*, uint32_t*, double*, double*, uint32_t*);
template hipError_t dl_launch_residuals<float>(ss_hip_ctx*, const float*, long long, long long, const unsigned char*, size_t, uint32_t, uint32_t,
                                               float*, double*);
template hipError_t dl_launch_residuals<double>(ss_hip_ctx*, const double*, long long, long long, const unsigned char*, size_t, uint32_t, uint32_t,
                                                double*, double*);

void dictlearn_free(ss_hip_ctx* ctx)
{
    DictLearnState* ds = static_cast<DictLearnState*>(ctx->dl);
    if (!ds) return;
    if (ds->index) (void)hipFree(ds->index);
    if (ds->work) (void)hipFree(ds->work);
    if (ds->vc) (void)hipFree(ds->vc);
    delete ds;
    ctx->dl = nullptr;
}

}  // namespace sship

using namespace sship;

extern "C" {

int ss_hip_homotopy_atom_update_f32(ss_hip_ctx* ctx, const float* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const void* records,
                                    uint32_t kmax, const uint32_t* cols, size_t S, float* V, ptrdiff_t stride_row, ptrdiff_t stride_col,
                                    uint32_t* usage, double* objective, uint32_t apply, char* err, size_t errlen)
{
    return atom_update_entry<float>(ctx, Y, B, y_stride, incy, records, kmax, cols, S, V, stride_row, stride_col, usage, objective, apply, err, errlen);
}
int ss_hip_homotopy_atom_update_f64(ss_hip_ctx* ctx, const double* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const void* records,
                                    uint32_t kmax, const uint32_t* cols, size_t S, double* V, ptrdiff_t stride_row, ptrdiff_t stride_col,
                                    uint32_t* usage, double* objective, uint32_t apply, char* err, size_t errlen)
{
    return atom_update_entry<double>(ctx, Y, B, y_stride, incy, records, kmax, cols, S, V, stride_row, stride_col, usage, objective, apply, err, errlen);
}

}  // extern "C"
