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
// The host steps around the launches are the three learners' (learn_driver.h); this unit also holds their arena (learn_arena).
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
#include "learn_driver.h"

#include <algorithm>
#include <cmath>
#include <limits>

namespace sship {

namespace {

constexpr uint32_t kDlRankMax = 512;                    // longest list one wave rank-sorts (512^2 / 64 steps a lane); longer ones: k_dl_long

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
        if (row0[j] < ldm) cls_store<T>(R + (size_t)b * ldm + row0[j], d);
    }
    q = wave_sum(q);
    if (lane == 0u) part[((size_t)b * ntiles + tile) * 4u + wave] = q;
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
        if (row0[j] < ldm) cls_store<T>(g + row0[j], acc[j]);
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

// the index and the workspace: the common pieces (learn_driver.h), and the norm's partials, g and the residual block of a chunk
template <typename T> struct DlIndex : LearnIndex<T> {
    double* partg;
    void carve(Carver& cv, const LearnCall<T>& c)
    {
        this->head(cv, c, 1);
        partg = cv.take<double>(c.S * c.per);
        this->tail(cv, c);
    }
};

template <typename T> struct DlWork : LearnWork<T> {
    size_t chunk;
    T *G, *R;
    void carve(Carver& cv, const LearnCall<T>& c)
    {
        this->lists(cv, c);
        G = cv.take<T>(c.S * c.ldm);
        R = cv.take<T>(chunk * c.ldm);
        this->signals(cv, c, chunk);
    }
};

template <typename T>
int atom_update_impl(LearnCall<T>& c)
{
    ss_hip_ctx* ctx = c.ctx;
    int rc = learn_atoms(c);
    if (rc != SS_HIP_OK) return rc;
    hipStream_t st = ctx->stream;
    const size_t B = c.B, m = c.m, rb = c.rb;
    const uint32_t Su = (uint32_t)c.S, Bu = (uint32_t)B, ldm = c.ldm, ntiles = c.ntiles, per = c.per;
    const T* At = static_cast<const T*>(ctx->At);

    DlIndex<T> ix;
    learn_carve(learn_arena(ctx).index, ix, c, "hipMalloc(atom learning index)");
    if ((rc = learn_open(c, ix)) != SS_HIP_OK) return rc;

    // ---- the lists, g, the residual block of a chunk ----
    DlWork<T> wk;
    wk.chunk = learn_chunk(c);
    learn_carve(learn_arena(ctx).work, wk, c, "hipMalloc(atom learning workspace)");
    if (c.total != 0u)
        HIPCHK(dl_launch_lists<T>(ctx, c.place.din, rb, c.kmax, Bu, ix.slot_of, ix.dcols, Su, ix.counts, ix.off, c.longest, wk.pair_b, wk.pair_e, wk.sb,
                                  wk.sw, ix.s2, ix.bad));
    std::vector<T> tmp;
    if (c.total != 0u || c.objective) {
        for (size_t b0 = 0; b0 < B; b0 += wk.chunk) {
            const uint32_t Bc = (uint32_t)std::min(wk.chunk, B - b0);
            const ChunkSignals<T> y = chunk_signals<T>(ctx, c.Y, c.y_stride, c.incy, c.y_dev, wk.ybuf, b0, Bc, tmp);
            HIPCHK(dl_launch_residuals<T>(ctx, y.yd, y.ys, y.yi, c.place.din + b0 * rb, rb, c.kmax, Bc, wk.R, ix.part + b0 * per));
            if (c.total != 0u) {
                hipLaunchKernelGGL((k_dl_atoms<T>), dim3(Su, ntiles), dim3(kClsThreads), 0, st, At, ldm, (const uint32_t*)ix.dcols,
                                   (const uint32_t*)ix.off, (const uint32_t*)wk.sb, (const T*)wk.sw, (const T*)ix.s2, (const T*)wk.R, (uint32_t)b0,
                                   (uint32_t)b0 + Bc, b0 == 0 ? 1 : 0, b0 + Bc >= B ? 1 : 0, wk.G, ix.partg);
                HIPCHK(hipGetLastError());
            }
        }
    }
    if (c.objective) HIPCHK(dl_launch_objective(ctx, ix.part, per, Bu, ix.sig, ix.obj));
    // ---- norms, changed / unchanged, V: straight into a device V, else in place over g ([S][ldm]) ----
    const LearnOut<T> out = learn_out(c, wk.G);
    hipLaunchKernelGGL((k_dl_finish<T>), dim3(Su), dim3(256), 0, st, At, ldm, (uint32_t)m, (const uint32_t*)ix.dcols, (const uint32_t*)ix.off,
                       (const T*)wk.G, (const double*)ix.partg, ntiles, out.p, out.rs, out.cs, ix.dusage);
    HIPCHK(hipGetLastError());
    return learn_finish<T>(c, ix, 1, wk.G, out);
}

template <typename T>
int atom_update_entry(ss_hip_ctx* ctx, const T* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const void* records, uint32_t kmax,
                      const uint32_t* cols, size_t S, T* V, ptrdiff_t rs, ptrdiff_t cs, uint32_t* usage, double* objective, uint32_t apply,
                      char* err, size_t errlen)
{
    LearnCall<T> c{ ctx, "atom_update", Y, B, y_stride, incy, records, kmax, nullptr, cols, S, V, rs, cs, usage, objective, apply != 0, err, errlen };
    LearnRules r{};
    r.null_y = "Y must not be null";
    if (!V && apply == 0) r.own = "V must not be null unless the atoms are applied";
    bool empty = false;
    const int rc = learn_check_args(c, r, empty);
    if (rc != SS_HIP_OK || empty) return rc;
    return guarded(err, errlen, c.who, [&] { return atom_update_impl<T>(c); });
}

}  // namespace

// ---- the launches of the kernels above on the context's stream, nothing else: the three learners' (learn_driver.h), this unit's included ----

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

LearnArena& learn_arena(ss_hip_ctx* ctx)
{
    return part<LearnArena>(ctx->learn);
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
