// wdictlearn.hip — the atom step of dictionary learning under a non-negative weight per row and signal, from compact records
// (include/ss_hip.h):
//   ss_hip_weighted_atom_update_*.
//
// min sum_b sum_k w_kb (y_b - A x_b)_k^2 over the atoms, the records' values fixed.  For every requested atom j, with U_j the counting
// signals (K_b <= kmax) whose record holds j in ascending (b, position in the record), c_b that record's value and r_b = y_b - A x_b
// the UNWEIGHTED residual (dictlearn.hip's k_dl_residual, its words):
//   num_k = sum_{b in U_j} (w_kb c_b) r_kb      den_k = sum_{b in U_j} (w_kb c_b) c_b      row k is SEEN when den_k > 0
//   d_k   = a_kj + num_k / den_k (seen),  a_kj (not seen)      nu = ||d||_2      v_j = d / nu      c_b <- c_b nu in records_out
// d is the row-wise weighted least-squares minimiser over the atom for fixed c; the values are rescaled so that v_j c'_b = d c_b.
// The atom is left as it is (the stored column bit for bit, no record value touched) when U_j is empty, when no row is seen or when
// nu is zero or not finite.  All atoms see the same old dictionary and residuals (a Jacobi step, like dictlearn.hip's).  The chains
// cannot be had from dictlearn.hip's by scaling Y: the weights differ per signal while the atom is shared.
//
//   dl_launch_count / dl_launch_lists / dl_launch_residuals / dl_launch_objective / dl_launch_gather
//                    dictlearn.hip's kernels through its launches: the inverted index atom -> (signal, value) in ascending (signal,
//                    position) order with its rank-sort and long-list paths, the residual block of a chunk, the objective's two
//                    sums, the changed atoms gathered for the column replacement.
//   weights_on_device   weighted.hip's staging and device check of the weights (the first offender, before anything is written).
//   k_wdl_stage      grid = (row tile, signal of the chunk).  Wb[b][0 .. ldm) = w_b, zero from row m on: the caller's rows are m long
//                    at any stride >= m, so they are read as scalars and stored as the 16-byte vectors k_wdl_atoms loads.  The same
//                    pass reads the tile of R[b] and overwrites k_dl_residual's partial sums with the weighted ones.
//   k_wdl_atoms      grid = (atom, row tile of 1024), k_dl_atoms' register tile with two accumulator sets.  num and den start at 0
//                    (first chunk) or as the previous chunk left them ([S][ldm] each), and take the atom's users in this chunk in list
//                    order, eight users' rows of R and of Wb in flight.
//   k_wdl_finish     one workgroup per atom: d (in place over num), ||d||^2, nu, changed / left, v = d / nu (or the stored column)
//                    through the caller's strides, usage, nu per slot (0 for an atom that is left).
//   k_wdl_scale      one workgroup per record: the record copied word for word (out of place), then the values of changed atoms
//                    multiplied by their nu through the slot map: integer work plus one product per entry.
// The residuals and weights of B signals are held for a chunk of signals at a time (dictlearn.hip's byte budget for each block; option
// "dl_chunk_max"): chunks in ascending order, num and den carried between them in memory — the chain of a row is the unchunked one.
//
// SUMMATION ORDER (the tests' bounds follow from it; build flag -ffp-contract=off: products and sums are rounded separately):
//   r_b        dictlearn.hip's words;
//   t          = w_kb * c_b, one rounding in T;
//   num_k      starts at 0 and takes t * r_kb, den_k starts at 0 and takes t * c_b, one user after the other in list order, every
//              product and every sum rounded in T — a chain is never split across threads, workgroups or chunks;
//   d_k        = a_kj + num_k / den_k where den_k > 0: one division, one addition, one comparison, no arithmetic masks;
//   ||d||^2    in double, dictlearn.hip's order: a thread's squares in ascending row order, the butterfly lane ^ 32 .. ^ 1, then the
//              wave sums one after the other: tiles ascending, inside a tile waves 0, 1, 2, 3;
//   nu         = (T) sqrt(||d||^2);  v_k = d_k / nu;  c'_b = c_b * nu, one product in T;
//   objective  every square of r_kb formed in double and multiplied by (double) w_kb before it enters k_dl_residual's sums, then
//              k_dl_signal_sums and k_dl_objective: with every weight exactly 1 dictlearn.hip's objective, word for word.
// With W == 1 the atoms agree with dictlearn.hip's only to rounding, not bit for bit: that unit starts its chain at (sum c^2) a_j
// with sum c^2 summed in double, here den is a chain in T per row.
// No floating-point atomics; nothing depends on B, on the chunking, on the launch geometry, on which other atoms were requested or on
// w_stride == 0 against repeated rows.
// RANGE: no step has an absolute constant.  Under A 2^a, Y 2^b, record values 2^(b-a), W 2^c: the same v and usage, nu times 2^a (so
// records_out holds the unscaled call's values times 2^b), the objective times 2^(2b+c) — as long as every intermediate is a normal
// number of its type: t (2^(c+b-a)), t r (2^(c+2b-a)), t c (2^(c+2b-2a)) and num / den (2^a) in T, ||d||^2 (2^2a) and w r^2 in double.
// RESOURCES (the compiler's report for gfx950, -O3): k_wdl_atoms<float> 98 VGPRs, 4 waves a SIMD; k_wdl_atoms<double> 152 VGPRs, 3
// waves a SIMD; no scratch and no spill in either, nor in the other six instantiations (at most 40 VGPRs).  The loads of the users'
// rows are 16 bytes wide: a row of R and of Wb starts at a multiple of ldm elements, a multiple of 16 bytes, which a caller's weight
// row (m long at any stride >= m: m = 70, w_stride = m + 3) does not — hence the staging.
#include "ss_hip_internal.h"
#include "record_common.h"

#include <algorithm>
#include <cmath>
#include <limits>

namespace sship {

namespace {

constexpr size_t kWdlChunkBytes = (size_t)256 << 20;     // byte budget of each of a chunk's two blocks, R and Wb (never changes a result)
constexpr uint32_t kWdlChunkMax = 32768;                 // most signals per chunk (grid.y of the residual kernel)
constexpr uint32_t kWdlNone = 0xffffffffu;
constexpr uint32_t kWdlLeft = 0x80000000u;               // usage bit: the atom had users but was left as it is

struct WdlState {
    unsigned char* index = nullptr;    // records (staged), slot map, counts, offsets, partial sums, usage, nu
    size_t index_bytes = 0;
    unsigned char* work = nullptr;     // the lists, num and den [S][ldm], the residual and weight blocks of a chunk, a host caller's signals
    size_t work_bytes = 0;
    unsigned char* vc = nullptr;       // apply: the changed atoms, contiguous
    size_t vc_bytes = 0;
};

WdlState* state_of(ss_hip_ctx* ctx)
{
    if (!ctx->wdl) ctx->wdl = new WdlState();
    return static_cast<WdlState*>(ctx->wdl);
}

__device__ inline void store_val(unsigned char* p, uint32_t e, float v) { reinterpret_cast<float*>(p)[e] = v; }
__device__ inline void store_val(unsigned char* p, uint32_t e, double v)
{
    uint32_t* w = reinterpret_cast<uint32_t*>(p) + 2u * e;       // (4-byte aligned only when kmax is odd: record_common.h, load_val)
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    w[0] = (uint32_t)u;
    w[1] = (uint32_t)(u >> 32);
}

template <typename T> __device__ inline typename ClsVec<T>::type wdl_pack(const T* d);
template <> __device__ inline float4 wdl_pack<float>(const float* d) { return float4{ d[0], d[1], d[2], d[3] }; }
template <> __device__ inline double2 wdl_pack<double>(const double* d) { return double2{ d[0], d[1] }; }

// first position in sb[lo .. hi) whose signal is >= b (the list is ascending)
__device__ inline uint32_t wdl_lower_bound(const uint32_t* __restrict__ sb, uint32_t lo, uint32_t hi, uint32_t b)
{
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (sb[mid] < b) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

// ---- kernels -------------------------------------------------------------------------------------------------------------------

// Wt: the chunk's weights (row b at Wt[b * w_stride], m long); Wb, R: [chunk][ldm]; part[b][tile][wave] = the tile's weighted sums of
// squares (0 for a truncated record, whose row of R was never written)
template <typename T>
__global__ __launch_bounds__(256)
void k_wdl_stage(const T* __restrict__ Wt, long long w_stride, uint32_t m, uint32_t ldm, const unsigned char* __restrict__ rec, size_t rb,
                 uint32_t kmax, const T* __restrict__ R, T* __restrict__ Wb, double* __restrict__ part)
{
    typedef typename ClsVec<T>::type V;
    constexpr uint32_t VW = ClsVec<T>::W, L = ClsVec<T>::L;
    const uint32_t tile = blockIdx.x, b = blockIdx.y, ntiles = gridDim.x;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const bool counts = *reinterpret_cast<const uint32_t*>(rec + (size_t)b * rb) <= kmax;
    const T* w = Wt + (long long)b * w_stride;
    double q = 0.0;
#pragma unroll
    for (uint32_t j = 0; j < L; ++j) {
        const uint32_t row0 = tile * kClsTileRows + j * (256u * VW) + tid * VW;
        if (row0 >= ldm) continue;
        T wv[VW];
#pragma unroll
        for (uint32_t e = 0; e < VW; ++e) wv[e] = row0 + e < m ? w[row0 + e] : T(0);
        *reinterpret_cast<V*>(Wb + (size_t)b * ldm + row0) = wdl_pack<T>(wv);
        if (counts) {
            const V rv = *reinterpret_cast<const V*>(R + (size_t)b * ldm + row0);
#pragma unroll
            for (uint32_t e = 0; e < VW; ++e) q += ((double)vget(rv, e) * (double)vget(rv, e)) * (double)wv[e];
        }
    }
    q = wave_sum(q);
    if (lane == 0u) part[((size_t)b * ntiles + tile) * 4u + wave] = counts ? q : 0.0;
}

// the chunk holds signals b0 .. b1 - 1, R their residuals, Wb their weights
template <typename T>
__global__ __launch_bounds__(256)
void k_wdl_atoms(uint32_t ldm, const uint32_t* __restrict__ off, const uint32_t* __restrict__ sb, const T* __restrict__ sw,
                 const T* __restrict__ R, const T* __restrict__ Wb, uint32_t b0, uint32_t b1, int first, T* Num, T* Den)
{
    typedef typename ClsVec<T>::type V;
    constexpr uint32_t VW = ClsVec<T>::W, L = ClsVec<T>::L, U = kClsInFlight;
    const uint32_t s = blockIdx.x, tile = blockIdx.y, tid = threadIdx.x;
    const uint32_t beg = off[s], end = off[s + 1u];
    if (beg == end) return;                             // no user: k_wdl_finish hands the stored column back
    uint32_t row0[L];
#pragma unroll
    for (uint32_t j = 0; j < L; ++j) row0[j] = tile * kClsTileRows + j * (256u * VW) + tid * VW;
    T* nump = Num + (size_t)s * ldm;
    T* denp = Den + (size_t)s * ldm;
    T num[L][VW], den[L][VW];
#pragma unroll
    for (uint32_t j = 0; j < L; ++j) {
        V a = V{}, d = V{};
        if (!first && row0[j] < ldm) {
            a = *reinterpret_cast<const V*>(nump + row0[j]);
            d = *reinterpret_cast<const V*>(denp + row0[j]);
        }
#pragma unroll
        for (uint32_t e = 0; e < VW; ++e) { num[j][e] = vget(a, e); den[j][e] = vget(d, e); }
    }
    const uint32_t lo = wdl_lower_bound(sb, beg, end, b0), hi = wdl_lower_bound(sb, lo, end, b1);
    uint32_t k = lo;
    for (; k + U <= hi; k += U) {                       // U users' rows of R and of Wb in flight, added in order
        V r[U][L], w[U][L];
        T c[U];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            const size_t rowoff = (size_t)(sb[k + u] - b0) * ldm;
            c[u] = sw[k + u];
#pragma unroll
            for (uint32_t j = 0; j < L; ++j) {
                r[u][j] = row0[j] < ldm ? *reinterpret_cast<const V*>(R + rowoff + row0[j]) : V{};
                w[u][j] = row0[j] < ldm ? *reinterpret_cast<const V*>(Wb + rowoff + row0[j]) : V{};
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < U; ++u)
#pragma unroll
            for (uint32_t j = 0; j < L; ++j)
#pragma unroll
                for (uint32_t e = 0; e < VW; ++e) {
                    const T t = vget(w[u][j], e) * c[u];
                    num[j][e] = num[j][e] + t * vget(r[u][j], e);
                    den[j][e] = den[j][e] + t * c[u];
                }
    }
    for (; k < hi; ++k) {
        const size_t rowoff = (size_t)(sb[k] - b0) * ldm;
        const T c = sw[k];
#pragma unroll
        for (uint32_t j = 0; j < L; ++j) {
            const V r = row0[j] < ldm ? *reinterpret_cast<const V*>(R + rowoff + row0[j]) : V{};
            const V w = row0[j] < ldm ? *reinterpret_cast<const V*>(Wb + rowoff + row0[j]) : V{};
#pragma unroll
            for (uint32_t e = 0; e < VW; ++e) {
                const T t = vget(w, e) * c;
                num[j][e] = num[j][e] + t * vget(r, e);
                den[j][e] = den[j][e] + t * c;
            }
        }
    }
#pragma unroll
    for (uint32_t j = 0; j < L; ++j)
        if (row0[j] < ldm) {
            *reinterpret_cast<V*>(nump + row0[j]) = wdl_pack<T>(num[j]);
            *reinterpret_cast<V*>(denp + row0[j]) = wdl_pack<T>(den[j]);
        }
}

// one workgroup per atom: Num[s] becomes d; out(i, s) = out[i * ors + s * ocs] = d / nu or the stored column; out may be Num itself
// (ors 1, ocs ldm); nu[s] = the atom's nu, 0 when it is left as it is
template <typename T>
__global__ __launch_bounds__(256)
void k_wdl_finish(const T* __restrict__ At, uint32_t ldm, uint32_t m, const uint32_t* __restrict__ cols, const uint32_t* __restrict__ off,
                  T* Num, const T* __restrict__ Den, uint32_t ntiles, T* out, long long ors, long long ocs, uint32_t* __restrict__ usage,
                  T* __restrict__ nu)
{
    typedef typename ClsVec<T>::type V;
    constexpr uint32_t VW = ClsVec<T>::W, L = ClsVec<T>::L;
    __shared__ double s_wave[4];
    __shared__ uint32_t s_seen[4];
    __shared__ T s_nu;
    __shared__ uint32_t s_ok;
    const uint32_t s = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t cnt = off[s + 1u] - off[s];
    const T* colp = At + (size_t)(cols ? cols[s] : s) * ldm;
    T* d = Num + (size_t)s * ldm;
    const T* denp = Den + (size_t)s * ldm;
    double total = 0.0;
    uint32_t seen_any = 0u;
    if (cnt != 0u) {
        for (uint32_t tile = 0; tile < ntiles; ++tile) {
            double q = 0.0;
            uint32_t seen = 0u;
#pragma unroll
            for (uint32_t j = 0; j < L; ++j) {
                const uint32_t row0 = tile * kClsTileRows + j * (256u * VW) + tid * VW;
                if (row0 >= ldm) continue;
                const V a = *reinterpret_cast<const V*>(colp + row0);
                const V nv = *reinterpret_cast<const V*>(d + row0);
                const V dv = *reinterpret_cast<const V*>(denp + row0);
                T dk[VW];
#pragma unroll
                for (uint32_t e = 0; e < VW; ++e) {
                    const bool is_seen = vget(dv, e) > T(0);
                    dk[e] = is_seen ? vget(a, e) + vget(nv, e) / vget(dv, e) : vget(a, e);
                    seen |= is_seen ? 1u : 0u;
                    q += (double)dk[e] * (double)dk[e];
                }
                *reinterpret_cast<V*>(d + row0) = wdl_pack<T>(dk);
            }
            q = wave_sum(q);
            seen = __any((int)seen) ? 1u : 0u;
            if (lane == 0u) { s_wave[wave] = q; s_seen[wave] = seen; }
            __syncthreads();
            if (tid == 0) {
                total += s_wave[0]; total += s_wave[1]; total += s_wave[2]; total += s_wave[3];
                seen_any |= s_seen[0] | s_seen[1] | s_seen[2] | s_seen[3];
            }
            __syncthreads();
        }
    }
    if (tid == 0) {
        const T nrm = (T)sqrt(total);
        const uint32_t ok = (cnt != 0u && seen_any != 0u && nrm > T(0) && nrm <= std::numeric_limits<T>::max()) ? 1u : 0u;
        s_nu = nrm;
        s_ok = ok;
        usage[s] = cnt != 0u && ok == 0u ? (cnt | kWdlLeft) : cnt;
        nu[s] = ok != 0u ? nrm : T(0);
    }
    __threadfence_block();
    __syncthreads();
    const T nrm = s_nu;
    const bool ok = s_ok != 0u;
    for (uint32_t i = tid; i < m; i += 256u) out[(long long)i * ors + (long long)s * ocs] = ok ? d[i] / nrm : colp[i];
}

// one workgroup per record: out[b] = in[b] word for word (out != in), then value * nu[slot] for the entries of a counting record whose
// atom changed (nu != 0).  slot_of == nullptr: atom s is column s
template <typename T>
__global__ __launch_bounds__(256)
void k_wdl_scale(const unsigned char* in, unsigned char* out, size_t rb, uint32_t kmax, const uint32_t* __restrict__ slot_of,
                 const T* __restrict__ nu)
{
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    const unsigned char* ri = in + (size_t)b * rb;
    unsigned char* ro = out + (size_t)b * rb;
    const uint32_t K = *reinterpret_cast<const uint32_t*>(ri);
    const uint32_t* idx = reinterpret_cast<const uint32_t*>(ri + 16);
    const unsigned char* vin = ri + 16 + (size_t)kmax * 4;
    if (ro != ri) {                                     // (disjoint: the entry point refuses a partial overlap)
        const uint32_t words = (uint32_t)(rb / 4);
        for (uint32_t w = tid; w < words; w += 256u) reinterpret_cast<uint32_t*>(ro)[w] = reinterpret_cast<const uint32_t*>(ri)[w];
        __threadfence_block();
        __syncthreads();                                // (the products below land after the copy of their words)
    }
    if (K > kmax) return;                               // a truncated record does not count
    unsigned char* vout = ro + 16 + (size_t)kmax * 4;
    for (uint32_t e = tid; e < K; e += 256u) {          // (in place an entry is read and written by this thread alone)
        const uint32_t col = idx[e];
        const uint32_t s = slot_of ? slot_of[col] : col;
        if (s == kWdlNone) continue;
        const T f = nu[s];
        if (f != T(0)) store_val(vout, e, load_val(vin, e, T(0)) * f);
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------

template <typename T>
int wdl_impl(ss_hip_ctx* ctx, const T* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const T* W, ptrdiff_t w_stride, const void* records,
             uint32_t kmax, void* records_out, const uint32_t* cols, size_t S, T* Vout, ptrdiff_t rs, ptrdiff_t cs, uint32_t* usage,
             double* objective, bool apply, char* err, size_t errlen)
{
    static const char* who = "weighted_atom_update";
    HIPCHK(hipSetDevice(ctx->device));
    WdlState* ds = state_of(ctx);
    hipStream_t st = ctx->stream;
    const size_t m = ctx->m, n = ctx->n, rb = record_bytes(kmax, sizeof(T));
    const uint32_t ldm = ctx->ldm, ntiles = (uint32_t)((m + kClsTileRows - 1) / kClsTileRows), per = ntiles * 4u;
    const T* At = static_cast<const T*>(ctx->At);

    // ---- the list of atoms, on a host copy: nothing has been written when it fails ----
    std::vector<uint32_t> hc, slots;
    if (cols) {
        hc.resize(S);
        if (on_device(cols)) HIPCHK(hipMemcpy(hc.data(), cols, S * sizeof(uint32_t), hipMemcpyDeviceToHost));
        else std::memcpy(hc.data(), cols, S * sizeof(uint32_t));
        std::vector<uint32_t> sorted(hc);
        std::sort(sorted.begin(), sorted.end());
        if (sorted.back() >= n) { set_err(err, errlen, "weighted_atom_update: column index out of range"); return SS_HIP_EINVAL; }
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) { set_err(err, errlen, "weighted_atom_update: a column is named twice"); return SS_HIP_EINVAL; }
    } else {
        S = n;
    }
    const uint32_t Su = (uint32_t)S, Bu = (uint32_t)B;
    const bool in_dev = on_device(records), out_dev = records_out != nullptr && on_device(records_out), y_dev = on_device(Y);
    const bool v_dev = Vout != nullptr && on_device(Vout), staged = !in_dev || (records_out != nullptr && !out_dev);

    // ---- the index's fixed-size part ----
    auto carve_index = [&](unsigned char* base, auto&& use) {
        Carver cv(base);
        unsigned char* stage = staged ? cv.take<unsigned char>(B * rb) : nullptr;
        uint32_t* slot_of = cols ? cv.take<uint32_t>(n) : nullptr;
        uint32_t* dcols = cols ? cv.take<uint32_t>(S) : nullptr;
        uint32_t* counts = cv.take<uint32_t>(S);
        uint32_t* off = cv.take<uint32_t>(S + 2);         // (+ the total, + the longest list)
        uint32_t* bad = cv.take<uint32_t>(1);
        double* part = cv.take<double>(B * per);
        double* sig = cv.take<double>(B);
        double* obj = cv.take<double>(1);
        T* s2 = cv.take<T>(S);                            // (the index's sum c^2: not used here)
        T* nu = cv.take<T>(S);
        uint32_t* dusage = cv.take<uint32_t>(S);
        uint32_t* sel = cv.take<uint32_t>(2 * S);         // apply: positions of the changed atoms, then their columns
        use(stage, slot_of, dcols, counts, off, bad, part, sig, obj, s2, nu, dusage, sel);
        return cv.off;
    };
    grow(ds->index, ds->index_bytes, carve_index(nullptr, [](auto...) {}), "hipMalloc(weighted atom update index)");

    int rc = SS_HIP_OK;
    carve_index(ds->index, [&](unsigned char* stage, uint32_t* slot_of, uint32_t* dcols, uint32_t* counts, uint32_t* off, uint32_t* bad,
                               double* part, double* sig, double* obj, T* s2, T* nu, uint32_t* dusage, uint32_t* sel) {
        // din: the input records on the device; dout: where the output records are written there (a host caller's: the staging, in
        // place when the input is staged too)
        const unsigned char* din = static_cast<const unsigned char*>(records);
        if (!in_dev) { HIPCHK(hipMemcpyAsync(stage, records, B * rb, hipMemcpyHostToDevice, st)); din = stage; }
        unsigned char* dout = !records_out ? nullptr : out_dev ? static_cast<unsigned char*>(records_out) : stage;
        if (cols) {
            slots.assign(n, kWdlNone);
            for (size_t s = 0; s < S; ++s) slots[hc[s]] = (uint32_t)s;
            HIPCHK(hipMemcpyAsync(slot_of, slots.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(dcols, hc.data(), S * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        }
        HIPCHK(dl_launch_count(ctx, din, rb, kmax, Bu, slot_of, Su, counts, off, bad));
        uint32_t first_bad = kWdlNone, tail[2] = { 0u, 0u };
        HIPCHK(hipMemcpyAsync(&first_bad, bad, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(tail, off + S, sizeof(tail), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));                // (the first host read: is a record invalid; how long are the lists)
        const uint32_t total = tail[0], longest = tail[1];
        if (first_bad != kWdlNone) { rc = bad_index(first_bad, who, err, errlen); return; }

        // ---- the weights where the kernels read them, checked: the last thing that can fail before an output is written ----
        const T* Wd = nullptr;
        long long wsd = 0;
        if ((rc = weights_on_device<T>(ctx, who, W, B, w_stride, &Wd, &wsd, err, errlen)) != SS_HIP_OK) return;

        // ---- the lists, num and den, the residual and weight blocks of a chunk ----
        size_t chunk = std::max<size_t>(1, std::min<size_t>(kWdlChunkMax, kWdlChunkBytes / ((size_t)ldm * sizeof(T))));
        if (ctx->dl_chunk_max > 0) chunk = std::min<size_t>(chunk, (size_t)ctx->dl_chunk_max);
        chunk = std::min(chunk, B);
        auto carve_work = [&](unsigned char* base, auto&& use) {
            Carver cv(base);
            uint32_t* pair_b = cv.take<uint32_t>(total);
            uint32_t* pair_e = cv.take<uint32_t>(total);
            uint32_t* sb = cv.take<uint32_t>(total);
            T* sw = cv.take<T>(total);
            T* Num = cv.take<T>(S * ldm);
            T* Den = cv.take<T>(S * ldm);
            T* R = cv.take<T>(chunk * ldm);
            T* Wb = cv.take<T>(chunk * ldm);
            T* ybuf = y_dev ? nullptr : cv.take<T>(chunk * m);
            use(pair_b, pair_e, sb, sw, Num, Den, R, Wb, ybuf);
            return cv.off;
        };
        grow(ds->work, ds->work_bytes, carve_work(nullptr, [](auto...) {}), "hipMalloc(weighted atom update workspace)");
        carve_work(ds->work, [&](uint32_t* pair_b, uint32_t* pair_e, uint32_t* sb, T* sw, T* Num, T* Den, T* R, T* Wb, T* ybuf) {
            if (total != 0u)
                HIPCHK(dl_launch_lists<T>(ctx, din, rb, kmax, Bu, slot_of, dcols, Su, counts, off, longest, pair_b, pair_e, sb, sw, s2, bad));
            std::vector<T> tmp;
            if (total != 0u || objective) {
                for (size_t b0 = 0; b0 < B; b0 += chunk) {
                    const uint32_t Bc = (uint32_t)std::min(chunk, B - b0);
                    const T* yd = Y + (ptrdiff_t)b0 * y_stride;
                    long long ys = y_stride, yi = incy;
                    if (!y_dev) { upload_rows<T>(ctx, ybuf, Y, y_stride, incy, b0, Bc, tmp); yd = ybuf; ys = (long long)m; yi = 1; }
                    HIPCHK(dl_launch_residuals<T>(ctx, yd, ys, yi, din + b0 * rb, rb, kmax, Bc, R, part + b0 * per));
                    hipLaunchKernelGGL((k_wdl_stage<T>), dim3(ntiles, Bc), dim3(kClsThreads), 0, st, Wd + (ptrdiff_t)b0 * wsd, wsd, (uint32_t)m, ldm,
                                       din + b0 * rb, rb, kmax, (const T*)R, Wb, part + b0 * per);
                    if (total != 0u)
                        hipLaunchKernelGGL((k_wdl_atoms<T>), dim3(Su, ntiles), dim3(kClsThreads), 0, st, ldm, (const uint32_t*)off, (const uint32_t*)sb,
                                           (const T*)sw, (const T*)R, (const T*)Wb, (uint32_t)b0, (uint32_t)b0 + Bc, b0 == 0 ? 1 : 0, Num, Den);
                    HIPCHK(hipGetLastError());
                }
            }
            if (objective) HIPCHK(dl_launch_objective(ctx, part, per, Bu, sig, obj));
            // ---- d, nu, changed / left, V: straight into a device V, else in place over num ([S][ldm]) ----
            T* out = v_dev ? Vout : Num;
            const long long ors = v_dev ? (long long)rs : 1ll, ocs = v_dev ? (long long)cs : (long long)ldm;
            hipLaunchKernelGGL((k_wdl_finish<T>), dim3(Su), dim3(256), 0, st, At, ldm, (uint32_t)m, (const uint32_t*)dcols, (const uint32_t*)off, Num,
                               (const T*)Den, ntiles, out, ors, ocs, dusage, nu);
            HIPCHK(hipGetLastError());
            if (dout) {
                hipLaunchKernelGGL((k_wdl_scale<T>), dim3(Bu), dim3(256), 0, st, din, dout, rb, kmax, (const uint32_t*)slot_of, (const T*)nu);
                HIPCHK(hipGetLastError());
                if (!out_dev) HIPCHK(hipMemcpyAsync(records_out, stage, B * rb, hipMemcpyDeviceToHost, st));
            }
            if (objective) HIPCHK(hipMemcpyAsync(objective, obj, sizeof(double), hipMemcpyDefault, st));
            if (usage) HIPCHK(hipMemcpyAsync(usage, dusage, S * sizeof(uint32_t), hipMemcpyDefault, st));
            std::vector<uint32_t> hus;
            if (apply) {
                hus.resize(S);
                HIPCHK(hipMemcpyAsync(hus.data(), dusage, S * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            }
            if (Vout && !v_dev) {
                tmp.resize(S * m);
                HIPCHK(hipMemcpy2DAsync(tmp.data(), m * sizeof(T), Num, (size_t)ldm * sizeof(T), m * sizeof(T), S, hipMemcpyDeviceToHost, st));
                HIPCHK(hipStreamSynchronize(st));
                for (size_t s = 0; s < S; ++s)
                    for (size_t i = 0; i < m; ++i) Vout[(ptrdiff_t)i * rs + (ptrdiff_t)s * cs] = tmp[s * m + i];
            }
            HIPCHK(hipStreamSynchronize(st));
            if (!apply) return;
            // ---- apply: the changed atoms as a device column list + a contiguous device V, through the column replacement ----
            std::vector<uint32_t> pos, ccols;
            for (size_t s = 0; s < S; ++s)
                if (hus[s] != 0u && (hus[s] & kWdlLeft) == 0u) { pos.push_back((uint32_t)s); ccols.push_back(cols ? hc[s] : (uint32_t)s); }
            if (pos.empty()) return;
            const size_t nc = pos.size();
            grow(ds->vc, ds->vc_bytes, nc * m * sizeof(T), "hipMalloc(weighted atom update: changed atoms)");
            T* Vc = reinterpret_cast<T*>(ds->vc);
            HIPCHK(hipMemcpyAsync(sel, pos.data(), nc * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(sel + S, ccols.data(), nc * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            HIPCHK(dl_launch_gather<T>(ctx, (const T*)out, ors, ocs, (const uint32_t*)sel, (uint32_t)nc, Vc));
            HIPCHK(hipStreamSynchronize(st));
            rc = replace_columns_device<T>(ctx, sel + S, ccols, Vc, 1ll, (long long)m, err, errlen);
        });
    });
    return rc;
}

template <typename T>
int wdl_entry(ss_hip_ctx* ctx, const T* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const T* W, ptrdiff_t w_stride, const void* records,
              uint32_t kmax, void* records_out, const uint32_t* cols, size_t S, T* V, ptrdiff_t rs, ptrdiff_t cs, uint32_t* usage,
              double* objective, uint32_t flags, char* err, size_t errlen)
{
    static const char* who = "weighted_atom_update";
    int rc = check_common<T>(ctx, who, records, true, kmax, err, errlen);
    if (rc != SS_HIP_OK) return rc;
    if (!Y) { set_err(err, errlen, "weighted_atom_update: Y must not be null"); return SS_HIP_EINVAL; }
    if ((rc = weights_check_args(ctx, who, W, w_stride, err, errlen)) != SS_HIP_OK) return rc;
    if (flags & ~(uint32_t)SS_HIP_WDL_APPLY) { set_err(err, errlen, "weighted_atom_update: unknown flag bit"); return SS_HIP_EINVAL; }
    if (!V && !(flags & SS_HIP_WDL_APPLY) && !usage && !objective && !records_out) {
        set_err(err, errlen, "weighted_atom_update: nothing asked for (V, usage, objective and records_out are null and the atoms are not applied)");
        return SS_HIP_EINVAL;
    }
    if (reinterpret_cast<uintptr_t>(records_out) & 7u) { set_err(err, errlen, "weighted_atom_update: records_out must be 8-byte aligned"); return SS_HIP_EINVAL; }
    if (incy <= 0 || y_stride <= 0 || (V && (rs <= 0 || cs <= 0))) { set_err(err, errlen, "weighted_atom_update: increments and strides must be positive"); return SS_HIP_EINVAL; }
    if (B >= 0x80000000ull || (unsigned long long)B * kmax >= 0xffffffffull) { set_err(err, errlen, "weighted_atom_update: B * kmax must stay below 2^32"); return SS_HIP_EINVAL; }
    if (records_out && records_out != records) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(records), b = reinterpret_cast<uintptr_t>(records_out);
        const size_t bytes = B * record_bytes(kmax, sizeof(T));
        if (a < b + bytes && b < a + bytes) { set_err(err, errlen, "weighted_atom_update: records and records_out overlap in part"); return SS_HIP_EINVAL; }
    }
    if (B == 0 || (cols && S == 0)) return SS_HIP_OK;         // (every argument above was checked all the same)
    if (cols && S > ctx->n) { set_err(err, errlen, "weighted_atom_update: more columns than the dictionary has (a column is named twice)"); return SS_HIP_EINVAL; }
    return guarded(err, errlen, who, [&] {
        return wdl_impl<T>(ctx, Y, B, y_stride, incy, W, w_stride, records, kmax, records_out, cols, S, V, rs, cs, usage, objective,
                           (flags & SS_HIP_WDL_APPLY) != 0u, err, errlen);
    });
}

}  // namespace

void wdictlearn_free(ss_hip_ctx* ctx)
{
    WdlState* ds = static_cast<WdlState*>(ctx->wdl);
    if (!ds) return;
    if (ds->index) (void)hipFree(ds->index);
    if (ds->work) (void)hipFree(ds->work);
    if (ds->vc) (void)hipFree(ds->vc);
    delete ds;
    ctx->wdl = nullptr;
}

}  // namespace sship

using namespace sship;

extern "C" {

int ss_hip_weighted_atom_update_f32(ss_hip_ctx* ctx, const float* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const float* W,
                                    ptrdiff_t w_stride, const void* records, uint32_t kmax, void* records_out, const uint32_t* cols, size_t S,
                                    float* V, ptrdiff_t stride_row, ptrdiff_t stride_col, uint32_t* usage, double* objective, uint32_t flags,
                                    char* err, size_t errlen)
{
    return wdl_entry<float>(ctx, Y, B, y_stride, incy, W, w_stride, records, kmax, records_out, cols, S, V, stride_row, stride_col, usage, objective,
                            flags, err, errlen);
}
int ss_hip_weighted_atom_update_f64(ss_hip_ctx* ctx, const double* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const double* W,
                                    ptrdiff_t w_stride, const void* records, uint32_t kmax, void* records_out, const uint32_t* cols, size_t S,
                                    double* V, ptrdiff_t stride_row, ptrdiff_t stride_col, uint32_t* usage, double* objective, uint32_t flags,
                                    char* err, size_t errlen)
{
    return wdl_entry<double>(ctx, Y, B, y_stride, incy, W, w_stride, records, kmax, records_out, cols, S, V, stride_row, stride_col, usage, objective,
                             flags, err, errlen);
}

}  // extern "C"
