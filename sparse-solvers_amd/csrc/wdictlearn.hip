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
//   learn_*          the host steps the three learners share (learn_driver.h): checks, the atom list, the arena, the index, the chunk
//                    size, the copies out and apply.  dl_launch_*: the lists, the residual block, the objective's sums: dictlearn.hip's
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
#include "learn_driver.h"

#include <algorithm>
#include <cmath>
#include <limits>

namespace sship {

namespace {

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
        *reinterpret_cast<V*>(Wb + (size_t)b * ldm + row0) = cls_pack<T>(wv);
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
    const uint32_t lo = dl_lower_bound(sb, beg, end, b0), hi = dl_lower_bound(sb, lo, end, b1);
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
            *reinterpret_cast<V*>(nump + row0[j]) = cls_pack<T>(num[j]);
            *reinterpret_cast<V*>(denp + row0[j]) = cls_pack<T>(den[j]);
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
                *reinterpret_cast<V*>(d + row0) = cls_pack<T>(dk);
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
        usage[s] = cnt != 0u && ok == 0u ? (cnt | kDlLeft) : cnt;
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
        if (s == kDlNone) continue;
        const T f = nu[s];
        if (f != T(0)) store_val(vout, e, load_val(vin, e, T(0)) * f);
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------

// the index and the workspace: the common pieces (learn_driver.h; the index's sum c^2 is not used here), and nu per slot; num and
// den, the residual and weight blocks of a chunk
template <typename T> struct WdlIndex : LearnIndex<T> {
    T* nu;
    void carve(Carver& cv, const LearnCall<T>& c)
    {
        this->head(cv, c, 1);
        nu = cv.take<T>(c.S);
        this->tail(cv, c);
    }
};

template <typename T> struct WdlWork : LearnWork<T> {
    size_t chunk;
    T *Num, *Den, *R, *Wb;
    void carve(Carver& cv, const LearnCall<T>& c)
    {
        this->lists(cv, c);
        Num = cv.take<T>(c.S * c.ldm);
        Den = cv.take<T>(c.S * c.ldm);
        R = cv.take<T>(chunk * c.ldm);
        Wb = cv.take<T>(chunk * c.ldm);
        this->signals(cv, c, chunk);
    }
};

template <typename T>
int wdl_impl(LearnCall<T>& c, const T* W, ptrdiff_t w_stride)
{
    ss_hip_ctx* ctx = c.ctx;
    int rc = learn_atoms(c);
    if (rc != SS_HIP_OK) return rc;
    hipStream_t st = ctx->stream;
    const size_t B = c.B, m = c.m, rb = c.rb;
    const uint32_t Su = (uint32_t)c.S, Bu = (uint32_t)B, ldm = c.ldm, ntiles = c.ntiles, per = c.per;
    const T* At = static_cast<const T*>(ctx->At);

    WdlIndex<T> ix;
    learn_carve(learn_arena(ctx).index, ix, c, "hipMalloc(atom learning index)");
    if ((rc = learn_open(c, ix)) != SS_HIP_OK) return rc;

    // ---- the weights where the kernels read them, checked: the last thing that can fail before an output is written ----
    const T* Wd = nullptr;
    long long wsd = 0;
    if ((rc = weights_on_device<T>(ctx, c.who, W, B, w_stride, &Wd, &wsd, c.err, c.errlen)) != SS_HIP_OK) return rc;

    // ---- the lists, num and den, the residual and weight blocks of a chunk ----
    WdlWork<T> wk;
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
            hipLaunchKernelGGL((k_wdl_stage<T>), dim3(ntiles, Bc), dim3(kClsThreads), 0, st, Wd + (ptrdiff_t)b0 * wsd, wsd, (uint32_t)m, ldm,
                               c.place.din + b0 * rb, rb, c.kmax, (const T*)wk.R, wk.Wb, ix.part + b0 * per);
            if (c.total != 0u)
                hipLaunchKernelGGL((k_wdl_atoms<T>), dim3(Su, ntiles), dim3(kClsThreads), 0, st, ldm, (const uint32_t*)ix.off, (const uint32_t*)wk.sb,
                                   (const T*)wk.sw, (const T*)wk.R, (const T*)wk.Wb, (uint32_t)b0, (uint32_t)b0 + Bc, b0 == 0 ? 1 : 0, wk.Num, wk.Den);
            HIPCHK(hipGetLastError());
        }
    }
    if (c.objective) HIPCHK(dl_launch_objective(ctx, ix.part, per, Bu, ix.sig, ix.obj));
    // ---- d, nu, changed / left, V: straight into a device V, else in place over num ([S][ldm]); the records' values times nu ----
    const LearnOut<T> out = learn_out(c, wk.Num);
    hipLaunchKernelGGL((k_wdl_finish<T>), dim3(Su), dim3(256), 0, st, At, ldm, (uint32_t)m, (const uint32_t*)ix.dcols, (const uint32_t*)ix.off, wk.Num,
                       (const T*)wk.Den, ntiles, out.p, out.rs, out.cs, ix.dusage, ix.nu);
    HIPCHK(hipGetLastError());
    if (c.place.dout) {
        hipLaunchKernelGGL((k_wdl_scale<T>), dim3(Bu), dim3(256), 0, st, c.place.din, c.place.dout, rb, c.kmax, (const uint32_t*)ix.slot_of, (const T*)ix.nu);
        HIPCHK(hipGetLastError());
    }
    return learn_finish<T>(c, ix, 1, wk.Num, out);
}

template <typename T>
int wdl_entry(ss_hip_ctx* ctx, const T* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const T* W, ptrdiff_t w_stride, const void* records,
              uint32_t kmax, void* records_out, const uint32_t* cols, size_t S, T* V, ptrdiff_t rs, ptrdiff_t cs, uint32_t* usage,
              double* objective, uint32_t flags, char* err, size_t errlen)
{
    const bool apply = (flags & SS_HIP_WDL_APPLY) != 0u;
    LearnCall<T> c{ ctx, "weighted_atom_update", Y, B, y_stride, incy, records, kmax, records_out, cols, S, V, rs, cs, usage, objective, apply, err, errlen };
    LearnRules r{};
    r.null_y = "Y must not be null";
    r.flags = flags;
    r.mask = SS_HIP_WDL_APPLY;
    if (!V && !apply && !usage && !objective && !records_out)
        r.nothing = "nothing asked for (V, usage, objective and records_out are null and the atoms are not applied)";
    r.weighted = true;
    r.W = W;
    r.w_stride = w_stride;
    bool empty = false;
    const int rc = learn_check_args(c, r, empty);
    if (rc != SS_HIP_OK || empty) return rc;
    return guarded(err, errlen, c.who, [&] { return wdl_impl<T>(c, W, w_stride); });
}

}  // namespace

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
