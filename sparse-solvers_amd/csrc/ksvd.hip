// ksvd.hip — the sequential atom and coefficient sweep of approximate K-SVD on the device, from compact records (include/ss_hip.h):
//   ss_hip_homotopy_ksvd_sweep_*.
//
// The working residuals start as r_b = y_b - A x_b (dictlearn.hip's k_dl_residual, all B signals in one block).  Then, one requested
// atom after the other (s = 0 .. S - 1, j = cols[s]), with U_j the counting signals (K_b <= kmax) whose record holds j in ascending b
// and w_b the INPUT record's value for j:
//   g   = (sum w_b^2) a_j + sum_{b in U_j} w_b r_b,      v = g / ||g||_2          (dictlearn.hip's atom, with the CURRENT residuals)
//   rho = a_j . v,     t_b = r_b . v,     w'_b = t_b + w_b rho                    (row b of E_j^T v,  E_j = R_U + a_j w^T)
//   r_b <- (r_b + w_b a_j) - w'_b v,      the output record's value for j <- w'_b
// and the atom is left as it is (no record value, no residual touched) when U_j is empty or ||g||_2 is zero or not finite.
// v is the direction of the minimiser E w / ||w||^2 over the atom for fixed w, w' = E^T v the minimiser over the coefficients for the
// unit v: ||E - v w'^T||_F <= ||E - a w^T||_F whatever the norm of a, so no atom step raises sum ||r_b||^2 in exact arithmetic.
//
// An atom's step touches only the rows and record values of its own users, so atoms that share no signal commute exactly.  The host
// computes the level schedule from the inverted index (ks_levels.h) and the atoms run by (level, s): every level in parallel over its
// atoms, three launches a level, back to back on the context's stream, no host synchronisation between levels.
//
//   learn_*          the host steps the three learners share (learn_driver.h): checks, the atom list, the arena, the index, the copies
//                    out and apply.  dl_launch_*: the inverted index, the initial residuals, the objective's sums: dictlearn.hip's words
//   k_ks_g           phase 1, grid = (atom of the level, row tile of 1024).  The accumulator starts from (sum w^2) a_j and takes
//                    w_b * R[b] of the atom's users in list order, eight rows in flight, writes g and the tile's sum of squares.
//   k_ks_norm        phase 2, one workgroup per atom of the level: ||g||_2 from the partials, the verdict, usage, v (or the stored
//                    column) in place over g ([S][ldm], rows m .. ldm - 1 zero), the partials of rho and rho.
//   k_ks_pairs       phase 3, one workgroup per (atom, user) pair of the level: t_b over the row (first pass), w'_b, the residual
//                    update (second pass over the row: an L2 hit), the store of w'_b into the output record.
//   k_ks_resnorm     grid = (signal, row tile): the tile's sums of squares of the final residuals, for the objective after.
//   k_ks_vout        V through a device caller's strides.
//
// SUMMATION ORDER (the tests' bounds follow from it; build flag -ffp-contract=off: products and sums are rounded separately):
//   r_b, sum w^2, the objective   dictlearn.hip's words (r_b,i = y_b,i - acc_i; sum w^2 in double, ascending b, rounded once to T);
//   g_i        starts at (sum w^2) * a_ij and takes w_b * r_b,i one user after the other in ascending b, in the context's
//              precision — one chain per element, never split;
//   ||g||^2, ||r_b||^2, rho, t_b   in double, classify.hip's order: a thread adds its four terms (squares, or products of the two
//              operands widened to double) in ascending row order, a wave its 64 thread sums by the butterfly lane ^ 32, ^ 16, ^ 8,
//              ^ 4, ^ 2, ^ 1, then the wave sums one after the other: tiles ascending, inside a tile waves 0, 1, 2, 3 — a function of
//              m alone.  rho and t_b take rows 0 .. m - 1 only;
//   v_i        = g_i / (T) sqrt(||g||^2);
//   w'_b       = (T)(t_b + (double) w_b * rho), the product and the sum in double;
//   r_b,i      = (r_b,i + w_b * a_ij) - w'_b * v_i, each product and sum rounded in the context's precision, a_ij the STORED column;
//   objective[0], objective[1] = the ||r_b||^2 of the initial / final residuals one after the other in ascending b (truncated: +0).
// No floating-point atomics.  The outputs are a function of (records, Y, A, cols as an ordered list) alone: the same words with or
// without SS_HIP_KSVD_SERIAL, with host or device pointers, in place or out of place, whatever the context did before.
// RANGE: dictlearn.hip's — under A 2^a, Y 2^b, record values 2^(b-a) the atoms and usage are the same words, the output values those
// of the unscaled call times 2^b (the coefficients of unit atoms), the objectives times 2^2b, as long as sum w^2 (2^(2b-2a)),
// (sum w^2) a_ij and w_b r_b,i (2^(2b-a)) are normal numbers of the context's precision and ||g||^2 (2^(4b-2a)) of double.
#include "ss_hip_internal.h"
#include "learn_driver.h"
#include "ks_levels.h"

#include <algorithm>
#include <cmath>
#include <limits>

namespace sship {

namespace {

constexpr uint32_t kKsResidualRows = 32768;              // most signals per launch of the residual kernel (its grid.y)

// ---- kernels -------------------------------------------------------------------------------------------------------------------

// phase 1: atom s = order[blockIdx.x], row tile blockIdx.y.  k_dl_atoms' chain over the whole list, from the working residuals
template <typename T>
__global__ __launch_bounds__(256)
void k_ks_g(const T* __restrict__ At, uint32_t ldm, const uint32_t* __restrict__ cols, const uint32_t* __restrict__ order,
            const uint32_t* __restrict__ off, const uint32_t* __restrict__ sb, const T* __restrict__ sw, const T* __restrict__ s2,
            const T* __restrict__ R, T* __restrict__ G, double* __restrict__ partg)
{
    typedef typename ClsVec<T>::type V;
    constexpr uint32_t W = ClsVec<T>::W, L = ClsVec<T>::L, U = kClsInFlight;
    const uint32_t s = order[blockIdx.x], tile = blockIdx.y, ntiles = gridDim.y;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t beg = off[s], end = off[s + 1u];
    if (beg == end) return;                             // no user: k_ks_norm hands the stored column back
    uint32_t row0[L];
#pragma unroll
    for (uint32_t j = 0; j < L; ++j) row0[j] = tile * kClsTileRows + j * (256u * W) + tid * W;
    T acc[L][W];
    {
        const T q = s2[s];
        const T* colp = At + (size_t)(cols ? cols[s] : s) * ldm;
#pragma unroll
        for (uint32_t j = 0; j < L; ++j) {
            const V a = row0[j] < ldm ? *reinterpret_cast<const V*>(colp + row0[j]) : V{};
#pragma unroll
            for (uint32_t e = 0; e < W; ++e) acc[j][e] = q * vget(a, e);
        }
    }
    uint32_t k = beg;
    for (; k + U <= end; k += U) {                      // U users' rows in flight, added in order
        V a[U][L];
        T w[U];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            const T* rowp = R + (size_t)sb[k + u] * ldm;
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
    for (; k < end; ++k) {
        const T* rowp = R + (size_t)sb[k] * ldm;
        const T w = sw[k];
#pragma unroll
        for (uint32_t j = 0; j < L; ++j) {
            const V a = row0[j] < ldm ? *reinterpret_cast<const V*>(rowp + row0[j]) : V{};
#pragma unroll
            for (uint32_t e = 0; e < W; ++e) acc[j][e] = acc[j][e] + w * vget(a, e);
        }
    }
    T* g = G + (size_t)s * ldm;
    double q = 0.0;
#pragma unroll
    for (uint32_t j = 0; j < L; ++j) {
#pragma unroll
        for (uint32_t e = 0; e < W; ++e) q += (double)acc[j][e] * (double)acc[j][e];
        if (row0[j] < ldm) *reinterpret_cast<V*>(g + row0[j]) = cls_pack<T>(acc[j]);
    }
    q = wave_sum(q);
    if (lane == 0u) partg[((size_t)s * ntiles + tile) * 4u + wave] = q;
}

// phase 2: atom s = order[blockIdx.x].  G[s] becomes v = g / ||g|| or the stored column (rows m .. ldm - 1: zero); rho[s] = a . v
template <typename T>
__global__ __launch_bounds__(256)
void k_ks_norm(const T* __restrict__ At, uint32_t ldm, uint32_t m, const uint32_t* __restrict__ cols, const uint32_t* __restrict__ order,
               const uint32_t* __restrict__ off, T* G, const double* __restrict__ partg, uint32_t ntiles, double* rho_part,
               double* __restrict__ rho, uint32_t* __restrict__ usage, uint32_t* __restrict__ verdict)
{
    typedef typename ClsVec<T>::type V;
    constexpr uint32_t W = ClsVec<T>::W, L = ClsVec<T>::L;
    __shared__ T s_norm;
    __shared__ uint32_t s_ok;
    const uint32_t s = order[blockIdx.x], tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
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
        verdict[s] = ok;
    }
    __syncthreads();
    const T nrm = s_norm;
    const bool ok = s_ok != 0u;
    T* g = G + (size_t)s * ldm;
    const T* colp = At + (size_t)(cols ? cols[s] : s) * ldm;
    double* rp = rho_part + (size_t)s * ntiles * 4u;
    for (uint32_t tile = 0; tile < ntiles; ++tile) {
        double q = 0.0;
#pragma unroll
        for (uint32_t j = 0; j < L; ++j) {
            const uint32_t row0 = tile * kClsTileRows + j * (256u * W) + tid * W;
            if (row0 >= ldm) continue;
            const V a = *reinterpret_cast<const V*>(colp + row0);
            V gv = V{};
            if (ok) gv = *reinterpret_cast<const V*>(g + row0);
            T d[W];
#pragma unroll
            for (uint32_t e = 0; e < W; ++e) {
                d[e] = row0 + e < m ? (ok ? vget(gv, e) / nrm : vget(a, e)) : T(0);
                if (row0 + e < m) q += (double)vget(a, e) * (double)d[e];
            }
            *reinterpret_cast<V*>(g + row0) = cls_pack<T>(d);
        }
        q = wave_sum(q);
        if (lane == 0u) rp[tile * 4u + wave] = q;
    }
    __threadfence_block();
    __syncthreads();
    if (tid == 0) {
        double q = 0.0;
        for (uint32_t t = 0; t < ntiles * 4u; ++t) q += rp[t];
        rho[s] = q;
    }
}

// phase 3: pair blockIdx.x of the level = (atom pair_s, list position pair_p).  The atoms of a level share no signal and a list names
// a signal once, so no two workgroups of a launch touch the same row or the same record
template <typename T>
__global__ __launch_bounds__(256)
void k_ks_pairs(const T* __restrict__ At, uint32_t ldm, uint32_t m, const uint32_t* __restrict__ cols, const uint32_t* __restrict__ pair_s,
                const uint32_t* __restrict__ pair_p, const uint32_t* __restrict__ sb, const T* __restrict__ sw, const T* __restrict__ Vw,
                const double* __restrict__ rho, const uint32_t* __restrict__ verdict, T* R, unsigned char* rec_out, size_t rb, uint32_t kmax,
                uint32_t ntiles)
{
    typedef typename ClsVec<T>::type V;
    constexpr uint32_t W = ClsVec<T>::W, L = ClsVec<T>::L;
    __shared__ double s_wave[4];
    __shared__ T s_new;
    const uint32_t s = pair_s[blockIdx.x];
    if (verdict[s] == 0u) return;                       // the atom is left as it is
    const uint32_t p = pair_p[blockIdx.x], b = sb[p], col = cols ? cols[s] : s;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const T w = sw[p];
    const T* v = Vw + (size_t)s * ldm;
    const T* colp = At + (size_t)col * ldm;
    T* r = R + (size_t)b * ldm;
    double t = 0.0;
    for (uint32_t tile = 0; tile < ntiles; ++tile) {
        double q = 0.0;
#pragma unroll
        for (uint32_t j = 0; j < L; ++j) {
            const uint32_t row0 = tile * kClsTileRows + j * (256u * W) + tid * W;
            if (row0 >= ldm) continue;
            const V rv = *reinterpret_cast<const V*>(r + row0);
            const V vv = *reinterpret_cast<const V*>(v + row0);
#pragma unroll
            for (uint32_t e = 0; e < W; ++e)
                if (row0 + e < m) q += (double)vget(rv, e) * (double)vget(vv, e);
        }
        q = wave_sum(q);
        if (lane == 0u) s_wave[wave] = q;
        __syncthreads();
        if (tid == 0) { t += s_wave[0]; t += s_wave[1]; t += s_wave[2]; t += s_wave[3]; }
        __syncthreads();
    }
    if (tid == 0) s_new = (T)(t + (double)w * rho[s]);
    __syncthreads();
    const T wn = s_new;
    for (uint32_t tile = 0; tile < ntiles; ++tile) {
#pragma unroll
        for (uint32_t j = 0; j < L; ++j) {
            const uint32_t row0 = tile * kClsTileRows + j * (256u * W) + tid * W;
            if (row0 >= ldm) continue;
            const V rv = *reinterpret_cast<const V*>(r + row0);
            const V vv = *reinterpret_cast<const V*>(v + row0);
            const V av = *reinterpret_cast<const V*>(colp + row0);
            T d[W];
#pragma unroll
            for (uint32_t e = 0; e < W; ++e) d[e] = row0 + e < m ? (vget(rv, e) + w * vget(av, e)) - wn * vget(vv, e) : T(0);
            *reinterpret_cast<V*>(r + row0) = cls_pack<T>(d);
        }
    }
    unsigned char* ro = rec_out + (size_t)b * rb;
    const uint32_t K = *reinterpret_cast<const uint32_t*>(ro);           // (a user's record counts: K <= kmax)
    const uint32_t* idx = reinterpret_cast<const uint32_t*>(ro + 16);
    unsigned char* valp = ro + 16 + (size_t)kmax * 4;
    for (uint32_t e = tid; e < K && e < kmax; e += 256u)
        if (idx[e] == col) store_val(valp, e, wn);
}

// part[b][tile][wave] = the tile's sums of squares of R[b] (0 for a truncated record, whose row was never written)
template <typename T>
__global__ __launch_bounds__(256)
void k_ks_resnorm(const T* __restrict__ R, uint32_t ldm, const unsigned char* __restrict__ rec, size_t rb, uint32_t kmax,
                  double* __restrict__ part)
{
    typedef typename ClsVec<T>::type V;
    constexpr uint32_t W = ClsVec<T>::W, L = ClsVec<T>::L;
    const uint32_t b = blockIdx.x, tile = blockIdx.y, ntiles = gridDim.y;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t K = *reinterpret_cast<const uint32_t*>(rec + (size_t)b * rb);
    double q = 0.0;
    if (K <= kmax) {
#pragma unroll
        for (uint32_t j = 0; j < L; ++j) {
            const uint32_t row0 = tile * kClsTileRows + j * (256u * W) + tid * W;
            const V rv = row0 < ldm ? *reinterpret_cast<const V*>(R + (size_t)b * ldm + row0) : V{};
#pragma unroll
            for (uint32_t e = 0; e < W; ++e) q += (double)vget(rv, e) * (double)vget(rv, e);
        }
        q = wave_sum(q);
    }
    if (lane == 0u) part[((size_t)b * ntiles + tile) * 4u + wave] = q;
}

// out(i, s) = out[i * ors + s * ocs] = Vw[s][i]
template <typename T>
__global__ __launch_bounds__(256)
void k_ks_vout(const T* __restrict__ Vw, uint32_t ldm, uint32_t m, T* __restrict__ out, long long ors, long long ocs)
{
    const uint32_t s = blockIdx.x;
    for (uint32_t i = threadIdx.x; i < m; i += 256u) out[(long long)i * ors + (long long)s * ocs] = Vw[(size_t)s * ldm + i];
}

// ---- host side -----------------------------------------------------------------------------------------------------------------

// the index and the workspace: the common pieces (learn_driver.h), and the partials of ||g||^2 and rho, rho, the verdicts, the atoms
// by (level, s); g / v and the residual block of ALL signals (an atom needs all its users at once)
template <typename T> struct KsIndex : LearnIndex<T> {
    double *partg, *rho_part, *rho;
    uint32_t *verdict, *order;
    void carve(Carver& cv, const LearnCall<T>& c)
    {
        this->head(cv, c, 2);
        partg = cv.take<double>(c.S * c.per);
        rho_part = cv.take<double>(c.S * c.per);
        rho = cv.take<double>(c.S);
        this->dusage = cv.take<uint32_t>(c.S);
        verdict = cv.take<uint32_t>(c.S);
        order = cv.take<uint32_t>(c.S);
        this->sel = cv.take<uint32_t>(2 * c.S);          // apply: positions of the changed atoms, then their columns
    }
};

// (pair_b / pair_e: scratch of the index; then the schedule: the pairs' atoms and their list positions, by (level, s, b))
template <typename T> struct KsWork : LearnWork<T> {
    T *G, *R;
    void carve(Carver& cv, const LearnCall<T>& c)
    {
        this->lists(cv, c);
        G = cv.take<T>(c.S * c.ldm);
        R = cv.take<T>(c.B * c.ldm);
        this->signals(cv, c, c.B);
    }
};

template <typename T>
int ksvd_impl(LearnCall<T>& c, bool serial)
{
    ss_hip_ctx* ctx = c.ctx;
    int rc = learn_atoms(c);
    if (rc != SS_HIP_OK) return rc;
    hipStream_t st = ctx->stream;
    const size_t B = c.B, S = c.S, m = c.m, rb = c.rb;
    const uint32_t Su = (uint32_t)S, Bu = (uint32_t)B, ldm = c.ldm, ntiles = c.ntiles, per = c.per;
    const T* At = static_cast<const T*>(ctx->At);

    KsIndex<T> ix;
    learn_carve(learn_arena(ctx).index, ix, c, "hipMalloc(atom learning index)");
    if ((rc = learn_open(c, ix)) != SS_HIP_OK) return rc;
    const uint32_t total = c.total;

    KsWork<T> wk;
    const size_t need = learn_bytes(wk, c);
    try {
        learn_carve(learn_arena(ctx).work, wk, c, "hipMalloc(atom learning workspace)");
    } catch (const HipFail& f) {
        if (f.code != hipErrorOutOfMemory) throw;
        (void)hipGetLastError();
        set_err(c.err, c.errlen, std::string(c.who) + ": no device memory for a workspace of " + std::to_string(need) + " bytes (the residual block of all " +
                                     std::to_string(B) + " signals, " + std::to_string(B * (size_t)ldm * sizeof(T)) + " bytes, must be resident)");
        return SS_HIP_ENOMEM;
    }

    // ---- the lists; the schedule on the host from their offsets and signals ----
    std::vector<uint32_t> hoff(S + 1, 0u), hsb(total);
    if (total != 0u) {
        HIPCHK(dl_launch_lists<T>(ctx, c.place.din, rb, c.kmax, Bu, ix.slot_of, ix.dcols, Su, ix.counts, ix.off, c.longest, wk.pair_b, wk.pair_e, wk.sb,
                                  wk.sw, ix.s2, ix.bad));
        HIPCHK(hipMemcpyAsync(hoff.data(), ix.off, (S + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(hsb.data(), wk.sb, (size_t)total * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (uint32_t p = 0; p < total; ++p)
            if (hsb[p] >= Bu) { set_err(c.err, c.errlen, "ksvd_sweep: internal error (a list names a signal >= B)"); return SS_HIP_ERUNTIME; }
        const size_t dup = ks_first_duplicate(hoff.data(), hsb.data(), S);
        if (dup != S) {
            set_err(c.err, c.errlen, std::string(c.who) + ": column " + std::to_string(c.cols ? c.hc[dup] : (uint32_t)dup) + " is listed twice in one record");
            return SS_HIP_EINVAL;
        }
    }
    std::vector<uint32_t> level, horder, first;
    const uint32_t nlevels = ks_levels(hoff.data(), hsb.data(), S, B, serial, level);
    ks_order(level, nlevels, horder, first);
    std::vector<uint32_t> hps(total), hpp(total), pfirst((size_t)nlevels + 1u, 0u);
    {
        uint32_t q = 0;
        for (uint32_t l = 0; l < nlevels; ++l) {
            pfirst[l] = q;
            for (uint32_t i = first[l]; i < first[l + 1u]; ++i) {
                const uint32_t s = horder[i];
                for (uint32_t p = hoff[s]; p < hoff[s + 1u]; ++p) { hps[q] = s; hpp[q] = p; ++q; }
            }
        }
        pfirst[nlevels] = q;
    }
    HIPCHK(hipMemcpyAsync(ix.order, horder.data(), S * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    if (total != 0u) {
        HIPCHK(hipMemcpyAsync(wk.pair_b, hps.data(), (size_t)total * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(wk.pair_e, hpp.data(), (size_t)total * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    }

    // ---- the initial residuals and the objective before; from here on outputs are written ----
    std::vector<T> tmp;
    const T* yd = c.Y;
    long long ysd = c.y_stride, yid = c.incy;
    if (!c.y_dev) { upload_rows<T>(ctx, wk.ybuf, c.Y, c.y_stride, c.incy, 0, B, tmp); yd = wk.ybuf; ysd = (long long)m; yid = 1; }
    for (size_t b0 = 0; b0 < B; b0 += kKsResidualRows) {
        const uint32_t Bc = (uint32_t)std::min<size_t>(kKsResidualRows, B - b0);
        HIPCHK(dl_launch_residuals<T>(ctx, yd + (ptrdiff_t)b0 * ysd, ysd, yid, c.place.din + b0 * rb, rb, c.kmax, Bc, wk.R + b0 * ldm, ix.part + b0 * per));
    }
    if (c.objective) HIPCHK(dl_launch_objective(ctx, ix.part, per, Bu, ix.sig, ix.obj));
    if (c.place.dout != c.place.din) HIPCHK(hipMemcpyAsync(c.place.dout, c.place.din, B * rb, hipMemcpyDeviceToDevice, st));

    // ---- the levels: three launches each, back to back ----
    for (uint32_t l = 0; l < nlevels; ++l) {
        const uint32_t na = first[l + 1u] - first[l], np = pfirst[l + 1u] - pfirst[l];
        if (na == 0u) continue;
        if (np != 0u)
            hipLaunchKernelGGL((k_ks_g<T>), dim3(na, ntiles), dim3(kClsThreads), 0, st, At, ldm, (const uint32_t*)ix.dcols,
                               (const uint32_t*)(ix.order + first[l]), (const uint32_t*)ix.off, (const uint32_t*)wk.sb, (const T*)wk.sw, (const T*)ix.s2,
                               (const T*)wk.R, wk.G, ix.partg);
        hipLaunchKernelGGL((k_ks_norm<T>), dim3(na), dim3(kClsThreads), 0, st, At, ldm, (uint32_t)m, (const uint32_t*)ix.dcols,
                           (const uint32_t*)(ix.order + first[l]), (const uint32_t*)ix.off, wk.G, (const double*)ix.partg, ntiles, ix.rho_part, ix.rho,
                           ix.dusage, ix.verdict);
        if (np != 0u)
            hipLaunchKernelGGL((k_ks_pairs<T>), dim3(np), dim3(kClsThreads), 0, st, At, ldm, (uint32_t)m, (const uint32_t*)ix.dcols,
                               (const uint32_t*)(wk.pair_b + pfirst[l]), (const uint32_t*)(wk.pair_e + pfirst[l]), (const uint32_t*)wk.sb, (const T*)wk.sw,
                               (const T*)wk.G, (const double*)ix.rho, (const uint32_t*)ix.verdict, wk.R, c.place.dout, rb, c.kmax, ntiles);
        HIPCHK(hipGetLastError());
    }

    // ---- the objective after, V in a device caller's strides; the copies out and apply from v in place over g ([S][ldm]) ----
    if (c.objective) {
        hipLaunchKernelGGL((k_ks_resnorm<T>), dim3(Bu, ntiles), dim3(kClsThreads), 0, st, (const T*)wk.R, ldm, c.place.din, rb, c.kmax, ix.part);
        HIPCHK(hipGetLastError());
        HIPCHK(dl_launch_objective(ctx, ix.part, per, Bu, ix.sig, ix.obj + 1));
    }
    if (c.v_dev) {
        hipLaunchKernelGGL((k_ks_vout<T>), dim3(Su), dim3(256), 0, st, (const T*)wk.G, ldm, (uint32_t)m, c.V, (long long)c.rs, (long long)c.cs);
        HIPCHK(hipGetLastError());
    }
    return learn_finish<T>(c, ix, 2, wk.G, LearnOut<T>{ wk.G, 1ll, (long long)ldm });
}

template <typename T>
int ksvd_entry(ss_hip_ctx* ctx, const T* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const void* records, uint32_t kmax, void* records_out,
               const uint32_t* cols, size_t S, T* V, ptrdiff_t rs, ptrdiff_t cs, uint32_t* usage, double* objective, uint32_t flags, char* err,
               size_t errlen)
{
    const bool apply = (flags & SS_HIP_KSVD_APPLY) != 0u;
    LearnCall<T> c{ ctx, "ksvd_sweep", Y, B, y_stride, incy, records, kmax, records_out, cols, S, V, rs, cs, usage, objective, apply, err, errlen };
    LearnRules r{};
    r.null_y = "Y and records_out must not be null";
    if (!records_out) r.own = r.null_y;
    r.flags = flags;
    r.mask = SS_HIP_KSVD_APPLY | SS_HIP_KSVD_SERIAL;
    if (!V && !apply && !usage && !objective) r.nothing = "nothing asked for (V, usage and objective are null and the atoms are not applied)";
    bool empty = false;
    const int rc = learn_check_args(c, r, empty);
    if (rc != SS_HIP_OK || empty) return rc;
    return guarded(err, errlen, c.who, [&] { return ksvd_impl<T>(c, (flags & SS_HIP_KSVD_SERIAL) != 0u); });
}

}  // namespace

}  // namespace sship

using namespace sship;

extern "C" {

int ss_hip_homotopy_ksvd_sweep_f32(ss_hip_ctx* ctx, const float* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const void* records,
                                   uint32_t kmax, void* records_out, const uint32_t* cols, size_t S, float* V, ptrdiff_t stride_row,
                                   ptrdiff_t stride_col, uint32_t* usage, double* objective, uint32_t flags, char* err, size_t errlen)
{
    return ksvd_entry<float>(ctx, Y, B, y_stride, incy, records, kmax, records_out, cols, S, V, stride_row, stride_col, usage, objective, flags, err, errlen);
}
int ss_hip_homotopy_ksvd_sweep_f64(ss_hip_ctx* ctx, const double* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const void* records,
                                   uint32_t kmax, void* records_out, const uint32_t* cols, size_t S, double* V, ptrdiff_t stride_row,
                                   ptrdiff_t stride_col, uint32_t* usage, double* objective, uint32_t flags, char* err, size_t errlen)
{
    return ksvd_entry<double>(ctx, Y, B, y_stride, incy, records, kmax, records_out, cols, S, V, stride_row, stride_col, usage, objective, flags, err, errlen);
}

}  // extern "C"
