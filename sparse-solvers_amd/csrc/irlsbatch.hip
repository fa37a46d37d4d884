// irlsbatch.hip — IRLS for BATCHES of signals against one factorised matrix (ss_hip_irls_solve_batch_*).
//
// Every step of the single solve (irls.hip) is independent per signal, so a batch runs the same statements in the same
// order per signal — slot-indexed sibling kernels of the single solve's, built like irls.hip with -ffp-contract=off — and
// returns, for every signal, the single solve's words bit for bit.  Two forms, the single solve's rule picks between them:
//
//   * one-workgroup form (n < kIrlsBlockedMin, the LDS limit, or SS_HIP_IRLS_FUSED): k_irlsb_solve is k_irls_solve with the
//     slot taken from blockIdx.x — one launch per chunk runs every Newton round of every signal;
//   * blocked lock-step form: the single solve's chain of launches (scale, Cholesky by panels of 32, blocked triangular
//     solves, t = Q s, Q^T t, tail), each launch covering every live slot of the chunk (blockIdx.y indexes the live list).
//     The products with Q take a group of kQGroup signals per thread (t = Q s) or per wave (Q^T v): each signal keeps its own
//     accumulator in the single kernel's order, Q is read once per group.  A slot that has finished leaves each kernel at its
//     first instruction, as the single kernels do with ctl->done; after every round k_irlsb_live compacts the live list on
//     the device and the host reads ONE word, the number of live slots.
//
// Per slot the workspace holds L (n^2), the vectors of the single solve (qTb, s, xnext, w, x: 5 x [n]; t, y: 2 x [ldm]),
// the loop state and the report.  Host side: irls_batch_impl in homotopy.hip (validation, chunks, copies, statistics).
#include "ss_hip_internal.h"
#include "ss_hip_device.h"

#include <algorithm>
#include <cstdlib>

namespace sship {

namespace {

constexpr int kIbThreads = 1024;                  // = kIrlsThreads of irls.hip
constexpr uint32_t kIbBlockedMin = 96;            // = kIrlsBlockedMin
constexpr uint32_t kIbB = 32;                     // = kChB: panel width / solve block
constexpr uint32_t kQGroup = 8;                   // signals per pass over Q in the two products with Q
constexpr size_t kIbBudget = (size_t)1 << 30;     // bytes of per-slot state a chunk may hold

template <typename T>
struct IbCtl {                                    // IrlsCtl<T> of irls.hip, one per slot
    T eps, abstol, second;
    uint32_t iter, done, spd_bad, pad_;
};

// block_max_excl of irls.hip
template <typename T>
__device__ __forceinline__ void ib_max_excl(const T* v, uint32_t n, uint32_t excl, T& mv, uint32_t& mi, T* sv, uint32_t* si)
{
    mv = -Lim<T>::max();
    mi = 0xffffffffu;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x)
        if (i != excl && better_max(v[i], i, mv, mi)) { mv = v[i]; mi = i; }
    block_reduce_pair<T, true>(mv, mi, sv, si);
    __syncthreads();
}

// ---- one-workgroup form: k_irls_solve's statements, one workgroup per slot --------------------------------------------
template <typename T>
__global__ __launch_bounds__(kIbThreads)
void k_irlsb_solve(const T* __restrict__ Qt, const T* __restrict__ R, const T* __restrict__ G0, T* __restrict__ Lall,
                   T* __restrict__ vecall, uint32_t ldm, uint32_t m, uint32_t n, size_t vstride, T tol, uint32_t max_iter,
                   IrlsResult* resall)
{
    __shared__ T sv[16];
    __shared__ uint32_t si[16];
    T* L = Lall + (size_t)blockIdx.x * n * n;
    T* vec = vecall + (size_t)blockIdx.x * vstride;
    IrlsResult* res = resall + blockIdx.x;
    T* qTb = vec;
    T* s = vec + n;
    T* xnext = vec + 2 * (size_t)n;
    T* w = vec + 3 * (size_t)n;
    T* x = vec + 4 * (size_t)n;
    T* t = vec + 5 * (size_t)n;
    const T* y = t + ldm;
    const uint32_t tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    constexpr int NW = kIbThreads / 64;
    const T p = T(0.9);

    for (uint32_t i = tid; i < n; i += kIbThreads) { x[i] = T(0); w[i] = T(1); xnext[i] = T(1); }
    for (uint32_t j = wave; j < n; j += NW) {
        T acc = T(0);
        const T* qj = Qt + (size_t)j * ldm;
        for (uint32_t r = lane; r < m; r += 64) acc += qj[r] * y[r];
        acc = wave_sum(acc);
        if (lane == 0) qTb[j] = acc;
    }
    __syncthreads();

    uint32_t iter = 0;
    int spd_error = 0;
    T abstol = T(1), eps = T(1), second = T(0);
    do {
        for (size_t e = tid; e < (size_t)n * n; e += kIbThreads) {
            const uint32_t i = (uint32_t)(e / n), j = (uint32_t)(e - (size_t)i * n);
            L[e] = j <= i ? G0[e] * w[j] : T(0);
        }
        __syncthreads();
        bool isspd = true;
        for (uint32_t j = 0; j < n; ++j) {
            if (j > 0) {
                const T* lj = L + (size_t)j * n;
                for (uint32_t i = j + wave; i < n; i += NW) {
                    const T* li = L + (size_t)i * n;
                    T acc = T(0);
                    for (uint32_t k2 = lane; k2 < j; k2 += 64) acc += li[k2] * lj[k2];
                    acc = wave_sum(acc);
                    if (lane == 0) s[i] = acc;
                }
                __syncthreads();
                for (uint32_t i = j + tid; i < n; i += kIbThreads) L[(size_t)i * n + j] -= s[i];
                __syncthreads();
            }
            const T ajj = sqrt(L[(size_t)j * n + j]);
            if (ajj <= Lim<T>::eps()) isspd = false;
            const T inv = T(1) / ajj;
            __syncthreads();
            for (uint32_t i = j + tid; i < n; i += kIbThreads) L[(size_t)i * n + j] *= inv;
            __syncthreads();
        }
        if (!isspd) { spd_error = 1; break; }
        for (uint32_t i = tid; i < n; i += kIbThreads) s[i] = qTb[i];
        __syncthreads();
        for (uint32_t i = 0; i < n; ++i) {
            T part = T(0);
            for (uint32_t k2 = tid; k2 < i; k2 += kIbThreads) part += L[(size_t)i * n + k2] * s[k2];
            const T acc = block_sum(part, sv);
            __syncthreads();
            if (tid == 0) s[i] = (s[i] - acc) / L[(size_t)i * n + i];
            __syncthreads();
        }
        for (uint32_t ii = n; ii-- > 0;) {
            T part = T(0);
            for (uint32_t k2 = ii + 1 + tid; k2 < n; k2 += kIbThreads) part += L[(size_t)k2 * n + ii] * s[k2];
            const T acc = block_sum(part, sv);
            __syncthreads();
            if (tid == 0) s[ii] = (s[ii] - acc) / L[(size_t)ii * n + ii];
            __syncthreads();
        }
        for (uint32_t r = tid; r < m; r += kIbThreads) {
            T acc = T(0);
            for (uint32_t j = 0; j < n; ++j) acc += Qt[(size_t)j * ldm + r] * s[j];
            t[r] = acc;
        }
        __syncthreads();
        for (uint32_t j = wave; j < n; j += NW) {
            T acc = T(0);
            const T* qj = Qt + (size_t)j * ldm;
            for (uint32_t r = lane; r < m; r += 64) acc += qj[r] * t[r];
            acc = wave_sum(acc);
            if (lane == 0) xnext[j] = acc;
        }
        __syncthreads();
        for (uint32_t ii = n; ii-- > 0;) {
            T part = T(0);
            for (uint32_t k2 = ii + 1 + tid; k2 < n; k2 += kIbThreads) part += R[(size_t)ii * n + k2] * xnext[k2];
            const T acc = block_sum(part, sv);
            __syncthreads();
            if (tid == 0) xnext[ii] = (xnext[ii] - acc) / R[(size_t)ii * n + ii];
            __syncthreads();
        }
        T mx;
        uint32_t mi;
        ib_max_excl(xnext, n, 0xffffffffu, mx, mi, sv, si);
        const bool has_nan = block_any_nan(xnext, n);             // (an exact-zero pivot of the QR: the reference's order decides)
        if (has_nan) mx = block_seq_max<T, false>(xnext, n, sv);
        abstol = mx * tol;
        for (uint32_t i = tid; i < n; i += kIbThreads) {
            const T v = xnext[i] < abstol ? T(0) : xnext[i];
            xnext[i] = v;
            x[i] = v;
        }
        __syncthreads();
        ib_max_excl(xnext, n, 0xffffffffu, mx, mi, sv, si);
        if (n >= 2) {
            T m2;
            uint32_t i2;
            ib_max_excl(xnext, n, mi, m2, i2, sv, si);
            second = m2;
        } else {
            second = mx;
        }
        if (has_nan) second = block_seq_max<T, true>(xnext, n, sv);
        {
            const T cand = second / T(n);
            if (cand < eps) eps = cand;
        }
        T part = T(0);
        for (uint32_t i = tid; i < n; i += kIbThreads) {
            const T v = (T)pow((double)(x[i] * x[i] + eps), (double)p / 2.0 - 1.0);
            w[i] = v;
            part += v;
        }
        const T sum = block_sum(part, sv);
        __syncthreads();
        for (uint32_t i = tid; i < n; i += kIbThreads) w[i] /= sum;
        __syncthreads();
        ++iter;
    } while (iter < max_iter && second > abstol);

    T part = T(0);
    for (uint32_t i = tid; i < n; i += kIbThreads) part += x[i];
    const T sum = block_sum(part, sv);
    __syncthreads();
    for (uint32_t i = tid; i < n; i += kIbThreads) x[i] /= sum;
    if (tid == 0) {
        res->iter = iter;
        res->spd_failure = (uint32_t)spd_error;
        res->solution_error = (double)eps;
    }
}

// ---- blocked lock-step form: the single solve's chain, slot = live[blockIdx.y] ---------------------------------------
// (every kernel below is its irls.hip namesake with the slot's L / vec / ctl; the per-element statements are unchanged)
struct IbSlots {
    const uint32_t* live;     // live slot numbers, ascending
    size_t lstride;           // elements of L per slot (n^2)
    size_t vstride;           // elements of vec per slot (5 n + 2 ldm)
};

template <typename T>
__global__ __launch_bounds__(256)
void k_irlsb_init(T* __restrict__ vecall, uint32_t n, size_t vstride, IbCtl<T>* __restrict__ ctlall, uint32_t* __restrict__ live)
{
    const uint32_t b = blockIdx.y;
    T* vec = vecall + (size_t)b * vstride;
    T* xnext = vec + 2 * (size_t)n;
    T* w = vec + 3 * (size_t)n;
    T* x = vec + 4 * (size_t)n;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) { x[i] = T(0); w[i] = T(1); xnext[i] = T(1); }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        IbCtl<T>* ctl = ctlall + b;
        ctl->eps = T(1); ctl->abstol = T(1); ctl->second = T(0); ctl->iter = 0; ctl->done = 0; ctl->spd_bad = 0;
        live[b] = b;
    }
}

// out_b[j] = Qt[j] . v_b for the slots live[G blockIdx.y + g], g < G (one wave per column of Q, k_irls_qt_vec's order per slot).
// voff / ooff: offsets of v and out in a slot's vec; check_done = false for Q^T y (k_irls_qt_vec with ctl == nullptr).
template <typename T, uint32_t G>
__global__ __launch_bounds__(256)
void k_irlsb_qt_vec(const T* __restrict__ Qt, uint32_t ldm, uint32_t m, uint32_t n, T* __restrict__ vecall, IbSlots sl,
                    uint32_t nlive, size_t voff, size_t ooff, const IbCtl<T>* __restrict__ ctlall, int check_done)
{
    const uint32_t lane = threadIdx.x & 63u, j = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (j >= n) return;
    const uint32_t g0 = blockIdx.y * G;
    const T* v[G];
    bool act[G];
    uint32_t slot[G];
#pragma unroll
    for (uint32_t g = 0; g < G; ++g) {
        const bool in = g0 + g < nlive;
        slot[g] = sl.live[in ? g0 + g : g0];
        act[g] = in && !(check_done && ctlall[slot[g]].done);
        v[g] = vecall + (size_t)slot[g] * sl.vstride + voff;
    }
    const T* q = Qt + (size_t)j * ldm;
    T acc[G];
#pragma unroll
    for (uint32_t g = 0; g < G; ++g) acc[g] = T(0);
    for (uint32_t r = lane; r < m; r += 64u) {
        const T qv = q[r];
#pragma unroll
        for (uint32_t g = 0; g < G; ++g) acc[g] += qv * v[g][r];
    }
#pragma unroll
    for (uint32_t g = 0; g < G; ++g) {
        const T a = wave_sum(acc[g]);
        if (lane == 0 && act[g]) vecall[(size_t)slot[g] * sl.vstride + ooff + j] = a;
    }
}

// t_b[r] = sum_j Qt[j][r] s_b[j] for the slots of a group (a thread per row, k_irls_q_vec's order per slot)
template <typename T, uint32_t G>
__global__ __launch_bounds__(256)
void k_irlsb_q_vec(const T* __restrict__ Qt, uint32_t ldm, uint32_t m, uint32_t n, T* __restrict__ vecall, IbSlots sl,
                   uint32_t nlive, const IbCtl<T>* __restrict__ ctlall)
{
    __shared__ T ss[G][256];
    const uint32_t g0 = blockIdx.y * G;
    const T* s[G];
    bool act[G];
    uint32_t slot[G];
    bool any = false;
#pragma unroll
    for (uint32_t g = 0; g < G; ++g) {
        const bool in = g0 + g < nlive;
        slot[g] = sl.live[in ? g0 + g : g0];
        act[g] = in && !ctlall[slot[g]].done;
        any = any || act[g];
        s[g] = vecall + (size_t)slot[g] * sl.vstride + n;
    }
    if (!any) return;
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    T acc[G];
#pragma unroll
    for (uint32_t g = 0; g < G; ++g) acc[g] = T(0);
    for (uint32_t j0 = 0; j0 < n; j0 += 256u) {
        __syncthreads();
        if (j0 + threadIdx.x < n) {
#pragma unroll
            for (uint32_t g = 0; g < G; ++g) ss[g][threadIdx.x] = s[g][j0 + threadIdx.x];
        }
        __syncthreads();
        const uint32_t cnt = n - j0 < 256u ? n - j0 : 256u;
        if (r < m)
            for (uint32_t j = 0; j < cnt; ++j) {
                const T qv = Qt[(size_t)(j0 + j) * ldm + r];
#pragma unroll
                for (uint32_t g = 0; g < G; ++g) acc[g] += qv * ss[g][j];
            }
    }
    if (r < m) {
#pragma unroll
        for (uint32_t g = 0; g < G; ++g)
            if (act[g]) vecall[(size_t)slot[g] * sl.vstride + 5 * (size_t)n + r] = acc[g];
    }
}

template <typename T>
__global__ __launch_bounds__(256)
void k_irlsb_scale(const T* __restrict__ G0, const T* __restrict__ vecall, T* __restrict__ Lall, uint32_t n, IbSlots sl,
                   const IbCtl<T>* __restrict__ ctlall)
{
    const uint32_t b = sl.live[blockIdx.y];
    if (ctlall[b].done) return;
    const T* w = vecall + (size_t)b * sl.vstride + 3 * (size_t)n;
    T* L = Lall + (size_t)b * sl.lstride;
    const size_t e = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (e >= (size_t)n * n) return;
    const uint32_t i = (uint32_t)(e / n), j = (uint32_t)(e - (size_t)i * n);
    L[e] = j <= i ? G0[e] * w[j] : T(0);
}

template <typename T>
__global__ __launch_bounds__(64)
void k_irlsb_chol_diag(T* __restrict__ Lall, uint32_t n, uint32_t k0, IbSlots sl, IbCtl<T>* __restrict__ ctlall)
{
    const uint32_t b = sl.live[blockIdx.y];
    IbCtl<T>* ctl = ctlall + b;
    if (ctl->done) return;
    T* L = Lall + (size_t)b * sl.lstride;
    __shared__ T colbuf[kIbB];
    __shared__ T s_diag;
    const uint32_t l = threadIdx.x;
    const uint32_t nb = n - k0 < kIbB ? n - k0 : kIbB;
    T row[kIbB];
#pragma unroll
    for (uint32_t c = 0; c < kIbB; ++c) row[c] = (l < nb && c <= l) ? L[(size_t)(k0 + l) * n + k0 + c] : T(0);
    bool bad = false;
#pragma unroll
    for (uint32_t c = 0; c < kIbB; ++c) {
        if (c < nb) {
            if (l == c) s_diag = row[c];
            __syncthreads();
            const T ajj = sqrt(s_diag);
            if (ajj <= Lim<T>::eps()) bad = true;
            const T inv = T(1) / ajj;
            if (l >= c && l < nb) row[c] *= inv;
            if (l < kIbB) colbuf[l] = row[c];
            __syncthreads();
#pragma unroll
            for (uint32_t c2 = c + 1; c2 < kIbB; ++c2)
                if (c2 < nb && l >= c2 && l < nb) row[c2] -= row[c] * colbuf[c2];
        }
    }
    if (l < nb) {
#pragma unroll
        for (uint32_t c = 0; c < kIbB; ++c)
            if (c <= l) L[(size_t)(k0 + l) * n + k0 + c] = row[c];
    }
    if (l == 0 && bad) ctl->spd_bad = 1;
}

template <typename T>
__global__ __launch_bounds__(256)
void k_irlsb_chol_below(T* __restrict__ Lall, uint32_t n, uint32_t k0, IbSlots sl, const IbCtl<T>* __restrict__ ctlall)
{
    const uint32_t b = sl.live[blockIdx.y];
    if (ctlall[b].done) return;
    T* L = Lall + (size_t)b * sl.lstride;
    __shared__ T D[kIbB][kIbB + 1];
    const uint32_t nb = kIbB;
    for (uint32_t e = threadIdx.x; e < kIbB * kIbB; e += 256u) { const uint32_t a = e / kIbB, c = e % kIbB; D[a][c] = L[(size_t)(k0 + a) * n + k0 + c]; }
    __syncthreads();
    const uint32_t i = k0 + kIbB + blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    T* row = L + (size_t)i * n + k0;
    T xv[kIbB];
#pragma unroll
    for (uint32_t c = 0; c < nb; ++c) {
        T a = row[c];
#pragma unroll
        for (uint32_t c2 = 0; c2 < c; ++c2) a -= xv[c2] * D[c][c2];
        xv[c] = a / D[c][c];
    }
#pragma unroll
    for (uint32_t c = 0; c < nb; ++c) row[c] = xv[c];
}

template <typename T>
__global__ __launch_bounds__(256)
void k_irlsb_chol_trail(T* __restrict__ Lall, uint32_t n, uint32_t k0, IbSlots sl, const IbCtl<T>* __restrict__ ctlall)
{
    const uint32_t bs = sl.live[blockIdx.y];
    if (ctlall[bs].done) return;
    T* L = Lall + (size_t)bs * sl.lstride;
    __shared__ T Pi[kIbB][kIbB + 1], Pj[kIbB][kIbB + 1];
    const uint32_t b = blockIdx.x;
    uint32_t t = (uint32_t)((sqrt(8.0 * (double)b + 1.0) - 1.0) * 0.5);
    while (t * (t + 1u) / 2u > b) --t;
    while ((t + 1u) * (t + 2u) / 2u <= b) ++t;
    const uint32_t ti = t, tj = b - t * (t + 1u) / 2u;
    const uint32_t base = k0 + kIbB;
    const uint32_t i0 = base + ti * kIbB, j0 = base + tj * kIbB;
    for (uint32_t e = threadIdx.x; e < kIbB * kIbB; e += 256u) {
        const uint32_t a = e / kIbB, c = e % kIbB;
        Pi[a][c] = i0 + a < n ? L[(size_t)(i0 + a) * n + k0 + c] : T(0);
        Pj[a][c] = j0 + a < n ? L[(size_t)(j0 + a) * n + k0 + c] : T(0);
    }
    __syncthreads();
    const uint32_t jj = threadIdx.x & 31u, ib = threadIdx.x >> 5;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
        const uint32_t ii = ib * 4u + q;
        const uint32_t i = i0 + ii, j = j0 + jj;
        if (i < n && j < n && j <= i) {
            T acc = T(0);
#pragma unroll
            for (uint32_t c = 0; c < kIbB; ++c) acc += Pi[ii][c] * Pj[jj][c];
            L[(size_t)i * n + j] -= acc;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(kIbThreads)
void k_irlsb_chol_solve(const T* __restrict__ Lall, uint32_t n, T* __restrict__ vecall, IbSlots sl, IbCtl<T>* __restrict__ ctlall)
{
    const uint32_t bs = sl.live[blockIdx.y];
    IbCtl<T>* ctl = ctlall + bs;
    if (ctl->done) return;
    const T* L = Lall + (size_t)bs * sl.lstride;
    T* vec = vecall + (size_t)bs * sl.vstride;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_ibcs[];
    T* ss = reinterpret_cast<T*>(smem_ibcs);
    __shared__ T D[kIbB][kIbB + 1];
    __shared__ T z[kIbB];
    const uint32_t tid = threadIdx.x;
    if (ctl->spd_bad) {
        if (tid == 0) ctl->done = 1;
        return;
    }
    const T* qTb = vec;
    T* s = vec + n;
    for (uint32_t i = tid; i < n; i += kIbThreads) ss[i] = qTb[i];
    __syncthreads();
    for (uint32_t b0 = 0; b0 < n; b0 += kIbB) {
        const uint32_t nb = n - b0 < kIbB ? n - b0 : kIbB;
        for (uint32_t e = tid; e < kIbB * kIbB; e += kIbThreads) { const uint32_t a = e / kIbB, c = e % kIbB; D[a][c] = (a < nb && c <= a) ? L[(size_t)(b0 + a) * n + b0 + c] : T(0); }
        __syncthreads();
        if (tid < 64) {
            T mine = tid < nb ? ss[b0 + tid] : T(0);
            for (uint32_t c = 0; c < nb; ++c) {
                const T zc = lane_value(mine, (int)c) / D[c][c];
                if (tid == c) mine = zc;
                else if (tid > c && tid < nb) mine -= D[tid][c] * zc;
            }
            if (tid < nb) { ss[b0 + tid] = mine; z[tid] = mine; }
        }
        __syncthreads();
        for (uint32_t i = b0 + kIbB + tid; i < n; i += kIbThreads) {
            const T* row = L + (size_t)i * n + b0;
            T acc = T(0);
#pragma unroll 8
            for (uint32_t c = 0; c < kIbB; ++c) acc += row[c] * z[c];
            ss[i] -= acc;
        }
        __syncthreads();
    }
    const uint32_t nblk = (n + kIbB - 1) / kIbB;
    for (uint32_t bb = nblk; bb-- > 0;) {
        const uint32_t b0 = bb * kIbB;
        const uint32_t nb = n - b0 < kIbB ? n - b0 : kIbB;
        for (uint32_t e = tid; e < kIbB * kIbB; e += kIbThreads) { const uint32_t a = e / kIbB, c = e % kIbB; D[a][c] = (a < nb && c <= a) ? L[(size_t)(b0 + a) * n + b0 + c] : T(0); }
        __syncthreads();
        if (tid < 64) {
            T mine = tid < nb ? ss[b0 + tid] : T(0);
            for (uint32_t cc = nb; cc-- > 0;) {
                const T xc = lane_value(mine, (int)cc) / D[cc][cc];
                if (tid == cc) mine = xc;
                else if (tid < cc) mine -= D[cc][tid] * xc;
            }
            if (tid < nb) { ss[b0 + tid] = mine; z[tid] = mine; }
        }
        __syncthreads();
        for (uint32_t i = tid; i < b0; i += kIbThreads) {
            T acc = T(0);
            for (uint32_t c = 0; c < nb; ++c) acc += L[(size_t)(b0 + c) * n + i] * z[c];
            ss[i] -= acc;
        }
        __syncthreads();
    }
    for (uint32_t i = tid; i < n; i += kIbThreads) s[i] = ss[i];
}

template <typename T>
__global__ __launch_bounds__(kIbThreads)
void k_irlsb_tail(const T* __restrict__ R, uint32_t n, T* __restrict__ vecall, T tol, uint32_t max_iter, IbSlots sl,
                  IbCtl<T>* __restrict__ ctlall)
{
    const uint32_t bs = sl.live[blockIdx.y];
    IbCtl<T>* ctl = ctlall + bs;
    if (ctl->done) return;
    T* vec = vecall + (size_t)bs * sl.vstride;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_ibtl[];
    T* xs = reinterpret_cast<T*>(smem_ibtl);
    __shared__ T D[kIbB][kIbB + 1];
    __shared__ T z[kIbB];
    __shared__ T sv[16];
    __shared__ uint32_t si[16];
    const uint32_t tid = threadIdx.x;
    T* xnext = vec + 2 * (size_t)n;
    T* w = vec + 3 * (size_t)n;
    T* x = vec + 4 * (size_t)n;
    const T p = T(0.9);
    for (uint32_t i = tid; i < n; i += kIbThreads) xs[i] = xnext[i];
    __syncthreads();
    const uint32_t nblk = (n + kIbB - 1) / kIbB;
    for (uint32_t bb = nblk; bb-- > 0;) {
        const uint32_t b0 = bb * kIbB;
        const uint32_t nb = n - b0 < kIbB ? n - b0 : kIbB;
        for (uint32_t e = tid; e < kIbB * kIbB; e += kIbThreads) { const uint32_t a = e / kIbB, c = e % kIbB; D[a][c] = (a < nb && c < nb && c >= a) ? R[(size_t)(b0 + a) * n + b0 + c] : T(0); }
        __syncthreads();
        if (tid < 64) {
            T mine = tid < nb ? xs[b0 + tid] : T(0);
            for (uint32_t cc = nb; cc-- > 0;) {
                const T xc = lane_value(mine, (int)cc) / D[cc][cc];
                if (tid == cc) mine = xc;
                else if (tid < cc) mine -= D[tid][cc] * xc;
            }
            if (tid < nb) { xs[b0 + tid] = mine; z[tid] = mine; }
        }
        __syncthreads();
        for (uint32_t i = tid; i < b0; i += kIbThreads) {
            const T* row = R + (size_t)i * n + b0;
            T acc = T(0);
            for (uint32_t c = 0; c < nb; ++c) acc += row[c] * z[c];
            xs[i] -= acc;
        }
        __syncthreads();
    }
    for (uint32_t i = tid; i < n; i += kIbThreads) xnext[i] = xs[i];
    __syncthreads();
    T mx;
    uint32_t mi;
    ib_max_excl(xnext, n, 0xffffffffu, mx, mi, sv, si);
    const bool has_nan = block_any_nan(xnext, n);                 // (an exact-zero pivot of the QR: the reference's order decides)
    if (has_nan) mx = block_seq_max<T, false>(xnext, n, sv);
    const T abstol = mx * tol;
    for (uint32_t i = tid; i < n; i += kIbThreads) {
        const T v = xnext[i] < abstol ? T(0) : xnext[i];
        xnext[i] = v;
        x[i] = v;
    }
    __syncthreads();
    ib_max_excl(xnext, n, 0xffffffffu, mx, mi, sv, si);
    T second;
    if (n >= 2) {
        T m2;
        uint32_t i2;
        ib_max_excl(xnext, n, mi, m2, i2, sv, si);
        second = m2;
    } else {
        second = mx;
    }
    if (has_nan) second = block_seq_max<T, true>(xnext, n, sv);
    T eps = ctl->eps;
    {
        const T cand = second / T(n);
        if (cand < eps) eps = cand;
    }
    T part = T(0);
    for (uint32_t i = tid; i < n; i += kIbThreads) {
        const T v = (T)pow((double)(x[i] * x[i] + eps), (double)p / 2.0 - 1.0);
        w[i] = v;
        part += v;
    }
    const T sum = block_sum(part, sv);
    __syncthreads();
    for (uint32_t i = tid; i < n; i += kIbThreads) w[i] /= sum;
    if (tid == 0) {
        const uint32_t it = ctl->iter + 1u;
        ctl->iter = it;
        ctl->eps = eps;
        ctl->abstol = abstol;
        ctl->second = second;
        if (!(it < max_iter && second > abstol)) ctl->done = 1;
    }
}

// the live list: slots 0 .. nslots - 1 whose done word is 0, ascending, and their number in live[nslots] (one workgroup)
template <typename T>
__global__ __launch_bounds__(256)
void k_irlsb_live(const IbCtl<T>* __restrict__ ctlall, uint32_t nslots, uint32_t* __restrict__ live)
{
    __shared__ uint32_t wcnt[4];
    __shared__ uint32_t s_base;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (tid == 0) s_base = 0u;
    __syncthreads();
    for (uint32_t c0 = 0; c0 < nslots; c0 += 256u) {
        const uint32_t b = c0 + tid;
        const bool on = b < nslots && ctlall[b].done == 0u;
        const uint64_t mask = __ballot(on);
        if (lane == 0) wcnt[wave] = (uint32_t)__popcll(mask);
        __syncthreads();
        uint32_t off = s_base;
        for (uint32_t w = 0; w < wave; ++w) off += wcnt[w];
        off += (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        if (on) live[off] = b;
        __syncthreads();
        if (tid == 0) s_base += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        __syncthreads();
    }
    if (tid == 0) live[nslots] = s_base;
}

// k_irls_finish per slot (every slot of the chunk)
template <typename T>
__global__ __launch_bounds__(kIbThreads)
void k_irlsb_finish(T* __restrict__ vecall, uint32_t n, size_t vstride, const IbCtl<T>* __restrict__ ctlall, IrlsResult* __restrict__ resall)
{
    __shared__ T sv[16];
    const uint32_t b = blockIdx.x;
    T* x = vecall + (size_t)b * vstride + 4 * (size_t)n;
    const IbCtl<T>* ctl = ctlall + b;
    const uint32_t tid = threadIdx.x;
    T part = T(0);
    for (uint32_t i = tid; i < n; i += kIbThreads) part += x[i];
    const T sum = block_sum(part, sv);
    __syncthreads();
    for (uint32_t i = tid; i < n; i += kIbThreads) x[i] /= sum;
    if (tid == 0) {
        resall[b].iter = ctl->iter;
        resall[b].spd_failure = ctl->spd_bad;
        resall[b].solution_error = (double)ctl->eps;
    }
}

// ---- workspace ---------------------------------------------------------------------------------------------------------
// the buffers that grow with the chunk, owned by `own`: a regrow is a fresh IbBuffers
struct IbBuffers {
    Holdings own;
    uint32_t cap = 0;             // slots the buffers hold
    void* L = nullptr;            // [cap][n][n]
    void* vec = nullptr;          // [cap][5 n + 2 ldm]
    void* ctl = nullptr;          // [cap] IbCtl<T>
    IrlsResult* res = nullptr;    // [cap]
    uint32_t* live = nullptr;     // [cap + 1]: the live list, then its length
};
struct IrlsBatchWs : IbBuffers {
    int is_f64 = 0;
    Holdings pinned;
    uint32_t* nlive_host = nullptr;   // pinned: the live count, read once per round
};

void free_buffers(IrlsBatchWs* W) { static_cast<IbBuffers&>(*W) = IbBuffers(); }

template <typename T>
size_t slot_bytes(const ss_hip_ctx* ctx)
{
    const size_t n = ctx->n, ldm = ctx->ldm;
    return (n * n + 5 * n + 2 * ldm) * sizeof(T) + sizeof(IbCtl<T>) + sizeof(IrlsResult) + sizeof(uint32_t);
}

template <typename T>
hipError_t alloc_buffers(ss_hip_ctx* ctx, IrlsBatchWs* W, uint32_t cap)
{
    const size_t n = ctx->n, ldm = ctx->ldm;
    hipError_t e;
    if ((e = W->own.device(&W->L, (size_t)cap * n * n * sizeof(T))) != hipSuccess) return e;
    if ((e = W->own.device(&W->vec, (size_t)cap * (5 * n + 2 * ldm) * sizeof(T))) != hipSuccess) return e;
    if ((e = W->own.device(&W->ctl, (size_t)cap * sizeof(IbCtl<T>))) != hipSuccess) return e;
    if ((e = W->own.device(&W->res, (size_t)cap * sizeof(IrlsResult))) != hipSuccess) return e;
    if ((e = W->own.device(&W->live, ((size_t)cap + 1) * sizeof(uint32_t))) != hipSuccess) return e;
    // (y rows m .. ldm - 1 are never read; zeroed so that no stale words are ever in play)
    if ((e = hipMemsetAsync(W->vec, 0, (size_t)cap * (5 * n + 2 * ldm) * sizeof(T), ctx->stream)) != hipSuccess) return e;
    W->cap = cap;
    return hipSuccess;
}

}  // namespace

// The batch's chunk size for B signals: min(B, irls_batch_max, the byte budget), the workspace grown to hold it.  A failed
// allocation halves the chunk before it gives up.
template <typename T>
hipError_t irls_batch_reserve(ss_hip_ctx* ctx, size_t B, uint32_t* chunk)
{
    auto* W = ctx->irls_batch.as<IrlsBatchWs>();
    if (W == nullptr) {
        W = &part<IrlsBatchWs>(ctx->irls_batch);
        W->is_f64 = sizeof(T) == 8;
        const hipError_t e = W->pinned.pinned(&W->nlive_host, 64, hipHostMallocDefault);
        if (e != hipSuccess) { ctx->irls_batch.reset(); return e; }      // (the next batch tries again)
    }
    size_t want = std::min<size_t>(B, (size_t)std::max(1, ctx->irls_batch_max));
    want = std::min<size_t>(want, std::max<size_t>(1, kIbBudget / slot_bytes<T>(ctx)));
    want = std::min<size_t>(want, 65535);                           // (grid y)
    uint32_t c = (uint32_t)want;
    if (W->cap >= c) { *chunk = c; return hipSuccess; }
    {
        const hipError_t e = hipStreamSynchronize(ctx->stream);     // (the old buffers may still be in use)
        if (e != hipSuccess) return e;
    }
    free_buffers(W);
    for (;;) {
        const hipError_t e = alloc_buffers<T>(ctx, W, c);
        if (e == hipSuccess) { *chunk = c; return hipSuccess; }
        (void)hipGetLastError();
        free_buffers(W);
        if (c == 1) return e;
        c = (c + 1) / 2;
    }
}

template <typename T>
T* irls_batch_y(ss_hip_ctx* ctx, uint32_t b)
{
    auto* W = ctx->irls_batch.as<IrlsBatchWs>();
    return static_cast<T*>(W->vec) + (size_t)b * (5 * ctx->n + 2 * (size_t)ctx->ldm) + 5 * ctx->n + ctx->ldm;
}

template <typename T>
T* irls_batch_x(ss_hip_ctx* ctx, uint32_t b)
{
    auto* W = ctx->irls_batch.as<IrlsBatchWs>();
    return static_cast<T*>(W->vec) + (size_t)b * (5 * ctx->n + 2 * (size_t)ctx->ldm) + 4 * ctx->n;
}

// One chunk: y of slot b in irls_batch_y(b), x left in irls_batch_x(b), reports copied to res_host[0 .. nb) (stream-ordered).
// *rounds receives the lock-step rounds run (0 for the one-workgroup form).
template <typename T>
hipError_t irls_batch_run(ss_hip_ctx* ctx, const T* Qt, const T* R, const T* G0, uint32_t nb, T tol, uint32_t max_iter,
                          IrlsResult* res_host, uint64_t* rounds)
{
#define IB_TRY(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) return e_; } while (0)
    auto* W = ctx->irls_batch.as<IrlsBatchWs>();
    const uint32_t n = (uint32_t)ctx->n, m = (uint32_t)ctx->m, ldm = ctx->ldm;
    const size_t vstride = 5 * (size_t)n + 2 * (size_t)ldm;
    hipStream_t st = ctx->stream;
    T* L = static_cast<T*>(W->L);
    T* vec = static_cast<T*>(W->vec);
    IbCtl<T>* ctl = static_cast<IbCtl<T>*>(W->ctl);
    *rounds = 0;
    // the single solve's choice of form (irls_solve in irls.hip)
    const size_t vec_lds = (size_t)n * sizeof(T);
    if (n < kIbBlockedMin || vec_lds > 96 * 1024 || std::getenv("SS_HIP_IRLS_FUSED")) {
        hipLaunchKernelGGL((k_irlsb_solve<T>), dim3(nb), dim3(kIbThreads), 0, st, Qt, R, G0, L, vec, ldm, m, n, vstride, tol,
                           max_iter, W->res);
        IB_TRY(hipGetLastError());
        IB_TRY(hipMemcpyAsync(res_host, W->res, (size_t)nb * sizeof(IrlsResult), hipMemcpyDeviceToHost, st));
        return hipSuccess;
    }
    static const bool attr_ok = [] {
        const bool a = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_irlsb_chol_solve<T>), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024) == hipSuccess;
        const bool b = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_irlsb_tail<T>), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024) == hipSuccess;
        if (!(a && b)) (void)hipGetLastError();
        return a && b;
    }();
    if (!attr_ok) return hipErrorInvalidConfiguration;
    IbSlots sl{ W->live, (size_t)n * n, vstride };
    hipLaunchKernelGGL((k_irlsb_init<T>), dim3((n + 255) / 256, nb), dim3(256), 0, st, vec, n, vstride, ctl, W->live);
    // qTb = Q^T y of every slot: y at 5 n + ldm, qTb at 0
    hipLaunchKernelGGL((k_irlsb_qt_vec<T, kQGroup>), dim3((n + 3) / 4, (nb + kQGroup - 1) / kQGroup), dim3(256), 0, st, Qt, ldm, m, n,
                       vec, sl, nb, 5 * (size_t)n + ldm, (size_t)0, (const IbCtl<T>*)ctl, 0);
    IB_TRY(hipGetLastError());
    uint32_t nlive = nb;
    for (uint32_t it = 0; it < max_iter && nlive > 0; ++it) {
        const dim3 one(1, nlive);
        hipLaunchKernelGGL((k_irlsb_scale<T>), dim3((unsigned)(((size_t)n * n + 255) / 256), nlive), dim3(256), 0, st, G0, (const T*)vec, L, n, sl,
                           (const IbCtl<T>*)ctl);
        for (uint32_t k0 = 0; k0 < n; k0 += kIbB) {
            hipLaunchKernelGGL((k_irlsb_chol_diag<T>), one, dim3(64), 0, st, L, n, k0, sl, ctl);
            if (k0 + kIbB < n) {
                const uint32_t below = n - (k0 + kIbB);
                hipLaunchKernelGGL((k_irlsb_chol_below<T>), dim3((below + 255) / 256, nlive), dim3(256), 0, st, L, n, k0, sl, (const IbCtl<T>*)ctl);
                const uint32_t T_ = (below + kIbB - 1) / kIbB;
                hipLaunchKernelGGL((k_irlsb_chol_trail<T>), dim3(T_ * (T_ + 1) / 2, nlive), dim3(256), 0, st, L, n, k0, sl, (const IbCtl<T>*)ctl);
            }
        }
        hipLaunchKernelGGL((k_irlsb_chol_solve<T>), one, dim3(kIbThreads), vec_lds, st, (const T*)L, n, vec, sl, ctl);
        const dim3 grp_q((m + 255) / 256, (nlive + kQGroup - 1) / kQGroup), grp_qt((n + 3) / 4, (nlive + kQGroup - 1) / kQGroup);
        hipLaunchKernelGGL((k_irlsb_q_vec<T, kQGroup>), grp_q, dim3(256), 0, st, Qt, ldm, m, n, vec, sl, nlive, (const IbCtl<T>*)ctl);
        // xnext = Q^T t: t at 5 n, xnext at 2 n
        hipLaunchKernelGGL((k_irlsb_qt_vec<T, kQGroup>), grp_qt, dim3(256), 0, st, Qt, ldm, m, n, vec, sl, nlive, 5 * (size_t)n,
                           2 * (size_t)n, (const IbCtl<T>*)ctl, 1);
        hipLaunchKernelGGL((k_irlsb_tail<T>), one, dim3(kIbThreads), vec_lds, st, R, n, vec, tol, max_iter, sl, ctl);
        hipLaunchKernelGGL((k_irlsb_live<T>), dim3(1), dim3(256), 0, st, (const IbCtl<T>*)ctl, nb, W->live);
        IB_TRY(hipGetLastError());
        IB_TRY(hipMemcpyAsync(W->nlive_host, W->live + nb, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        IB_TRY(hipStreamSynchronize(st));
        nlive = *W->nlive_host;
        *rounds += 1;
    }
    hipLaunchKernelGGL((k_irlsb_finish<T>), dim3(nb), dim3(kIbThreads), 0, st, vec, n, vstride, (const IbCtl<T>*)ctl, W->res);
    IB_TRY(hipGetLastError());
    IB_TRY(hipMemcpyAsync(res_host, W->res, (size_t)nb * sizeof(IrlsResult), hipMemcpyDeviceToHost, st));
    return hipSuccess;
#undef IB_TRY
}

template hipError_t irls_batch_reserve<float>(ss_hip_ctx*, size_t, uint32_t*);
template hipError_t irls_batch_reserve<double>(ss_hip_ctx*, size_t, uint32_t*);
template float* irls_batch_y<float>(ss_hip_ctx*, uint32_t);
template double* irls_batch_y<double>(ss_hip_ctx*, uint32_t);
template float* irls_batch_x<float>(ss_hip_ctx*, uint32_t);
template double* irls_batch_x<double>(ss_hip_ctx*, uint32_t);
template hipError_t irls_batch_run<float>(ss_hip_ctx*, const float*, const float*, const float*, uint32_t, float, uint32_t, IrlsResult*, uint64_t*);
template hipError_t irls_batch_run<double>(ss_hip_ctx*, const double*, const double*, const double*, uint32_t, double, uint32_t, IrlsResult*, uint64_t*);

}  // namespace sship
