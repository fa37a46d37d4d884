// The selection of the top correlations, stated once (topcorr.hip, nonneg.hip, weighted.hip, joint.hip): the chunk's constants, the
// choice of the k best columns of one row under the total order (score descending, index ascending) — tc_select_sorted, parameterised
// by where a column's key comes from — and k_tc_select, the kernel of the calls whose row is a signal: it strikes the record's
// columns out of the row of D, selects, and writes idx / coef / score; what a candidate is, its key and its coef come from a small
// device-side SCORER the call passes by value.  joint.hip's k_js_select calls tc_select_sorted with a group's stored score.
// Integer and comparison logic only outside the scorers: the result is a function of the keys, whichever kernel asks.
// Everything sits in an unnamed namespace: each unit gets its own copy, nothing here is part of the library's link surface.
#pragma once

#include "ss_hip_internal.h"

namespace sship {

namespace {

constexpr uint32_t kTcTile = 128;                        // signals and columns per tile
constexpr uint32_t kTcNone = SS_HIP_TOPCORR_NONE;
constexpr uint32_t kTcList = 1024;                       // entries of the selection's LDS list (>= 2 SS_HIP_TOPCORR_KMAX)
constexpr uint32_t kTcChunkMax = 32768;                  // most signals per chunk (grid.y of the residual kernels)
constexpr size_t kTcChunkBytes = (size_t)1536 << 20;     // the byte budget of a chunk's residuals and dots (never changes a result)
static_assert(kTcList >= 2 * SS_HIP_TOPCORR_KMAX, "the list holds the k best and a boundary bin");

// the quiet NaN that strikes a column out: a NaN score is never selected
__device__ inline float tc_nan(float) { return __int_as_float(0x7fc00000); }
__device__ inline double tc_nan(double) { return __longlong_as_double(0x7ff8000000000000ll); }

// (key, index): a comes before b when its score is larger, or equal with the smaller index; the keys are the bits of non-negative
// doubles, which order as the doubles do
__device__ inline bool tc_before(unsigned long long ka, uint32_t ia, unsigned long long kb, uint32_t ib) { return ka > kb || (ka == kb && ia < ib); }

// the LDS of a selection (one per workgroup of 256 threads)
struct TcSelectLds {
    unsigned long long lkey[kTcList];
    uint32_t lidx[kTcList];
    uint32_t hist[256];
    uint32_t sh[4], wcnt[4];
};

// The k best of the columns 0 .. n - 1 by the total order.  keyof(i, key): the key of column i, false for a column that is no
// candidate.  A radix selection on the key's bits — eight bits a pass, LDS histogram of integer counts — until the columns that can
// still be among the k best fit the list, which is sorted by the total order (bitonic).  All columns tied on the k-th key: the
// smallest indices are taken in ascending blocks.  Every thread of the workgroup (256) calls it; -> L, the number of entries:
// s.lkey / s.lidx [0 .. L) hold them in order (L >= min(k, candidates): the first k are the result, a prefix for every smaller k).
template <typename KeyOf>
__device__ inline uint32_t tc_select_sorted(TcSelectLds& s, uint32_t n, uint32_t k, KeyOf keyof)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;

    // ---- radix selection: P = the bits above `shift` of the k-th best key so far as they are known, `above` columns lie in higher
    // bins (all of them among the k best), `need` more come from the bin of P, which holds c columns ----
    unsigned long long P = 0;
    uint32_t need = k, above = 0, c = 0;
    int shift = 56;
    bool ties = false;
    for (;;) {
        s.hist[tid] = 0u;
        __syncthreads();
        for (uint32_t i = tid; i < n; i += 256u) {
            unsigned long long key;
            if (keyof(i, key) && (shift == 56 || (key >> (shift + 8)) == P)) atomicAdd(&s.hist[(uint32_t)(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t cum = 0, bin = 0;
            bool found = false;
            for (int bb = 255; bb >= 0; --bb) {
                if (cum + s.hist[bb] >= need) { bin = (uint32_t)bb; found = true; break; }
                cum += s.hist[bb];
            }
            if (!found) cum -= s.hist[0];                        // fewer candidates than k (first pass only): all of them, bin 0 last
            s.sh[0] = bin;
            s.sh[1] = cum;
            s.sh[2] = s.hist[bin];
        }
        __syncthreads();
        const uint32_t bin = s.sh[0], cum = s.sh[1];
        c = s.sh[2];
        above += cum;
        need -= cum < need ? cum : need;
        P = (P << 8) | bin;
        if (above + c <= kTcList) break;
        if (shift == 0) { ties = true; break; }
        shift -= 8;
    }

    // ---- the list: every column above the bin, and the bin itself unless it is one exact score that more than the list share ----
    if (tid == 0) s.sh[3] = 0u;
    __syncthreads();
    for (uint32_t i = tid; i < n; i += 256u) {
        unsigned long long key;
        if (!keyof(i, key)) continue;
        const unsigned long long top = key >> shift;
        if (top > P || (top == P && !ties)) {
            const uint32_t slot = atomicAdd(&s.sh[3], 1u);
            s.lkey[slot] = key;
            s.lidx[slot] = i;
        }
    }
    __syncthreads();
    uint32_t L = s.sh[3];
    if (ties) {
        // every column of the bin has the key P: the `need` smallest indices, in ascending blocks of 256
        for (uint32_t base = 0; base < n && need != 0u; base += 256u) {
            const uint32_t i = base + tid;
            unsigned long long key = 0;
            const bool mine = i < n && keyof(i, key) && key == P;
            const unsigned long long mask = __ballot(mine);
            if (lane == 0) s.wcnt[wave] = (uint32_t)__popcll(mask);
            __syncthreads();
            uint32_t before = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull)), total = 0;
            for (uint32_t w = 0; w < 4u; ++w) { if (w < wave) before += s.wcnt[w]; total += s.wcnt[w]; }
            if (mine && before < need) { s.lkey[L + before] = key; s.lidx[L + before] = i; }
            const uint32_t taken = total < need ? total : need;
            L += taken;
            need -= taken;
            __syncthreads();
        }
    }
    uint32_t S = 1;
    while (S < L) S <<= 1;
    for (uint32_t t = L + tid; t < S; t += 256u) { s.lkey[t] = 0ull; s.lidx[t] = kTcNone; }      // (behind every column: the largest index)
    for (uint32_t size = 2; size <= S; size <<= 1)
        for (uint32_t stride = size >> 1; stride > 0u; stride >>= 1) {
            __syncthreads();
            for (uint32_t t = tid; t < S / 2u; t += 256u) {
                const uint32_t lo = 2u * t - (t & (stride - 1u)), hi = lo + stride;
                const unsigned long long ka = s.lkey[lo], kb = s.lkey[hi];
                const uint32_t ia = s.lidx[lo], ib = s.lidx[hi];
                const bool fwd = (lo & size) == 0u;
                if (fwd ? tc_before(kb, ib, ka, ia) : tc_before(ka, ia, kb, ib)) { s.lkey[lo] = kb; s.lidx[lo] = ib; s.lkey[hi] = ka; s.lidx[hi] = ia; }
            }
        }
    __syncthreads();
    return L;
}

// One workgroup per signal.  D: the chunk's dots, row b of it is this workgroup's to strike columns out of; rec == nullptr: no
// records.  Scorer: sc.row(b, n_pad) -> the scorer of signal b, with key(d, i, key) — the key of column i from the row d, false for
// a column that is no candidate — and coef(d, i), the coefficient of a selected column
template <typename T, typename Scorer>
__global__ __launch_bounds__(256)
void k_tc_select(T* __restrict__ D, uint32_t n, uint32_t n_pad, const Scorer sc, const unsigned char* __restrict__ rec, size_t rb, uint32_t kmax,
                 uint32_t k, uint32_t* __restrict__ oidx, T* __restrict__ ocoef, double* __restrict__ oscore)
{
    __shared__ TcSelectLds lds;
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    T* d = D + (size_t)b * n_pad;
    oidx += (size_t)b * k;
    ocoef += (size_t)b * k;
    oscore += (size_t)b * k;
    if (rec) {
        const unsigned char* r = rec + (size_t)b * rb;
        const uint32_t K = *reinterpret_cast<const uint32_t*>(r);
        if (K > kmax) {                                          // a truncated record does not hold its support: no candidates
            for (uint32_t t = tid; t < k; t += 256u) { oidx[t] = kTcNone; ocoef[t] = T(0); oscore[t] = 0.0; }
            return;
        }
        const uint32_t* idx = reinterpret_cast<const uint32_t*>(r + 16);
        for (uint32_t e = tid; e < K; e += 256u) d[idx[e]] = tc_nan(T(0));        // (idx < n: tc_launch_record_check)
        __threadfence_block();
        __syncthreads();
    }
    const auto row = sc.row(b, n_pad);
    auto keyof = [&](uint32_t i, unsigned long long& key) -> bool { return row.key(d, i, key); };
    const uint32_t L = tc_select_sorted(lds, n, k, keyof);
    for (uint32_t t = tid; t < k; t += 256u) {
        if (t < L) {
            const uint32_t i = lds.lidx[t];
            oidx[t] = i;
            ocoef[t] = row.coef(d, i);
            oscore[t] = __longlong_as_double((long long)lds.lkey[t]);
        } else {
            oidx[t] = kTcNone;
            ocoef[t] = T(0);
            oscore[t] = 0.0;
        }
    }
}

}  // namespace

}  // namespace sship
