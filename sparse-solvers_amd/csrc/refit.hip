// refit.hip — the least-squares refit of compact records on their supports (debiasing), on the device (include/ss_hip.h):
//   ss_hip_refit_records_*.
//
// A Homotopy record holds the LASSO solution at lambda ~ tol: the right support, every coefficient shrunk by the l1 penalty.  For
// signal b with the record's stored columns S (record order, K of them) the refit replaces val[0 .. K) by
//   z = argmin || y_b - A_S z ||_2,      the solution of the normal equations (A_S^T A_S) z = A_S^T y_b,
// and copies everything else of the record word for word.  Only the record's columns of A are read, one contiguous run of ldm
// elements each (ctx->At, [n_pad][ldm]): sum K_b * ldm elements, never a resident G = A^T A (whose words depend on what the context
// did before).  Three kernels:
//
//   k_rf_check   one workgroup per signal, the whole batch before anything is written: the status from K (EMPTY, TRUNCATED,
//                TOO_LARGE, else DONE), and the first record with a column index >= n — never used as an address.
//   k_rf_gram    grid = (row chunk, signal).  The panel P = [A_S | y] (K + 1 columns, padded with zero columns to a multiple of 16)
//                is staged through LDS 32 rows at a time, the next stage's loads in flight under the MFMAs; the lower triangle of
//                P^T P (G = A_S^T A_S, and h = A_S^T y as its row K) is formed in 16 x 16 tiles on v_mfma_f32_16x16x4_f32 /
//                v_mfma_f64_16x16x4_f64, the tiles dealt round-robin to the four waves.  One partial per (signal, chunk, tile).
//   k_rf_solve   one workgroup per signal: the chunk partials added up in double, the packed lower triangle of [G h; h^T .] in LDS
//                ((K + 1)(K + 2) / 2 doubles, 104 KB at K = 160), its Cholesky factorisation column by column — row K takes the
//                forward substitution along — the pivot test, the back substitution, z rounded once to T into the output record.
// The residual norms are the words of ss_hip_class_residuals_* with every column in class 0 on the records as written: its kernels,
// reached through record_residual_norms (classify.hip).
// The weighted refit (ss_hip_weighted_refit_records_*, weighted.hip) is this unit with a flag: refit_weighted is refit_entry with the
// weights checked and brought to the device, k_rf_gram<T, NT, true> forms P^T W_b P (one operand scaled by w_k), k_rf_solve is the
// same kernel, the residual norms are the weighted ones (weighted_residual_rows).  The unflagged instantiations are the code they were.
// The non-negative refit (ss_hip_nonneg_refit_records_*, nonneg.hip) is this unit with another flag: refit_nonneg is refit_entry with
// k_rf_cap behind k_rf_check (a DONE record of more than SS_HIP_NNLS_KMAX columns becomes TOO_LARGE), k_rf_gram as it is, and
//   k_rf_nnls    in k_rf_solve's place, one workgroup per signal: Lawson-Hanson on the same [G h; h^T y^T y] in double, in LDS.
// The l1 refit (ss_hip_lasso_refit_records_*, lasso.hip) is this unit with a fourth flag: refit_lasso is refit_entry with k_rf_lam beside
// k_rf_check (the lam_b brought to the device, a negative or non-finite one reported before anything is written), k_rf_cap, and
//   k_rf_lasso   in k_rf_solve's place, one workgroup per signal: k_rf_nnls with a sign and a penalty — the fixed-lambda LASSO, with
//                ridge > 0 the elastic net — on the same [G h; h^T y^T y] in double, in LDS.
// The pruning call (ss_hip_prune_records_*, pursuit.hip) is this unit with a third flag: refit_prune is refit_entry with k_rf_check and
// k_rf_gram as they are and
//   k_rf_prune   in k_rf_solve's place, one workgroup per signal: k_rf_solve's solve on the whole record, a score per entry, the
//                entries to keep, and k_rf_solve's solve once more on the kept sub-block of the SAME panel words — G_ij is one chain
//                over the rows whichever tile holds it, so the panel of the kept record is a sub-block of this one word for word, and
//                the record written is what ss_hip_refit_records_* returns for it.  One Gram panel a call, not two.
//
// SUMMATION ORDER (the tests' bounds follow from it; build flag -ffp-contract=off: products and sums are rounded separately outside
// the MFMA, whose four products per instruction are a chain of fused multiply-adds):
//   row chunks   of kRfRows = 1024 rows: chunk c holds rows 1024 c .. min(1024 c + 1023, ldm - 1) — a function of m alone (rows
//                m .. ldm - 1 of At and of y are zero);
//   a partial    G_c[i][j] = sum over the chunk's rows r, ascending, of P[r][i] * P[r][j]: one accumulator per element, started at 0,
//                fma after fma in the context's precision (the longest chain: 1024 terms) — whichever wave or tile holds it;
//   G, h         = the chunk partials added one after the other in ascending chunk order, in double, starting from 0;
//   Cholesky     in double, right-looking: for j ascending  d_j = G_jj as updated so far (the pivot),  l_jj = sqrt(d_j),
//                l_ij = G_ij / l_jj for i > j (row K: w_j = h_j / l_jj),  then G_ik = G_ik - l_ij * l_kj for j < k <= i: every
//                element takes its updates one after the other in ascending j;
//   pivot test   the signal is SINGULAR when for some j  !(d_j > 8 K eps(T) G_jj)  with G_jj the diagonal before any update (a NaN
//                fails it; a column named twice gives a second pivot of rounding size, an all-zero column G_jj = 0);
//   back subst.  for j descending  z_j = w_j / l_jj,  then w_i = w_i - l_ji * z_j for i < j, in double;
//   val[e]       = z_e rounded once to T.
// NNLS ORDER (k_rf_nnls; G, h and y^T y are the words above, everything below in double, products and sums rounded separately):
//   state        P, the passive set, a list of record positions in the order they entered; z by record position, 0 outside P;
//                start P empty, z = 0.  L, the Cholesky factor of G_PP in P's order, row p packed at p (p + 1) / 2; u = L^-1 h_P.
//   entry test   for every position e not in P, ascending i over P's members BY RECORD POSITION:  w_e = h_e, then w_e = w_e - G_ei * z_i.
//                tau_e = 8 K eps(T) sqrt(G_ee * y^T y) (one product, one root, one product).  Among the e with w_e > tau_e the
//                largest w_e enters, ties to the smallest position; none: the signal is done.  (A comparison, so a NaN never enters.)
//   row p        the factor's row for column j = P[p]:  v_i = G_{j, P[i]} for i < p;  for k ascending  l_k = v_k / L_kk,  then
//                v_i = v_i - L_ik * l_k for k < i < p;  the pivot d = G_jj, then d = d - l_k * l_k in ascending k;  c = h_j, then
//                c = c - l_k * u_k in ascending k;  the signal is SINGULAR when !(d > 8 K eps(T) G_jj);  L_pp = sqrt(d), u_p = c / L_pp.
//                A column that enters appends its row; after a removal the rows 0, 1, ... of the shortened list are formed again
//                by the same statements — the factor is a function of the list, never of how the list came about.
//   a solve      L^T s = u:  t = u, for k descending  s_k = t_k / L_kk,  then t_i = t_i - L_ki * s_k for i < k.  At most 3 K solves
//                a signal; one more needed: SS_HIP_REFIT_STALLED.
//   inner loop   every s_p > 0: z_P = s, back to the entry test.  Else over the p with !(s_p > 0) in P's order  a_p = z_p / (z_p - s_p)
//                (0 where z_p is 0: a column that has just entered), alpha = their minimum, attained first at p*;  z_p = z_p +
//                alpha * (s_p - z_p) for every p;  p* and every p with !(z_p > 0) leave P with z = 0 exactly; the factor again; solve.
//   the record   the entries with (T) z_e > 0, in record order, compacted to the front of idx and val (z_e rounded once to T), zero
//                words from there to K, K' in word 0; every other word as it was.
// LASSO ORDER (k_rf_lasso; G, h and y^T y are the words above, everything below in double, products and sums rounded separately; lam =
// lam_b, g_e = sqrt(G_ee), one root each):
//   state        the NNLS state, and sigma by record position: the sign, +1 or -1, a member of P entered with.  L is the factor of
//                (G + ridge diag G)_PP in P's order, u = L^-1 (h_P - lam g_P sigma_P).  Start P empty, z = 0.
//   entry test   for every position e not in P with G_ee > 0:  w_e as NNLS forms it (w_e = h_e, then w_e = w_e - G_ei * z_i, ascending i
//                over P's members by record position),  v_e = |w_e| / g_e - lam (one quotient, one difference).  tau = 8 K eps(T)
//                sqrt(y^T y) (one root, one product).  Among the e with v_e > tau the largest v_e enters, ties to the smallest position;
//                none: the signal is done.  sigma_e = +1 when w_e > 0, else -1.  (A comparison, so a NaN never enters.)
//   factor row   NNLS' `row p` with the pivot's start d = G_jj * (1 + ridge) (1 + ridge formed once; one product) and the right-hand
//                side's start c = h_j - (lam * g_j) * sigma_j; the v_i are G's words (the ridge sits on the diagonal alone).  The
//                signal is SINGULAR when !(d > 8 K eps(T) (G_jj * (1 + ridge))).  After a removal the rows 0, 1, ... of the shortened
//                list are formed again by the same statements, the substituted right-hand side with them.
//   a solve      NNLS' statements.  At most 3 K solves a signal; one more needed: SS_HIP_REFIT_STALLED.
//   inner loop   every sigma_p * s_p > 0: z_P = s, back to the entry test.  Else over the p with !(sigma_p * s_p > 0) in P's order
//                a_p = z_p / (z_p - s_p) (0 where !(sigma_p * z_p > 0): a column that has just entered), alpha = their minimum,
//                attained first at p*;  z_p = z_p + alpha * (s_p - z_p) for every p;  p* and every p with !(sigma_p * z_p > 0) leave P
//                with z = 0 exactly and their sign forgotten (they may return with either); the factor again; solve.
//   the record   as k_rf_nnls writes it, the kept entries being those with (T) z_e != 0.
// PRUNE ORDER (k_rf_prune; G, h, y^T y and z are the words above — z in double, before it is rounded; everything below in double,
// every product, sum and quotient rounded separately):
//   inverse      (rule BACKWARD) M = L^-1, row after row over the factor, in place: for i ascending  M_ii = 1 / l_ii,  and for every
//                e < i  s = 0, then s = s + l_ik * M_ke for k ascending from e to i - 1,  M_ie = (-s) / l_ii.  The columns e of a
//                row are independent of each other: a workgroup barrier separates rows, never the terms of a sum;
//   q_e          = 0, then q_e = q_e + M_ie * M_ie for i ascending from e to K - 1: the diagonal of (G_T)^-1;
//   score_e      MAGNITUDE (z_e * z_e) * G_ee with G_ee the diagonal before any update;  BACKWARD (z_e * z_e) / q_e;
//   candidates   the e with score_e >= min_share * y^T y (one product; a comparison, so a NaN never passes);
//   kept         the min(keep, candidates) candidates that come first by (score descending, record position ascending): entry e is
//                kept when fewer than `keep` candidates come before it — a count of comparisons, no sort;
//   all kept     the record is ss_hip_refit_records_*' record: val[e] = z_e rounded once to T;
//   else         [G h; h^T .] of the kept entries, in record order, is summed again from the chunk partials (`G, h` above: the
//                Cholesky has overwritten the triangle) and solved by the statements above with K' in the pivot test;
//   the record   as k_rf_nnls writes it: the kept entries in record order, compacted to the front of idx and val (z rounded once
//                to T), zero words from there to K, K' in word 0; every other word as it was.
// No floating-point atomics; nothing depends on B, on the chunking of the batch, on the launch geometry, on where the pointers live or
// on what the context did before: a signal's record, residual norm and status are a function of its input record, its y and A.
#include "ss_hip_internal.h"
#include "record_common.h"
#include "tri_decode.h"

#include <algorithm>
#include <cmath>
#include <limits>

namespace sship {

namespace {

constexpr uint32_t kRfRows = 1024;                       // rows of a row chunk (a function of nothing: the split depends on m alone)
constexpr uint32_t kRfStep = 32;                         // rows staged through LDS at a time
constexpr uint32_t kRfChunkMax = 1024;                   // most signals per internal chunk ...
constexpr size_t kRfChunkBytes = (size_t)256 << 20;      // ... and the byte budget of a chunk's partials (never changes a result)

typedef float rf_v4f __attribute__((ext_vector_type(4)));
typedef double rf_v4d __attribute__((ext_vector_type(4)));
typedef double rf_v2d __attribute__((ext_vector_type(2)));

// the 16 x 16 x 4 MFMA of T: operands one element a lane (row / column lane & 15, k = lane >> 4), four results a lane at column
// lane & 15 and row `row(e, lane)`; slot(ri, cj) = where element (ri, cj) of a tile sits among a wave's 4 x 64 results
template <typename T> struct RfMma;
template <> struct RfMma<float> {
    typedef rf_v4f Acc;
    typedef rf_v4f V;
    static constexpr uint32_t W = 4;
    __device__ static Acc mma(float a, float b, Acc c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
    __device__ static uint32_t slot(uint32_t ri, uint32_t cj) { return (ri & 3u) * 64u + (ri >> 2) * 16u + cj; }
};
template <> struct RfMma<double> {
    typedef rf_v4d Acc;
    typedef rf_v2d V;
    static constexpr uint32_t W = 2;
    __device__ static Acc mma(double a, double b, Acc c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
    __device__ static uint32_t slot(uint32_t ri, uint32_t cj) { return (ri >> 2) * 64u + (ri & 3u) * 16u + cj; }
};

struct RefitState {
    WorkArena batch;                   // per call: staged records (a host caller's), status, residual norms, the bad-index word
    WorkArena arena;                   // per chunk of signals: the Gram partials, a host caller's signals
};

RefitState* state_of(ss_hip_ctx* ctx)
{
    return &part<RefitState>(ctx->rf);
}

// tile rows of the panel of a record with K stored columns (+ the column of y)
__host__ __device__ inline uint32_t rf_tile_rows(uint32_t K) { return (K + 16u) / 16u; }

// ---- kernels -------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(64)
void k_rf_check(const unsigned char* __restrict__ rec, size_t rb, uint32_t kmax, uint32_t n, uint32_t* __restrict__ stat,
                uint32_t* __restrict__ bad)
{
    const uint32_t b = blockIdx.x;
    const unsigned char* r = rec + (size_t)b * rb;
    const uint32_t Krec = *reinterpret_cast<const uint32_t*>(r);
    rec_check_indices(r, Krec, kmax, n, b, bad);
    if (threadIdx.x == 0)
        stat[b] = Krec == 0u ? (uint32_t)SS_HIP_REFIT_EMPTY : Krec > kmax ? (uint32_t)SS_HIP_REFIT_TRUNCATED
                  : Krec > (uint32_t)SS_HIP_REFIT_KMAX ? (uint32_t)SS_HIP_REFIT_TOO_LARGE : (uint32_t)SS_HIP_REFIT_DONE;
}

// NT: the most tile rows a panel of this call can have (from min(kmax, SS_HIP_REFIT_KMAX)); a wave holds up to NTW tiles.
// part: [signal][chunk][tile_cap tiles][4 results][64 lanes], tile t = ti (ti + 1) / 2 + tj with tj <= ti
// WGT (the weighted refit, weighted.hip): P^T W_b P.  The stage's 32 weights (row b of W; 0 for the rows m .. ldm - 1) sit in LDS in
// front of the panel, and ONE operand — the tile-row operand, the one that holds h's row — is multiplied by w_k in T as a lane
// reads it: element (i, j) is the chain of fma(P[r][i] * w_r, P[r][j], .), the panel, tiles and order unchanged.  With w_r == 1
// the product is P[r][i] itself: the unweighted kernel's words.  Without WGT nothing is added and W is not read.
template <typename T, int NT, bool WGT = false>
__global__ __launch_bounds__(256)
void k_rf_gram(const T* __restrict__ At, uint32_t ldm, uint32_t m, const T* __restrict__ Y, long long y_stride, long long incy,
               const unsigned char* __restrict__ rec, size_t rb, const uint32_t* __restrict__ stat, T* __restrict__ part, uint32_t tile_cap,
               const T* __restrict__ Wt = nullptr, long long w_stride = 0)
{
    typedef RfMma<T> M;
    typedef typename M::V V;
    typedef typename M::Acc Acc;
    constexpr uint32_t W = M::W, VPC = kRfStep / W, PITCH = kRfStep + W;
    constexpr int NTW = (NT * (NT + 1) / 2 + 3) / 4;
    constexpr int NV = (NT * 16 * (int)VPC + 255) / 256;
    extern __shared__ __align__(16) unsigned char s_rf_raw[];
    T* sW = reinterpret_cast<T*>(s_rf_raw);                  // WGT: [kRfStep] the stage's weights
    T* sP = sW + (WGT ? kRfStep : 0u);                       // [ncol][PITCH]: column c of the panel, the stage's 32 rows
    const uint32_t chunk = blockIdx.x, b = blockIdx.y, nchunks = gridDim.x;
    if (stat[b] != (uint32_t)SS_HIP_REFIT_DONE) return;
    const unsigned char* r = rec + (size_t)b * rb;
    const uint32_t K = *reinterpret_cast<const uint32_t*>(r);
    const uint32_t* idx = reinterpret_cast<const uint32_t*>(r + 16);
    const uint32_t nt = rf_tile_rows(K), ntile = nt * (nt + 1u) / 2u, ncol = nt * 16u;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, l15 = lane & 15u, kq = lane >> 4;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t row_lo = chunk * kRfRows, row_hi = row_lo + kRfRows < ldm ? row_lo + kRfRows : ldm;
    const T* y = Y + (long long)b * y_stride;

    for (uint32_t i = tid; i < ncol * PITCH; i += 256u) sP[i] = T(0);       // (the padding columns stay zero)

    // staging slots: vector v = tid + 256 s is rows q W .. q W + W - 1 of the stage, column c = v / VPC
    const T* cp[NV];
    uint32_t kind[NV], soff[NV], srow[NV];                   // kind: 0 nothing, 1 a column of A, 2 the signal
#pragma unroll
    for (int s = 0; s < NV; ++s) {
        const uint32_t v = tid + 256u * (uint32_t)s, c = v / VPC, q = (v % VPC) * W;
        kind[s] = c < K ? 1u : c == K ? 2u : 0u;
        cp[s] = At + (size_t)(c < K ? idx[c] : 0u) * ldm + q;
        soff[s] = c * PITCH + q;
        srow[s] = q;
    }
    V vr[NV];
    T wr = T(0);                                             // WGT: thread t < 32 stages the weight of row t of the stage
    const T* wrow = Wt + (long long)b * w_stride;
#define RF_LOAD(R0)                                                                                    \
    _Pragma("unroll") for (int s = 0; s < NV; ++s) {                                                   \
        if (kind[s] == 1u) vr[s] = *reinterpret_cast<const V*>(cp[s] + (R0));                          \
        else if (kind[s] == 2u) {                                                                      \
            _Pragma("unroll") for (uint32_t e = 0; e < W; ++e) {                                       \
                const uint32_t row = (R0) + srow[s] + e;                                               \
                vr[s][e] = row < m ? y[(long long)row * incy] : T(0);                                  \
            }                                                                                          \
        }                                                                                              \
    }                                                                                                  \
    if (WGT && tid < kRfStep) wr = (R0) + tid < m ? wrow[(R0) + tid] : T(0);
    RF_LOAD(row_lo)

    // this wave's tiles t = wave, wave + 4, ...: where a lane reads its two operands
    bool mine[NTW];
    uint32_t offa[NTW], offb[NTW];
    Acc acc[NTW];
#pragma unroll
    for (int s = 0; s < NTW; ++s) {
        const uint32_t t = wave + 4u * (uint32_t)s;
        mine[s] = t < ntile;
        uint32_t tj = 0, ti = 0;
        tri_tile_decode(mine[s] ? t : 0u, tj, ti);
        offa[s] = (ti * 16u + l15) * PITCH + kq;
        offb[s] = (tj * 16u + l15) * PITCH + kq;
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[s][e] = T(0);
    }

    for (uint32_t r0 = row_lo; r0 < row_hi; r0 += kRfStep) {
        __syncthreads();
#pragma unroll
        for (int s = 0; s < NV; ++s)
            if (kind[s] != 0u) *reinterpret_cast<V*>(&sP[soff[s]]) = vr[s];
        if (WGT && tid < kRfStep) sW[tid] = wr;
        __syncthreads();
        if (r0 + kRfStep < row_hi) { RF_LOAD(r0 + kRfStep) }
#pragma unroll
        for (int s = 0; s < NTW; ++s) {
            if (!mine[s]) continue;
#pragma unroll
            for (uint32_t k4 = 0; k4 < kRfStep; k4 += 4u) {
                if constexpr (WGT) acc[s] = M::mma(sP[offa[s] + k4] * sW[kq + k4], sP[offb[s] + k4], acc[s]);
                else acc[s] = M::mma(sP[offa[s] + k4], sP[offb[s] + k4], acc[s]);
            }
        }
    }
#undef RF_LOAD
    T* pp = part + ((size_t)b * nchunks + chunk) * tile_cap * 256u;
#pragma unroll
    for (int s = 0; s < NTW; ++s) {
        if (!mine[s]) continue;
        const uint32_t t = wave + 4u * (uint32_t)s;
#pragma unroll
        for (int e = 0; e < 4; ++e) pp[(size_t)t * 256u + (uint32_t)e * 64u + lane] = acc[s][e];
    }
}

// element (i, j), i >= j, of a signal's [G h; h^T y^T y] (pb: its partials): the chunk partials in ascending order, in double
// (SUMMATION ORDER: `G, h`)
template <typename T>
__device__ inline double rf_panel_word(const T* __restrict__ pb, uint32_t nchunks, uint32_t tile_cap, uint32_t i, uint32_t j)
{
    const size_t cstride = (size_t)tile_cap * 256u;
    const uint32_t ti = i >> 4, tj = j >> 4, t = ti * (ti + 1u) / 2u + tj;
    const T* pp = pb + (size_t)t * 256u + RfMma<T>::slot(i & 15u, j & 15u);
    double s = 0.0;
    for (uint32_t c = 0; c < nchunks; ++c) s += (double)pp[(size_t)c * cstride];
    return s;
}

// The solve of one signal's normal equations (SUMMATION ORDER: Cholesky, pivot test, back subst.) on the packed rows 0 .. K of
// [G h; h^T .] in LDS, (i, j) at i (i + 1) / 2 + j, written and made visible by the caller; g0: [K] for the diagonal before any update.
// Every thread of the workgroup calls it and gets the same verdict: false = the pivot test failed; true: row K holds z in double, the
// rows above it the factor.  T names the eps of the pivot test.
template <typename T>
__device__ inline bool rf_factor_solve(double* L, double* g0, uint32_t K)
{
    const uint32_t tid = threadIdx.x, KB = K * (K + 1u) / 2u;
    for (uint32_t j = tid; j < K; j += 256u) g0[j] = L[j * (j + 1u) / 2u + j];
    __syncthreads();
    const double thr = 8.0 * (double)K * (double)std::numeric_limits<T>::epsilon();
    for (uint32_t j = 0; j < K; ++j) {
        const uint32_t jj = j * (j + 1u) / 2u + j;
        const double d = L[jj];                              // (every thread reads the same word: the branch is uniform)
        if (!(d > thr * g0[j])) return false;
        const double ljj = sqrt(d);
        __syncthreads();
        for (uint32_t i = j + 1u + tid; i <= K; i += 256u) { const uint32_t ij = i * (i + 1u) / 2u + j; L[ij] = L[ij] / ljj; }
        if (tid == 0) L[jj] = ljj;
        __syncthreads();
        for (uint32_t i = j + 1u + tid; i <= K; i += 256u) {
            const uint32_t ib = i * (i + 1u) / 2u, kend = i < K ? i : K - 1u;
            const double lij = L[ib + j];
            for (uint32_t k = j + 1u; k <= kend; ++k) L[ib + k] = L[ib + k] - lij * L[k * (k + 1u) / 2u + j];
        }
        __syncthreads();
    }
    for (uint32_t j = K; j-- > 0u;) {
        const uint32_t jb = j * (j + 1u) / 2u;
        __syncthreads();
        const double zj = L[KB + j] / L[jb + j];
        __syncthreads();
        if (tid == 0) L[KB + j] = zj;
        for (uint32_t i = tid; i < j; i += 256u) L[KB + i] = L[KB + i] - L[jb + i] * zj;
    }
    __syncthreads();
    return true;
}

// rec_in and rec_out: the same records (in place) or disjoint ones
template <typename T>
__global__ __launch_bounds__(256)
void k_rf_solve(const T* __restrict__ part, uint32_t nchunks, uint32_t tile_cap, const unsigned char* rec_in, unsigned char* rec_out,
                size_t rb, uint32_t kmax, uint32_t* __restrict__ stat)
{
    extern __shared__ __align__(16) unsigned char s_rf_raw[];
    double* L = reinterpret_cast<double*>(s_rf_raw);         // packed rows 0 .. K of [G h; h^T .]: (i, j) at i (i + 1) / 2 + j
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    const unsigned char* ri = rec_in + (size_t)b * rb;
    unsigned char* ro = rec_out + (size_t)b * rb;
    const uint32_t* wi = reinterpret_cast<const uint32_t*>(ri);
    uint32_t* wo = reinterpret_cast<uint32_t*>(ro);
    const uint32_t words = (uint32_t)(rb / 4);
    if (stat[b] != (uint32_t)SS_HIP_REFIT_DONE) {
        if (ri != ro)
            for (uint32_t w = tid; w < words; w += 256u) wo[w] = wi[w];
        return;
    }
    const uint32_t K = wi[0], np = (K + 1u) * (K + 2u) / 2u, KB = K * (K + 1u) / 2u;
    const T* pb = part + (size_t)b * nchunks * tile_cap * 256u;
    for (uint32_t p = tid; p < np; p += 256u) {
        uint32_t j = 0, i = 0;
        tri_tile_decode(p, j, i);
        L[p] = rf_panel_word<T>(pb, nchunks, tile_cap, i, j);
    }
    __syncthreads();
    if (!rf_factor_solve<T>(L, L + np, K)) {
        if (tid == 0) stat[b] = (uint32_t)SS_HIP_REFIT_SINGULAR;
        if (ri != ro)
            for (uint32_t w = tid; w < words; w += 256u) wo[w] = wi[w];
        return;
    }
    // everything but val[0 .. K) word for word, then the fit
    const uint32_t v0 = 4u + kmax, v1 = v0 + K * (uint32_t)(sizeof(T) / 4);
    if (ri != ro)
        for (uint32_t w = tid; w < words; w += 256u)
            if (w < v0 || w >= v1) wo[w] = wi[w];
    unsigned char* valp = ro + 16 + (size_t)kmax * 4;
    for (uint32_t e = tid; e < K; e += 256u) store_val(valp, e, (T)L[KB + e]);
}

// the non-negative refit (nonneg.hip): a DONE record of more than `cap` columns does not fit k_rf_nnls' LDS
__global__ __launch_bounds__(256)
void k_rf_cap(const unsigned char* __restrict__ rec, size_t rb, uint32_t cap, uint32_t* __restrict__ stat, uint32_t B)
{
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= B) return;
    if (stat[b] == (uint32_t)SS_HIP_REFIT_DONE && *reinterpret_cast<const uint32_t*>(rec + (size_t)b * rb) > cap)
        stat[b] = (uint32_t)SS_HIP_REFIT_TOO_LARGE;
}

// element (a, b) of the packed lower triangle of a symmetric matrix, whichever way round
__device__ inline uint32_t rf_tri(uint32_t a, uint32_t b) { return a >= b ? a * (a + 1u) / 2u + b : b * (b + 1u) / 2u + a; }

// One row of the Cholesky factor of G_PP (P in entry order, plist[0 .. p]): row p from column j = plist[p], with the forward
// substitution of h along (u[p]).  Every thread of the workgroup calls it and gets the same verdict: false = the pivot failed.
// (NNLS ORDER in the header: `row p`.)  gjj: the row's diagonal before any update, cj: its right-hand side — G_jj and h_j for the
// non-negative refit, G_jj (1 + ridge) and h_j - lam g_j sigma_j for the l1 refit (LASSO ORDER: `factor row`).
__device__ inline bool rf_nn_row(const double* G, double* Lf, double* v, double* u, const uint32_t* plist, uint32_t p, double gjj, double cj, double thr)
{
    const uint32_t tid = threadIdx.x, j = plist[p], pb = p * (p + 1u) / 2u;
    __syncthreads();
    for (uint32_t i = tid; i < p; i += 256u) v[i] = G[rf_tri(j, plist[i])];
    double d = gjj, c = cj;
    for (uint32_t k = 0; k < p; ++k) {
        __syncthreads();
        const double lk = v[k] / Lf[k * (k + 1u) / 2u + k];      // (every thread forms the same word)
        for (uint32_t i = k + 1u + tid; i < p; i += 256u) v[i] = v[i] - Lf[i * (i + 1u) / 2u + k] * lk;
        if (tid == 0) Lf[pb + k] = lk;
        d = d - lk * lk;
        c = c - lk * u[k];
    }
    if (!(d > thr * gjj)) return false;
    const double lpp = sqrt(d);
    if (tid == 0) { Lf[pb + p] = lpp; u[p] = c / lpp; }
    __syncthreads();
    return true;
}

// The non-negative refit of one signal (ss_hip_nonneg_refit_records_*, nonneg.hip): Lawson-Hanson on the normal equations that
// k_rf_gram formed, in double, in LDS — the packed [G h; h^T y^T y], the packed Cholesky factor of G_PP beside it, a few vectors of
// K.  One workgroup per signal; every decision is taken by every thread from the same LDS words, so every branch is uniform.
// rec_in and rec_out: the same records (in place) or disjoint ones.  (NNLS ORDER in the header.)
template <typename T>
__global__ __launch_bounds__(256)
void k_rf_nnls(const T* __restrict__ part, uint32_t nchunks, uint32_t tile_cap, const unsigned char* rec_in, unsigned char* rec_out, size_t rb,
               uint32_t kmax, uint32_t* __restrict__ stat, uint32_t* __restrict__ dropped)
{
    extern __shared__ __align__(16) unsigned char s_rf_raw[];
    __shared__ uint32_t s_bad, s_np;
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    const unsigned char* ri = rec_in + (size_t)b * rb;
    unsigned char* ro = rec_out + (size_t)b * rb;
    const uint32_t* wi = reinterpret_cast<const uint32_t*>(ri);
    uint32_t* wo = reinterpret_cast<uint32_t*>(ro);
    const uint32_t words = (uint32_t)(rb / 4);
    // every status but DONE: the record unchanged, nothing dropped
    auto unchanged = [&](uint32_t status) {
        if (tid == 0) { stat[b] = status; dropped[b] = 0u; }
        if (ri != ro)
            for (uint32_t w = tid; w < words; w += 256u) wo[w] = wi[w];
    };
    if (stat[b] != (uint32_t)SS_HIP_REFIT_DONE) { unchanged(stat[b]); return; }
    const uint32_t K = wi[0], np = (K + 1u) * (K + 2u) / 2u, KB = K * (K + 1u) / 2u;
    double* G = reinterpret_cast<double*>(s_rf_raw);         // packed rows 0 .. K of [G h; h^T y^T y]: (i, j) at i (i + 1) / 2 + j
    double* Lf = G + np;                                     // packed rows of the factor of G_PP, row p at p (p + 1) / 2
    double* z = Lf + KB;                                     // [K] by record position, 0 outside P
    double* s = z + K;                                       // [K] by position in P: the solution of a solve
    double* v = s + K;                                       // [K] workspace: w of the entry test, a substitution's right-hand side
    double* u = v + K;                                       // [K] by position in P: h_P taken through the forward substitution
    uint32_t* plist = reinterpret_cast<uint32_t*>(u + K);    // [K] P in entry order (record positions)
    uint32_t* inP = plist + K;                               // [K] by record position
    uint32_t* sidx = inP + K;                                // [K] the record's columns; then the output slot of a kept entry
    const T* pb = part + (size_t)b * nchunks * tile_cap * 256u;
    for (uint32_t p = tid; p < np; p += 256u) {              // (k_rf_solve's words)
        uint32_t j = 0, i = 0;
        tri_tile_decode(p, j, i);
        G[p] = rf_panel_word<T>(pb, nchunks, tile_cap, i, j);
    }
    if (tid == 0) s_bad = 0u;
    for (uint32_t e = tid; e < K; e += 256u) { z[e] = 0.0; inP[e] = 0u; sidx[e] = wi[4u + e]; }
    __syncthreads();
    const double kDblMax = 1.7976931348623157e308;
    for (uint32_t e = tid; e <= K; e += 256u)                // (e == K: y^T y)
        if (!(fabs(G[e * (e + 1u) / 2u + e]) <= kDblMax) || !(fabs(G[KB + e]) <= kDblMax)) atomicOr(&s_bad, 1u);
    __syncthreads();
    if (s_bad != 0u) { unchanged((uint32_t)SS_HIP_REFIT_SINGULAR); return; }
    const double thr = 8.0 * (double)K * (double)std::numeric_limits<T>::epsilon(), yy = G[KB + K];
    // row p of the factor of G_PP: the diagonal G_jj, the right-hand side h_j
    auto row = [&](uint32_t p) { const uint32_t j = plist[p]; return rf_nn_row(G, Lf, v, u, plist, p, G[j * (j + 1u) / 2u + j], G[KB + j], thr); };
    uint32_t nP = 0, solves = 0, verdict = (uint32_t)SS_HIP_REFIT_DONE;
    for (;;) {
        // ---- the entry test: w over the columns not in P, the largest w_j above its threshold ----
        __syncthreads();
        for (uint32_t e = tid; e < K; e += 256u) {
            if (inP[e]) continue;
            double a = G[KB + e];
            for (uint32_t i = 0; i < K; ++i)
                if (inP[i]) a = a - G[rf_tri(e, i)] * z[i];
            v[e] = a;
        }
        __syncthreads();
        uint32_t best = K;
        double bw = 0.0;
        for (uint32_t e = 0; e < K; ++e) {
            if (inP[e]) continue;
            const double w = v[e], tau = thr * sqrt(G[e * (e + 1u) / 2u + e] * yy);
            if (w > tau && (best == K || w > bw)) { best = e; bw = w; }
        }
        if (best == K) break;
        __syncthreads();
        if (tid == 0) { plist[nP] = best; inP[best] = 1u; }
        __syncthreads();
        if (!row(nP)) { verdict = (uint32_t)SS_HIP_REFIT_SINGULAR; break; }
        nP += 1u;
        // ---- the inner loop: solve on P, step towards the solution as far as z stays non-negative, drop what reaches zero ----
        while (nP != 0u) {
            if (solves == 3u * K) { verdict = (uint32_t)SS_HIP_REFIT_STALLED; break; }
            solves += 1u;
            for (uint32_t i = tid; i < nP; i += 256u) v[i] = u[i];
            for (uint32_t k = nP; k-- > 0u;) {
                const uint32_t kb = k * (k + 1u) / 2u;
                __syncthreads();
                const double sk = v[k] / Lf[kb + k];
                for (uint32_t i = tid; i < k; i += 256u) v[i] = v[i] - Lf[kb + i] * sk;
                if (tid == 0) s[k] = sk;
            }
            __syncthreads();
            bool all_pos = true;
            double alpha = 0.0;
            uint32_t pmin = K;
            for (uint32_t p = 0; p < nP; ++p) {
                const double sp = s[p];
                if (sp > 0.0) continue;
                all_pos = false;
                const double zp = z[plist[p]], a = zp > 0.0 ? zp / (zp - sp) : 0.0;
                if (pmin == K || a < alpha) { alpha = a; pmin = p; }
            }
            if (all_pos) {
                for (uint32_t p = tid; p < nP; p += 256u) z[plist[p]] = s[p];
                break;
            }
            __syncthreads();
            for (uint32_t p = tid; p < nP; p += 256u) {
                const uint32_t e = plist[p];
                const double zn = z[e] + alpha * (s[p] - z[e]);
                if (p == pmin || !(zn > 0.0)) { z[e] = 0.0; inP[e] = 0u; }
                else z[e] = zn;
            }
            __syncthreads();
            // P without what left, in its order; the factor built again row by row
            if (tid == 0) {
                uint32_t kept = 0;
                for (uint32_t p = 0; p < nP; ++p) {
                    const uint32_t e = plist[p];
                    if (inP[e]) plist[kept++] = e;
                }
                s_np = kept;
            }
            __syncthreads();
            nP = s_np;
            bool ok = true;
            for (uint32_t p = 0; p < nP && ok; ++p) ok = row(p);
            if (!ok) { verdict = (uint32_t)SS_HIP_REFIT_SINGULAR; break; }
        }
        if (verdict != (uint32_t)SS_HIP_REFIT_DONE) break;
    }
    __syncthreads();
    if (verdict != (uint32_t)SS_HIP_REFIT_DONE) { unchanged(verdict); return; }
    // ---- the record: the entries with (T) z_e > 0 in record order, zero words up to K, everything else word for word ----
    if (tid == 0) {
        uint32_t kept = 0;
        for (uint32_t e = 0; e < K; ++e) {
            const bool keep = (T)z[e] > T(0);
            inP[e] = keep ? kept : K;                        // the output slot, K = dropped
            kept += keep ? 1u : 0u;
        }
        s_bad = kept;
    }
    __syncthreads();
    const uint32_t Kp = s_bad;
    const uint32_t v0 = 4u + kmax, v1 = v0 + K * (uint32_t)(sizeof(T) / 4);
    if (ri != ro)
        for (uint32_t w = tid; w < words; w += 256u)
            if (w != 0u && (w < 4u || (w >= 4u + K && w < v0) || w >= v1)) wo[w] = wi[w];
    unsigned char* valp = ro + 16 + (size_t)kmax * 4;
    for (uint32_t e = tid; e < K; e += 256u) {
        if (inP[e] != K) { wo[4u + inP[e]] = sidx[e]; store_val(valp, inP[e], (T)z[e]); }
        if (e >= Kp) { wo[4u + e] = 0u; store_val(valp, e, T(0)); }
    }
    if (tid == 0) { wo[0] = Kp; dropped[b] = K - Kp; }
}

// the l1 refit (lasso.hip): lam[b] = src[b * stride] for the kernels, whichever side the caller's lam was on (a host caller's is staged
// in front); a lam_b that is negative or not finite puts b into *bad — the records' flag word beside the index check's
__global__ __launch_bounds__(256)
void k_rf_lam(const double* __restrict__ src, long long stride, double* __restrict__ lam, uint32_t* __restrict__ bad, uint32_t B)
{
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= B) return;
    const double l = src[(long long)b * stride];
    if (!(l >= 0.0 && l <= 1.7976931348623157e308)) atomicMin(bad, b);
    lam[b] = l;
}

// The l1 refit of one signal (ss_hip_lasso_refit_records_*, lasso.hip): k_rf_nnls with a sign and a penalty on the normal equations
// that k_rf_gram formed, in double, in LDS — k_rf_nnls' block and two more vectors of K (the signs, g_e = sqrt(G_ee)).  One workgroup per
// signal; every decision is taken by every thread from the same LDS words, so every branch is uniform.  lam: the chunk's lam_b on the
// device (checked: k_rf_lam).  rec_in and rec_out: the same records (in place) or disjoint ones.  (LASSO ORDER in the header.)
template <typename T>
__global__ __launch_bounds__(256)
void k_rf_lasso(const T* __restrict__ part, uint32_t nchunks, uint32_t tile_cap, const unsigned char* rec_in, unsigned char* rec_out, size_t rb,
                uint32_t kmax, uint32_t* __restrict__ stat, uint32_t* __restrict__ dropped, const double* __restrict__ lam, double ridge)
{
    extern __shared__ __align__(16) unsigned char s_rf_raw[];
    __shared__ uint32_t s_bad, s_np;
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    const unsigned char* ri = rec_in + (size_t)b * rb;
    unsigned char* ro = rec_out + (size_t)b * rb;
    const uint32_t* wi = reinterpret_cast<const uint32_t*>(ri);
    uint32_t* wo = reinterpret_cast<uint32_t*>(ro);
    const uint32_t words = (uint32_t)(rb / 4);
    // every status but DONE: the record unchanged, nothing dropped
    auto unchanged = [&](uint32_t status) {
        if (tid == 0) { stat[b] = status; dropped[b] = 0u; }
        if (ri != ro)
            for (uint32_t w = tid; w < words; w += 256u) wo[w] = wi[w];
    };
    if (stat[b] != (uint32_t)SS_HIP_REFIT_DONE) { unchanged(stat[b]); return; }
    const uint32_t K = wi[0], np = (K + 1u) * (K + 2u) / 2u, KB = K * (K + 1u) / 2u;
    double* G = reinterpret_cast<double*>(s_rf_raw);         // packed rows 0 .. K of [G h; h^T y^T y]: (i, j) at i (i + 1) / 2 + j
    double* Lf = G + np;                                     // packed rows of the factor of (G + ridge diag G)_PP, row p at p (p + 1) / 2
    double* z = Lf + KB;                                     // [K] by record position, 0 outside P
    double* s = z + K;                                       // [K] by position in P: the solution of a solve
    double* v = s + K;                                       // [K] workspace: w of the entry test, a substitution's right-hand side
    double* u = v + K;                                       // [K] by position in P: the right-hand side taken through the forward substitution
    double* sg = u + K;                                      // [K] by record position: the sign a member of P entered with, +1 or -1
    double* gd = sg + K;                                     // [K] by record position: g_e = sqrt(G_ee)
    uint32_t* plist = reinterpret_cast<uint32_t*>(gd + K);   // [K] P in entry order (record positions)
    uint32_t* inP = plist + K;                               // [K] by record position
    uint32_t* sidx = inP + K;                                // [K] the record's columns; then the output slot of a kept entry
    const T* pb = part + (size_t)b * nchunks * tile_cap * 256u;
    for (uint32_t p = tid; p < np; p += 256u) {              // (k_rf_solve's words)
        uint32_t j = 0, i = 0;
        tri_tile_decode(p, j, i);
        G[p] = rf_panel_word<T>(pb, nchunks, tile_cap, i, j);
    }
    if (tid == 0) s_bad = 0u;
    for (uint32_t e = tid; e < K; e += 256u) { z[e] = 0.0; sg[e] = 0.0; inP[e] = 0u; sidx[e] = wi[4u + e]; }
    __syncthreads();
    const double kDblMax = 1.7976931348623157e308;
    for (uint32_t e = tid; e <= K; e += 256u) {              // (e == K: y^T y)
        const double gee = G[e * (e + 1u) / 2u + e];
        if (!(fabs(gee) <= kDblMax) || !(fabs(G[KB + e]) <= kDblMax)) atomicOr(&s_bad, 1u);
        if (e < K) gd[e] = sqrt(gee);
    }
    __syncthreads();
    if (s_bad != 0u) { unchanged((uint32_t)SS_HIP_REFIT_SINGULAR); return; }
    const double thr = 8.0 * (double)K * (double)std::numeric_limits<T>::epsilon(), tau = thr * sqrt(G[KB + K]);
    const double lb = lam[b], rp1 = 1.0 + ridge;
    // row p of the factor of (G + ridge diag G)_PP: the diagonal G_jj (1 + ridge), the right-hand side h_j - lam g_j sigma_j
    auto row = [&](uint32_t p) {
        const uint32_t j = plist[p];
        return rf_nn_row(G, Lf, v, u, plist, p, G[j * (j + 1u) / 2u + j] * rp1, G[KB + j] - (lb * gd[j]) * sg[j], thr);
    };
    uint32_t nP = 0, solves = 0, verdict = (uint32_t)SS_HIP_REFIT_DONE;
    for (;;) {
        // ---- 1. the entry test: w over the positions not in P, the largest |w_e| / g_e - lam above tau ----
        __syncthreads();
        for (uint32_t e = tid; e < K; e += 256u) {
            if (inP[e]) continue;
            double a = G[KB + e];
            for (uint32_t i = 0; i < K; ++i)
                if (inP[i]) a = a - G[rf_tri(e, i)] * z[i];
            v[e] = a;
        }
        __syncthreads();
        uint32_t best = K;
        double bv = 0.0;
        for (uint32_t e = 0; e < K; ++e) {
            if (inP[e] || !(G[e * (e + 1u) / 2u + e] > 0.0)) continue;
            const double ve = fabs(v[e]) / gd[e] - lb;
            if (ve > tau && (best == K || ve > bv)) { best = e; bv = ve; }
        }
        if (best == K) break;
        const double sgn = v[best] > 0.0 ? 1.0 : -1.0;
        __syncthreads();
        if (tid == 0) { plist[nP] = best; inP[best] = 1u; sg[best] = sgn; }
        __syncthreads();
        // ---- 2. the factor row of the entering position ----
        if (!row(nP)) { verdict = (uint32_t)SS_HIP_REFIT_SINGULAR; break; }
        nP += 1u;
        // ---- 3. the inner loop: solve on P, step towards the solution as far as every z keeps its sign, drop what reaches zero ----
        while (nP != 0u) {
            if (solves == 3u * K) { verdict = (uint32_t)SS_HIP_REFIT_STALLED; break; }
            solves += 1u;
            for (uint32_t i = tid; i < nP; i += 256u) v[i] = u[i];
            for (uint32_t k = nP; k-- > 0u;) {
                const uint32_t kb = k * (k + 1u) / 2u;
                __syncthreads();
                const double sk = v[k] / Lf[kb + k];
                for (uint32_t i = tid; i < k; i += 256u) v[i] = v[i] - Lf[kb + i] * sk;
                if (tid == 0) s[k] = sk;
            }
            __syncthreads();
            bool all_ok = true;
            double alpha = 0.0;
            uint32_t pmin = K;
            for (uint32_t p = 0; p < nP; ++p) {
                const uint32_t e = plist[p];
                const double sp = s[p], se = sg[e];
                if (se * sp > 0.0) continue;
                all_ok = false;
                const double zp = z[e], a = se * zp > 0.0 ? zp / (zp - sp) : 0.0;
                if (pmin == K || a < alpha) { alpha = a; pmin = p; }
            }
            if (all_ok) {
                for (uint32_t p = tid; p < nP; p += 256u) z[plist[p]] = s[p];
                break;
            }
            __syncthreads();
            for (uint32_t p = tid; p < nP; p += 256u) {
                const uint32_t e = plist[p];
                const double zn = z[e] + alpha * (s[p] - z[e]);
                if (p == pmin || !(sg[e] * zn > 0.0)) { z[e] = 0.0; inP[e] = 0u; }
                else z[e] = zn;
            }
            __syncthreads();
            // P without what left, in its order; the factor and the substituted right-hand side built again row by row
            if (tid == 0) {
                uint32_t kept = 0;
                for (uint32_t p = 0; p < nP; ++p) {
                    const uint32_t e = plist[p];
                    if (inP[e]) plist[kept++] = e;
                }
                s_np = kept;
            }
            __syncthreads();
            nP = s_np;
            bool ok = true;
            for (uint32_t p = 0; p < nP && ok; ++p) ok = row(p);
            if (!ok) { verdict = (uint32_t)SS_HIP_REFIT_SINGULAR; break; }
        }
        if (verdict != (uint32_t)SS_HIP_REFIT_DONE) break;
    }
    __syncthreads();
    if (verdict != (uint32_t)SS_HIP_REFIT_DONE) { unchanged(verdict); return; }
    // ---- the record: the entries with (T) z_e != 0 in record order, zero words up to K, everything else word for word ----
    if (tid == 0) {
        uint32_t kept = 0;
        for (uint32_t e = 0; e < K; ++e) {
            const bool keep = (T)z[e] != T(0);
            inP[e] = keep ? kept : K;                        // the output slot, K = dropped
            kept += keep ? 1u : 0u;
        }
        s_bad = kept;
    }
    __syncthreads();
    const uint32_t Kp = s_bad;
    const uint32_t v0 = 4u + kmax, v1 = v0 + K * (uint32_t)(sizeof(T) / 4);
    if (ri != ro)
        for (uint32_t w = tid; w < words; w += 256u)
            if (w != 0u && (w < 4u || (w >= 4u + K && w < v0) || w >= v1)) wo[w] = wi[w];
    unsigned char* valp = ro + 16 + (size_t)kmax * 4;
    for (uint32_t e = tid; e < K; e += 256u) {
        if (inP[e] != K) { wo[4u + inP[e]] = sidx[e]; store_val(valp, inP[e], (T)z[e]); }
        if (e >= Kp) { wo[4u + e] = 0u; store_val(valp, e, T(0)); }
    }
    if (tid == 0) { wo[0] = Kp; dropped[b] = K - Kp; }
}

// what the l1 refit adds to a refit (ss_hip_lasso_refit_records_*, lasso.hip): lam on either side, read at b * lam_stride
struct RfLasso {
    const double* lam;
    ptrdiff_t lam_stride;
    double ridge;
};

// what the pruning call adds to a refit (ss_hip_prune_records_*, pursuit.hip); score: [B][kmax] on the device, or null
struct RfPrune {
    uint32_t keep, rule;
    double min_share;
    double* score;
};

// The pruning of one signal's record (ss_hip_prune_records_*, pursuit.hip): k_rf_solve's solve on the whole record, a score per
// entry, the entries to keep, k_rf_solve's solve on the kept sub-block of the same panel words, the record as k_rf_nnls writes it.
// One workgroup per signal, in double, in LDS: the packed triangle (L^-1 overwrites L in place: a second triangle does not fit),
// three vectors of K doubles and three of K words.  Thread e owns column e of L^-1 and entry e of the selection (K <= 160 < 256);
// every decision is taken by every thread from the same LDS words, so every branch is uniform.  rec_in and rec_out: the same
// records (in place) or disjoint ones.  (PRUNE ORDER in the header.)
template <typename T>
__global__ __launch_bounds__(256)
void k_rf_prune(const T* __restrict__ part, uint32_t nchunks, uint32_t tile_cap, const unsigned char* rec_in, unsigned char* rec_out, size_t rb,
                uint32_t kmax, uint32_t* __restrict__ stat, uint32_t* __restrict__ dropped, RfPrune pr)
{
    extern __shared__ __align__(16) unsigned char s_rf_raw[];
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    const unsigned char* ri = rec_in + (size_t)b * rb;
    unsigned char* ro = rec_out + (size_t)b * rb;
    const uint32_t* wi = reinterpret_cast<const uint32_t*>(ri);
    uint32_t* wo = reinterpret_cast<uint32_t*>(ro);
    const uint32_t words = (uint32_t)(rb / 4);
    double* srow = pr.score ? pr.score + (size_t)b * kmax : nullptr;
    // every status but DONE: the record unchanged, nothing dropped, a zero score row
    auto unchanged = [&](uint32_t status) {
        if (tid == 0) { stat[b] = status; dropped[b] = 0u; }
        if (srow)
            for (uint32_t e = tid; e < kmax; e += 256u) srow[e] = 0.0;
        if (ri != ro)
            for (uint32_t w = tid; w < words; w += 256u) wo[w] = wi[w];
    };
    if (stat[b] != (uint32_t)SS_HIP_REFIT_DONE) { unchanged(stat[b]); return; }
    const uint32_t K = wi[0], np = (K + 1u) * (K + 2u) / 2u, KB = K * (K + 1u) / 2u;
    double* L = reinterpret_cast<double*>(s_rf_raw);         // packed rows 0 .. K of [G h; h^T y^T y], then the factor, then L^-1
    double* g0 = L + np;                                     // [K] the diagonal before any update
    double* sc = g0 + K;                                     // [K] the scores by record position
    double* zf = sc + K;                                     // [K] z of the whole record
    uint32_t* slot = reinterpret_cast<uint32_t*>(zf + K);    // [K] by record position: kept or not, then the output slot (K = dropped)
    uint32_t* plist = slot + K;                              // [K'] the kept record positions, ascending
    uint32_t* sidx = plist + K;                              // [K] the record's columns
    const T* pb = part + (size_t)b * nchunks * tile_cap * 256u;
    for (uint32_t p = tid; p < np; p += 256u) {
        uint32_t j = 0, i = 0;
        tri_tile_decode(p, j, i);
        L[p] = rf_panel_word<T>(pb, nchunks, tile_cap, i, j);
    }
    for (uint32_t e = tid; e < K; e += 256u) sidx[e] = wi[4u + e];
    __syncthreads();
    const double cut = pr.min_share * L[KB + K];             // (y^T y: no statement of the solve writes it)
    if (!rf_factor_solve<T>(L, g0, K)) { unchanged((uint32_t)SS_HIP_REFIT_SINGULAR); return; }
    if (tid < K) zf[tid] = L[KB + tid];
    // ---- the scores ----
    if (pr.rule == (uint32_t)SS_HIP_PRUNE_BACKWARD) {
        double q = 0.0;
        for (uint32_t i = 0; i < K; ++i) {                   // row i of L^-1 from row i of L and the rows of L^-1 above it
            const uint32_t ib = i * (i + 1u) / 2u;
            const double lii = L[ib + i];
            double mv = 0.0;
            if (tid < i) {
                double s = 0.0;
                for (uint32_t k = tid; k < i; ++k) s = s + L[ib + k] * L[k * (k + 1u) / 2u + tid];
                mv = (-s) / lii;
            } else if (tid == i) {
                mv = 1.0 / lii;
            }
            __syncthreads();
            if (tid <= i) { L[ib + tid] = mv; q = q + mv * mv; }
            __syncthreads();
        }
        if (tid < K) sc[tid] = (zf[tid] * zf[tid]) / q;
    } else if (tid < K) {
        sc[tid] = (zf[tid] * zf[tid]) * g0[tid];
    }
    __syncthreads();
    // ---- the selection: entry e is kept when it is a candidate and fewer than `keep` candidates come before it ----
    if (tid < K) {
        const double se = sc[tid];
        uint32_t before = 0;
        for (uint32_t f = 0; f < K; ++f) {
            const double sf = sc[f];
            before += (sf >= cut && (sf > se || (sf == se && f < tid))) ? 1u : 0u;
        }
        slot[tid] = (se >= cut && before < pr.keep) ? 1u : 0u;
    }
    __syncthreads();
    uint32_t Kp = 0, mine = 0;                               // the kept entries, those in front of entry tid
    for (uint32_t f = 0; f < K; ++f) {
        Kp += slot[f];
        mine += f < tid ? slot[f] : 0u;
    }
    const bool kept = tid < K && slot[tid] != 0u;
    __syncthreads();
    if (tid < K) slot[tid] = kept ? mine : K;
    if (kept) plist[mine] = tid;
    __syncthreads();
    // ---- the kept sub-block: its words summed again, the same solve with K' ----
    const uint32_t KBp = Kp * (Kp + 1u) / 2u;
    if (Kp != K && Kp != 0u) {
        const uint32_t npp = (Kp + 1u) * (Kp + 2u) / 2u;
        for (uint32_t p = tid; p < npp; p += 256u) {
            uint32_t j = 0, i = 0;
            tri_tile_decode(p, j, i);
            L[p] = rf_panel_word<T>(pb, nchunks, tile_cap, i == Kp ? K : plist[i], j == Kp ? K : plist[j]);
        }
        __syncthreads();
        if (!rf_factor_solve<T>(L, L + npp, Kp)) { unchanged((uint32_t)SS_HIP_REFIT_SINGULAR); return; }
    }
    const double* z = Kp == K ? zf : L + KBp;                // by output slot
    // ---- the record: the kept entries in record order, zero words up to K, everything else word for word ----
    const uint32_t v0 = 4u + kmax, v1 = v0 + K * (uint32_t)(sizeof(T) / 4);
    if (ri != ro)
        for (uint32_t w = tid; w < words; w += 256u)
            if (w != 0u && (w < 4u || (w >= 4u + K && w < v0) || w >= v1)) wo[w] = wi[w];
    unsigned char* valp = ro + 16 + (size_t)kmax * 4;
    if (tid < K) {
        if (kept) { wo[4u + mine] = sidx[tid]; store_val(valp, mine, (T)z[mine]); }
        if (tid >= Kp) { wo[4u + tid] = 0u; store_val(valp, tid, T(0)); }
    }
    if (srow)
        for (uint32_t e = tid; e < kmax; e += 256u) srow[e] = e < K ? sc[e] : 0.0;
    if (tid == 0) { wo[0] = Kp; dropped[b] = K - Kp; }
}

template <typename T>
__global__ __launch_bounds__(256)
void k_rf_widen(const T* __restrict__ in, double* __restrict__ out, uint32_t B)
{
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b < B) out[b] = (double)in[b];
}

// ---- host side -----------------------------------------------------------------------------------------------------------------

template <typename T> size_t rf_solve_lds(uint32_t kcap) { return ((size_t)(kcap + 1) * (kcap + 2) / 2 + kcap) * sizeof(double); }

template <typename T>
bool rf_solve_attr()
{
    static const bool ok = [] {
        const bool a = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_rf_solve<T>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)rf_solve_lds<T>(SS_HIP_REFIT_KMAX)) == hipSuccess;
        if (!a) (void)hipGetLastError();
        return a;
    }();
    return ok;
}

// the non-negative refit's LDS: [G h; h^T .] and the factor of G_PP packed, four vectors of doubles and three of words
template <typename T> size_t rf_nnls_lds(uint32_t kcap)
{
    return ((size_t)(kcap + 1) * (kcap + 2) / 2 + (size_t)kcap * (kcap + 1) / 2 + 4 * (size_t)kcap) * sizeof(double) + 3 * (size_t)kcap * sizeof(uint32_t);
}

template <typename T>
bool rf_nnls_attr()
{
    static const bool ok = [] {
        const bool a = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_rf_nnls<T>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)rf_nnls_lds<T>(SS_HIP_NNLS_KMAX)) == hipSuccess;
        if (!a) (void)hipGetLastError();
        return a;
    }();
    return ok;
}

// the l1 refit's LDS: the non-negative refit's and two more vectors of doubles (the signs, the g_e)
template <typename T> size_t rf_lasso_lds(uint32_t kcap) { return rf_nnls_lds<T>(kcap) + 2 * (size_t)kcap * sizeof(double); }

template <typename T>
bool rf_lasso_attr()
{
    static const bool ok = [] {
        const bool a = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_rf_lasso<T>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)rf_lasso_lds<T>(SS_HIP_LASSO_KMAX)) == hipSuccess;
        if (!a) (void)hipGetLastError();
        return a;
    }();
    return ok;
}

// the pruning call's LDS: k_rf_solve's, two more vectors of doubles and three of words
template <typename T> size_t rf_prune_lds(uint32_t kcap) { return rf_solve_lds<T>(kcap) + 2 * (size_t)kcap * sizeof(double) + 3 * (size_t)kcap * sizeof(uint32_t); }

template <typename T>
bool rf_prune_attr()
{
    static const bool ok = [] {
        const bool a = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_rf_prune<T>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)rf_prune_lds<T>(SS_HIP_REFIT_KMAX)) == hipSuccess;
        if (!a) (void)hipGetLastError();
        return a;
    }();
    return ok;
}

// Wd: the chunk's weights on the device (row b at Wd[b * ws]), null for the unweighted refit
template <typename T, int NT>
void launch_gram(hipStream_t st, uint32_t nchunks, uint32_t Bc, uint32_t ntc, const T* At, uint32_t ldm, uint32_t m, const T* yd, long long ys,
                 long long yi, const unsigned char* recs, size_t rb, const uint32_t* stat, T* part, uint32_t tile_cap, const T* Wd, long long ws)
{
    constexpr uint32_t PITCH = kRfStep + RfMma<T>::W;
    const size_t lds = (size_t)ntc * 16u * PITCH * sizeof(T);
    if (Wd)
        hipLaunchKernelGGL((k_rf_gram<T, NT, true>), dim3(nchunks, Bc), dim3(256), lds + kRfStep * sizeof(T), st, At, ldm, m, yd, ys, yi, recs, rb,
                           stat, part, tile_cap, Wd, ws);
    else
        hipLaunchKernelGGL((k_rf_gram<T, NT>), dim3(nchunks, Bc), dim3(256), lds, st, At, ldm, m, yd, ys, yi, recs, rb, stat, part, tile_cap,
                           (const T*)nullptr, 0ll);
}

// the batch's pieces in one buffer (the staging, the per-signal outputs, the bad-index word), a chunk's in the other
template <typename T> struct RfWork {
    unsigned char* stage;
    uint32_t *stat, *bad, *drop;
    T *rn, *part, *ybuf;
    double *rnd, *score, *lam_in, *lam;
    void carve(Carver& cv, const RecordPlace& place, size_t B, bool shrinks, size_t score_elems, bool lasso)
    {
        stage = place.carve(cv);
        stat = cv.take<uint32_t>(B);
        rn = cv.take<T>(B);
        rnd = cv.take<double>(B);
        bad = cv.take<uint32_t>(2);                          // (the index check's word, the l1 refit's lam check's)
        drop = shrinks ? cv.take<uint32_t>(B) : nullptr;
        score = score_elems ? cv.take<double>(score_elems) : nullptr;
        lam_in = lasso ? cv.take<double>(B) : nullptr;       // a host caller's lam, staged
        lam = lasso ? cv.take<double>(B) : nullptr;          // lam_b by signal
    }
    void carve(Carver& cv, size_t part_elems, size_t y_elems) { part = cv.take<T>(part_elems); ybuf = y_elems ? cv.take<T>(y_elems) : nullptr; }
};

// Wd / ws: the batch's weights on the device (validated: weights_on_device), null for the unweighted refit.  nonneg: k_rf_nnls in
// k_rf_solve's place, its capacity, `dropped` (may be null) behind status.  prune (null for the refits): k_rf_prune in k_rf_solve's place,
// `dropped` as there, prune->score the caller's [B][kmax] on either side (may be null).  lasso (null for the others): k_rf_lasso in
// k_rf_solve's place, the non-negative refit's capacity and `dropped`, lasso->lam on either side, checked on the device beside the indices
template <typename T>
int refit_impl(ss_hip_ctx* ctx, const char* who, const T* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const void* records, uint32_t kmax,
               void* records_out, double* resnorm, uint32_t* status, const T* Wd, long long ws, bool nonneg, uint32_t* dropped, const RfPrune* prune,
               const RfLasso* lasso, char* err, size_t errlen)
{
    HIPCHK(hipSetDevice(ctx->device));
    RefitState* rs = state_of(ctx);
    hipStream_t st = ctx->stream;
    const size_t m = ctx->m, rb = record_bytes(kmax, sizeof(T));
    const uint32_t ldm = ctx->ldm, n = (uint32_t)ctx->n, Bu = (uint32_t)B;
    const uint32_t nchunks = (uint32_t)((m + kRfRows - 1) / kRfRows);
    static_assert(SS_HIP_LASSO_KMAX == SS_HIP_NNLS_KMAX, "k_rf_cap is launched with one capacity for both");
    const uint32_t kcap = std::min<uint32_t>(kmax, nonneg || lasso ? SS_HIP_NNLS_KMAX : SS_HIP_REFIT_KMAX), ntc = rf_tile_rows(kcap), tile_cap = ntc * (ntc + 1u) / 2u;
    RecordPlace place(records, records_out, B * rb);
    const bool y_dev = on_device(Y);
    if (lasso   ? (rf_lasso_lds<T>(kcap) > 65536 && !rf_lasso_attr<T>())
        : nonneg ? (rf_nnls_lds<T>(kcap) > 65536 && !rf_nnls_attr<T>())
        : prune ? (rf_prune_lds<T>(kcap) > 65536 && !rf_prune_attr<T>())
                : (rf_solve_lds<T>(kcap) > 65536 && !rf_solve_attr<T>())) {
        set_err(err, errlen, std::string(who) + ": the device does not give a workgroup the LDS of a support this large");
        return SS_HIP_ERUNTIME;
    }

    // ---- the batch's records where the kernels read and write them, the per-signal outputs ----
    RfWork<T> w;
    const bool shrinks = nonneg || prune || lasso;
    const size_t score_elems = prune && prune->score ? B * kmax : 0;
    grow(rs->batch, carve_into(nullptr, w, place, B, shrinks, score_elems, lasso != nullptr), "hipMalloc(refit batch)");
    carve_into(rs->batch.buf, w, place, B, shrinks, score_elems, lasso != nullptr);
    const size_t per = (size_t)nchunks * tile_cap * 256u * sizeof(T) + (y_dev ? 0 : m * sizeof(T)) + 512;
    const size_t chunk = std::min<size_t>(B, std::max<size_t>(1, std::min<size_t>(kRfChunkMax, kRfChunkBytes / per)));
    const size_t part_elems = chunk * nchunks * tile_cap * 256u, y_elems = y_dev ? 0 : chunk * m;
    grow(rs->arena, carve_into(nullptr, w, part_elems, y_elems), "hipMalloc(refit workspace)");
    carve_into(rs->arena.buf, w, part_elems, y_elems);

    place.stage_in(w.stage, st);
    flag_arm(w.bad, st, 2);
    hipLaunchKernelGGL(k_rf_check, dim3(Bu), dim3(64), 0, st, place.din, rb, kmax, n, w.stat, w.bad);
    HIPCHK(hipGetLastError());
    if (lasso) {
        const bool lam_dev = on_device(lasso->lam);
        if (!lam_dev) HIPCHK(hipMemcpyAsync(w.lam_in, lasso->lam, (lasso->lam_stride ? B : 1) * sizeof(double), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_rf_lam, dim3((Bu + 255u) / 256u), dim3(256), 0, st, lam_dev ? lasso->lam : (const double*)w.lam_in,
                           (long long)lasso->lam_stride, w.lam, w.bad + 1, Bu);
        HIPCHK(hipGetLastError());
    }
    uint32_t first_bad[2];                                    // (both words in one fetch: nothing has been written when either is set)
    flag_fetch(first_bad, w.bad, st, 2);
    if (first_bad[0] != kNoRecord) return bad_index(first_bad[0], who, err, errlen);
    if (lasso && first_bad[1] != kNoRecord) {
        set_err(err, errlen, std::string(who) + ": lam of signal " + std::to_string(first_bad[1]) + " must be finite and >= 0");
        return SS_HIP_EINVAL;
    }
    if (nonneg || lasso) {
        hipLaunchKernelGGL(k_rf_cap, dim3((Bu + 255u) / 256u), dim3(256), 0, st, place.din, rb, (uint32_t)SS_HIP_NNLS_KMAX, w.stat, Bu);
        HIPCHK(hipGetLastError());
    }

    std::vector<T> tmp;
    for (size_t b0 = 0; b0 < B; b0 += chunk) {
        const uint32_t Bc = (uint32_t)std::min(chunk, B - b0);
        const ChunkSignals<T> y = chunk_signals<T>(ctx, Y, y_stride, incy, y_dev, w.ybuf, b0, Bc, tmp);
        const T* At = static_cast<const T*>(ctx->At);
        const T* wd = Wd ? Wd + (ptrdiff_t)b0 * ws : nullptr;
        const unsigned char* recs = place.din + b0 * rb;
        if (ntc <= 3u) launch_gram<T, 3>(st, nchunks, Bc, ntc, At, ldm, (uint32_t)m, y.yd, y.ys, y.yi, recs, rb, w.stat + b0, w.part, tile_cap, wd, ws);
        else if (ntc <= 7u) launch_gram<T, 7>(st, nchunks, Bc, ntc, At, ldm, (uint32_t)m, y.yd, y.ys, y.yi, recs, rb, w.stat + b0, w.part, tile_cap, wd, ws);
        else launch_gram<T, 11>(st, nchunks, Bc, ntc, At, ldm, (uint32_t)m, y.yd, y.ys, y.yi, recs, rb, w.stat + b0, w.part, tile_cap, wd, ws);
        if (lasso)
            hipLaunchKernelGGL((k_rf_lasso<T>), dim3(Bc), dim3(256), rf_lasso_lds<T>(kcap), st, (const T*)w.part, nchunks, tile_cap, recs,
                               place.dout + b0 * rb, rb, kmax, w.stat + b0, w.drop + b0, (const double*)w.lam + b0, lasso->ridge);
        else if (nonneg)
            hipLaunchKernelGGL((k_rf_nnls<T>), dim3(Bc), dim3(256), rf_nnls_lds<T>(kcap), st, (const T*)w.part, nchunks, tile_cap, recs,
                               place.dout + b0 * rb, rb, kmax, w.stat + b0, w.drop + b0);
        else if (prune)
            hipLaunchKernelGGL((k_rf_prune<T>), dim3(Bc), dim3(256), rf_prune_lds<T>(kcap), st, (const T*)w.part, nchunks, tile_cap, recs,
                               place.dout + b0 * rb, rb, kmax, w.stat + b0, w.drop + b0,
                               RfPrune{ prune->keep, prune->rule, prune->min_share, w.score ? w.score + b0 * kmax : nullptr });
        else
            hipLaunchKernelGGL((k_rf_solve<T>), dim3(Bc), dim3(256), rf_solve_lds<T>(kcap), st, (const T*)w.part, nchunks, tile_cap, recs,
                               place.dout + b0 * rb, rb, kmax, w.stat + b0);
        HIPCHK(hipGetLastError());
    }
    if (resnorm) {
        const int rr = Wd ? weighted_residual_rows<T>(ctx, who, false, Y, B, y_stride, incy, place.dout, kmax, w.rn, 1, nullptr, nullptr, Wd, ws, err, errlen)
                          : record_residual_norms<T>(ctx, who, Y, B, y_stride, incy, place.dout, kmax, w.rn, err, errlen);
        if (rr != SS_HIP_OK) return rr;
        hipLaunchKernelGGL((k_rf_widen<T>), dim3((Bu + 255u) / 256u), dim3(256), 0, st, (const T*)w.rn, w.rnd, Bu);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(resnorm, w.rnd, B * sizeof(double), hipMemcpyDefault, st));
    }
    if (status) HIPCHK(hipMemcpyAsync(status, w.stat, B * sizeof(uint32_t), hipMemcpyDefault, st));
    if (shrinks && dropped) HIPCHK(hipMemcpyAsync(dropped, w.drop, B * sizeof(uint32_t), hipMemcpyDefault, st));
    if (score_elems) HIPCHK(hipMemcpyAsync(prune->score, w.score, score_elems * sizeof(double), hipMemcpyDefault, st));
    place.copy_out(w.stage, st);
    HIPCHK(hipStreamSynchronize(st));
    return SS_HIP_OK;
}

// weighted: the call carries W / w_stride (ss_hip_weighted_refit_records_*), checked and brought to the device behind the other checks;
// nonneg: the non-negative fit (ss_hip_nonneg_refit_records_*), with `dropped`; prune: the pruning call (ss_hip_prune_records_*), its
// three settings checked behind the refit's arguments, with `dropped` and prune->score; lasso: the l1 refit (ss_hip_lasso_refit_records_*),
// lam, lam_stride and ridge checked there too (the lam_b themselves on the device), with `dropped`
template <typename T>
int refit_entry(ss_hip_ctx* ctx, const char* who, const T* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const void* records, uint32_t kmax,
                void* records_out, double* resnorm, uint32_t* status, bool weighted, const T* W, ptrdiff_t w_stride, char* err, size_t errlen,
                bool nonneg = false, uint32_t* dropped = nullptr, const RfPrune* prune = nullptr, const RfLasso* lasso = nullptr)
{
    const std::string w(who);
    int rc = check_common<T>(ctx, who, records, true, kmax, err, errlen);
    if (rc != SS_HIP_OK) return rc;
    if (!Y || !records_out) { set_err(err, errlen, w + ": Y and records_out must not be null"); return SS_HIP_EINVAL; }
    if ((rc = check_out_aligned(who, records_out, err, errlen)) != SS_HIP_OK) return rc;
    if (incy <= 0 || y_stride <= 0) { set_err(err, errlen, w + ": increments and strides must be positive"); return SS_HIP_EINVAL; }
    if (weighted && (rc = weights_check_args(ctx, who, W, w_stride, err, errlen)) != SS_HIP_OK) return rc;
    if (prune) {
        if (prune->keep == 0u) { set_err(err, errlen, w + ": keep must be at least 1"); return SS_HIP_EINVAL; }
        if (prune->rule != (uint32_t)SS_HIP_PRUNE_MAGNITUDE && prune->rule != (uint32_t)SS_HIP_PRUNE_BACKWARD) {
            set_err(err, errlen, w + ": rule must be SS_HIP_PRUNE_MAGNITUDE or SS_HIP_PRUNE_BACKWARD");
            return SS_HIP_EINVAL;
        }
        if (!(prune->min_share >= 0.0 && prune->min_share <= std::numeric_limits<double>::max())) {
            set_err(err, errlen, w + ": min_share must be finite and >= 0");
            return SS_HIP_EINVAL;
        }
    }
    if (lasso) {
        if (!lasso->lam) { set_err(err, errlen, w + ": lam must not be null"); return SS_HIP_EINVAL; }
        if (lasso->lam_stride != 0 && lasso->lam_stride != 1) { set_err(err, errlen, w + ": lam_stride must be 0 or 1"); return SS_HIP_EINVAL; }
        if (!(lasso->ridge >= 0.0 && lasso->ridge <= std::numeric_limits<double>::max())) {
            set_err(err, errlen, w + ": ridge must be finite and >= 0");
            return SS_HIP_EINVAL;
        }
    }
    if (B == 0) return SS_HIP_OK;                             // (every argument above was checked all the same)
    if ((rc = check_batch(who, B, err, errlen)) != SS_HIP_OK) return rc;
    return guarded(err, errlen, who, [&]() -> int {
        const T* Wd = nullptr;
        long long ws = 0;
        if (weighted) {
            const int rw = weights_on_device<T>(ctx, who, W, B, w_stride, &Wd, &ws, err, errlen);
            if (rw != SS_HIP_OK) return rw;
        }
        return refit_impl<T>(ctx, who, Y, B, y_stride, incy, records, kmax, records_out, resnorm, status, Wd, ws, nonneg, dropped, prune, lasso, err, errlen);
    });
}

}  // namespace

template <typename T>
int refit_weighted(ss_hip_ctx* ctx, const T* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const T* W, ptrdiff_t w_stride, const void* records,
                   uint32_t kmax, void* records_out, double* resnorm, uint32_t* status, char* err, size_t errlen)
{
    return refit_entry<T>(ctx, "weighted_refit_records", Y, B, y_stride, incy, records, kmax, records_out, resnorm, status, true, W, w_stride, err,
                          errlen);
}
template int refit_weighted<float>(ss_hip_ctx*, const float*, size_t, ptrdiff_t, ptrdiff_t, const float*, ptrdiff_t, const void*, uint32_t, void*,
                                   double*, uint32_t*, char*, size_t);
template int refit_weighted<double>(ss_hip_ctx*, const double*, size_t, ptrdiff_t, ptrdiff_t, const double*, ptrdiff_t, const void*, uint32_t, void*,
                                    double*, uint32_t*, char*, size_t);

template <typename T>
int refit_nonneg(ss_hip_ctx* ctx, const T* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const void* records, uint32_t kmax, void* records_out,
                 double* resnorm, uint32_t* status, uint32_t* dropped, char* err, size_t errlen)
{
    return refit_entry<T>(ctx, "nonneg_refit_records", Y, B, y_stride, incy, records, kmax, records_out, resnorm, status, false, nullptr, 0, err,
                          errlen, true, dropped);
}
template int refit_nonneg<float>(ss_hip_ctx*, const float*, size_t, ptrdiff_t, ptrdiff_t, const void*, uint32_t, void*, double*, uint32_t*, uint32_t*,
                                 char*, size_t);
template int refit_nonneg<double>(ss_hip_ctx*, const double*, size_t, ptrdiff_t, ptrdiff_t, const void*, uint32_t, void*, double*, uint32_t*, uint32_t*,
                                  char*, size_t);

template <typename T>
int refit_prune(ss_hip_ctx* ctx, const T* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const void* records, uint32_t kmax, void* records_out,
                uint32_t keep, uint32_t rule, double min_share, double* resnorm, uint32_t* status, uint32_t* dropped, double* score, char* err,
                size_t errlen)
{
    const RfPrune prune{ keep, rule, min_share, score };
    return refit_entry<T>(ctx, "prune_records", Y, B, y_stride, incy, records, kmax, records_out, resnorm, status, false, nullptr, 0, err, errlen,
                          false, dropped, &prune);
}
template int refit_prune<float>(ss_hip_ctx*, const float*, size_t, ptrdiff_t, ptrdiff_t, const void*, uint32_t, void*, uint32_t, uint32_t, double,
                                double*, uint32_t*, uint32_t*, double*, char*, size_t);
template int refit_prune<double>(ss_hip_ctx*, const double*, size_t, ptrdiff_t, ptrdiff_t, const void*, uint32_t, void*, uint32_t, uint32_t, double,
                                 double*, uint32_t*, uint32_t*, double*, char*, size_t);

template <typename T>
int refit_lasso(ss_hip_ctx* ctx, const T* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const void* records, uint32_t kmax, void* records_out,
                const double* lam, ptrdiff_t lam_stride, double ridge, double* resnorm, uint32_t* status, uint32_t* dropped, char* err,
                size_t errlen)
{
    const RfLasso lasso{ lam, lam_stride, ridge };
    return refit_entry<T>(ctx, "lasso_refit_records", Y, B, y_stride, incy, records, kmax, records_out, resnorm, status, false, nullptr, 0, err, errlen,
                          false, dropped, nullptr, &lasso);
}
template int refit_lasso<float>(ss_hip_ctx*, const float*, size_t, ptrdiff_t, ptrdiff_t, const void*, uint32_t, void*, const double*, ptrdiff_t, double,
                                double*, uint32_t*, uint32_t*, char*, size_t);
template int refit_lasso<double>(ss_hip_ctx*, const double*, size_t, ptrdiff_t, ptrdiff_t, const void*, uint32_t, void*, const double*, ptrdiff_t, double,
                                 double*, uint32_t*, uint32_t*, char*, size_t);

}  // namespace sship

using namespace sship;

extern "C" {

int ss_hip_refit_records_f32(ss_hip_ctx* ctx, const float* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const void* records,
                             uint32_t kmax, void* records_out, double* resnorm, uint32_t* status, char* err, size_t errlen)
{
    return refit_entry<float>(ctx, "refit_records", Y, B, y_stride, incy, records, kmax, records_out, resnorm, status, false, nullptr, 0, err, errlen);
}
int ss_hip_refit_records_f64(ss_hip_ctx* ctx, const double* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const void* records,
                             uint32_t kmax, void* records_out, double* resnorm, uint32_t* status, char* err, size_t errlen)
{
    return refit_entry<double>(ctx, "refit_records", Y, B, y_stride, incy, records, kmax, records_out, resnorm, status, false, nullptr, 0, err, errlen);
}

}  // extern "C"
