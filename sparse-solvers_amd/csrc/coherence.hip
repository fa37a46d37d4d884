// coherence.hip — the coherence of atoms on the matrix cores (include/ss_hip.h): ss_hip_atom_coherence_*.
//
// For a query atom j the call returns mu = max over the other atoms i of |a_i . a_j| / (||a_i|| ||a_j||) and the smallest i that
// attains it: a row arg-max over the normalised A^T A.  The Gram product runs on the MFMA units with the normalisation, the masks
// and the arg-max in the epilogue; G is never written and a resident G is never read (fp32 only, and its words are its own build's).
// Three kernels:
//
//   k_coh_norms  one wave per column of the padded dictionary: d_i = sum_k a_ki^2 in double, r_i = 1 / sqrt(d_i) — 0 for a column
//                that is excluded (d_i zero or not finite, or i >= n).  Per call, from A: nothing is kept on the context.
//   k_coh_tile   grid = (query tile, column tile), 128 x 128 x 128 bytes of K per step, 256 threads, two workgroups a CU (72 KiB of
//                staging LDS).  The queries are rows of At named by a device list (the staging loads index through it), the other
//                operand is At itself.  Both operands are K-contiguous; register-staged double buffer, one barrier per K-step.
//                fp32: four waves of 2 x 2 v_mfma_f32_32x32x2_f32 accumulators fed by ds_read_b128 (gemm.hip's idiom);
//                fp64: four waves of 4 x 4 v_mfma_f64_16x16x4_f64 accumulators.
//                Epilogue, per query row: score of every column of the tile, the masks, the best (score, smallest index) across
//                the lanes that hold the row (shuffles), then across the two waves that share it (LDS): one partial per
//                (query, column tile).
//   k_coh_finish one wave per query: the partials in ascending column-tile order, strictly-greater comparison.
//
// ORDER (stated once; build flag -ffp-contract=off: outside the MFMA products and sums are rounded separately):
//   dot(i, j)    one accumulator, started at 0, in the context's precision; the K-steps ascending over the padded rows (rows
//                m .. ldm - 1 are zero; ldm = m rounded up to 256).  fp32: a K-step holds 32 rows; MFMA (g, t), g = 0 .. 3 outer,
//                t = 0 .. 3 inner, adds the rows 8 g + t and 8 g + 4 + t of the step, in the instruction's order.  fp64: a K-step holds
//                16 rows; MFMA g = 0 .. 3 adds the rows 4 g .. 4 g + 3.  An MFMA is a chain of fused multiply-adds; the chain does
//                not depend on where in a tile the pair sits, and a product commutes: dot(i, j) is a function of the two columns
//                and m alone, and dot(i, j) == dot(j, i) bit for bit.
//   d_i          lane l of the column's wave adds the squares of rows l, l + 64, ... < m in ascending order (the square and the sum
//                in double, each rounded), then the 64 lane sums are added by the butterfly s += s(lane ^ o), o = 32, 16, .., 1.
//   r_i          = 1 / sqrt(d_i), both correctly rounded in double.
//   s(i, j)      = |dot(i, j)| * (r_i * r_j), dot widened to double: two multiplications, the product of the norms first (so that
//                s(i, j) == s(j, i) bit for bit).
//   mu, partner  the largest s(i, j) over the columns i != j that are not excluded, and the smallest i that attains it — a maximum
//                and a minimum: whichever order the comparisons run in, the result is the same.  A NaN score never wins.
// Exclusion is by index mask (r_i == 0 selects it), never by multiplying by zero.  No floating-point atomics; nothing depends on S, on
// what else is in cols, on the query chunking, on where the pointers live or on what the context did before.
#include "ss_hip_internal.h"
#include "record_common.h"

#include <algorithm>
#include <cmath>
#include <numeric>

namespace sship {

namespace {

constexpr uint32_t kCohTile = 128;                       // queries and columns per tile
constexpr uint32_t kCohVecs = 8;                         // 16-byte vectors of K per row and step (32 floats / 16 doubles)
constexpr uint32_t kCohPitch = kCohVecs + 1;             // LDS row pitch in vectors (144 B, as in gemm.hip)
constexpr uint32_t kCohNone = SS_HIP_COHERENCE_NONE;
static_assert(SS_HIP_COHERENCE_CHUNK % kCohTile == 0, "a chunk is whole query tiles");

typedef float coh_v4f __attribute__((ext_vector_type(4)));
typedef float coh_v16f __attribute__((ext_vector_type(16)));
typedef double coh_v2d __attribute__((ext_vector_type(2)));
typedef double coh_v4d __attribute__((ext_vector_type(4)));

// the wave's 64 x 64 share of a tile as NI x NI accumulators of WT x WT: a lane holds column (lane & (WT - 1)) of each, and the
// rows row(e, lane / WT) of its NE results
template <typename T> struct CohMma;
template <> struct CohMma<float> {
    typedef coh_v4f Vec;
    typedef coh_v16f Acc;
    static constexpr uint32_t NI = 2, NE = 16, WT = 32, KS = 32;
    // C/D layout of the 32 x 32 MFMA: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    __device__ static uint32_t row(uint32_t e, uint32_t hq) { return (e & 3u) + 8u * (e >> 2) + 4u * hq; }
};
template <> struct CohMma<double> {
    typedef coh_v2d Vec;
    typedef coh_v4d Acc;
    static constexpr uint32_t NI = 4, NE = 4, WT = 16, KS = 16;
    // C/D layout of the fp64 16 x 16 MFMA: col = lane & 15, row = (lane >> 4) + 4 reg
    __device__ static uint32_t row(uint32_t e, uint32_t hq) { return 4u * e + hq; }
};

// (score, index): a wins over b when it is larger, or equal with the smaller index
__device__ inline bool coh_better(double sa, uint32_t ia, double sb, uint32_t ib) { return sa > sb || (sa == sb && ia < ib); }

struct CoherenceState {
    Holdings own;
    unsigned char* buf = nullptr;      // inverse norms, the query list, the partials of a chunk, the staged outputs
    size_t bytes = 0;
};

CoherenceState* state_of(ss_hip_ctx* ctx)
{
    return &part<CoherenceState>(ctx->coh);
}

// ---- kernels -------------------------------------------------------------------------------------------------------------------

// SUM: d_i itself is stored instead of its inverse root (coh_launch_norms' flag: the weighted top correlations)
template <typename T, bool SUM = false>
__global__ __launch_bounds__(256)
void k_coh_norms(const T* __restrict__ At, uint32_t ldm, uint32_t m, uint32_t n, uint32_t n_pad, double* __restrict__ rinv)
{
    const uint32_t lane = threadIdx.x & 63u, i = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (i >= n_pad) return;
    double s = 0.0;
    if (i < n) {
        const T* a = At + (size_t)i * ldm;
        for (uint32_t k = lane; k < m; k += 64u) { const double v = (double)a[k]; s = s + v * v; }
    }
    s = wave_sum(s);
    if (lane == 0) rinv[i] = (i < n && s > 0.0 && s <= 1.7976931348623157e308) ? (SUM ? s : 1.0 / sqrt(s)) : 0.0;
}

// qlist: the chunk's queries, padded to whole tiles with SS_HIP_COHERENCE_NONE; pscore / pidx: [query of the chunk][ntiles]
template <typename T>
__global__ __launch_bounds__(256, 2)
void k_coh_tile(const T* __restrict__ At, uint32_t ldm, const uint32_t* __restrict__ qlist, const double* __restrict__ rinv,
                uint32_t ntiles, double* __restrict__ pscore, uint32_t* __restrict__ pidx)
{
    typedef CohMma<T> M;
    typedef typename M::Vec Vec;
    typedef typename M::Acc Acc;
    constexpr uint32_t NI = M::NI, NE = M::NE, WT = M::WT;
    __shared__ __attribute__((aligned(16))) Vec sA[2][kCohTile][kCohPitch];      // the queries
    __shared__ __attribute__((aligned(16))) Vec sB[2][kCohTile][kCohPitch];      // the columns
    __shared__ double sQr[kCohTile], sCr[kCohTile], sRs[2][kCohTile];
    __shared__ uint32_t sQi[kCohTile], sRi[2][kCohTile];

    // query tiles fastest: concurrently resident workgroups share the same panel of At
    const uint32_t qt = blockIdx.x, bn = blockIdx.y;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t wm = wave & 1u, wn = wave >> 1;
    const uint32_t lc = lane & (WT - 1u), hq = lane / WT;

    // staging map: thread -> (rows srow + 32 j, vector svec of the step)
    const uint32_t srow = tid >> 3, svec = tid & 7u;
    const Vec* gA[4];
    const Vec* gB[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t q = qlist[qt * kCohTile + srow + 32u * (uint32_t)j];
        gA[j] = reinterpret_cast<const Vec*>(At + (size_t)(q == kCohNone ? 0u : q) * ldm) + svec;
        gB[j] = reinterpret_cast<const Vec*>(At + (size_t)(bn * kCohTile + srow + 32u * (uint32_t)j) * ldm) + svec;
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
    for (int j = 0; j < 4; ++j) { stA[j] = gA[j][0]; stB[j] = gB[j][0]; }
#pragma unroll
    for (int j = 0; j < 4; ++j) { sA[0][srow + 32 * j][svec] = stA[j]; sB[0][srow + 32 * j][svec] = stB[j]; }
    __syncthreads();

    const uint32_t nk = ldm / M::KS;
    uint32_t cur = 0;
    for (uint32_t kt = 0; kt < nk; ++kt) {
        const bool more = (kt + 1u) < nk;
        if (more) {
            const uint32_t voff = (kt + 1u) * kCohVecs;
#pragma unroll
            for (int j = 0; j < 4; ++j) { stA[j] = gA[j][voff]; stB[j] = gB[j][voff]; }
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

    // ---- epilogue: normalise, mask, arg-max per query row ----
    if (tid < kCohTile) {
        const uint32_t q = qlist[qt * kCohTile + tid];
        sQi[tid] = q;
        sQr[tid] = q == kCohNone ? 0.0 : rinv[q];
    } else {
        sCr[tid - kCohTile] = rinv[bn * kCohTile + (tid - kCohTile)];
    }
    __syncthreads();
    double cr[NI];
#pragma unroll
    for (uint32_t j = 0; j < NI; ++j) cr[j] = sCr[wn * 64u + j * WT + lc];
    const uint32_t col0 = bn * kCohTile + wn * 64u + lc;
#pragma unroll
    for (uint32_t i = 0; i < NI; ++i)
#pragma unroll
        for (uint32_t e = 0; e < NE; ++e) {
            const uint32_t row = wm * 64u + i * WT + M::row(e, hq);
            const uint32_t qi = sQi[row];
            const double qr = sQr[row];
            double bs = -1.0;
            uint32_t bi = kCohNone;
#pragma unroll
            for (uint32_t j = 0; j < NI; ++j) {                  // (ascending columns: strictly greater keeps the smallest index)
                const uint32_t col = col0 + j * WT;
                const bool live = qr != 0.0 && cr[j] != 0.0 && col != qi;
                const double s = fabs((double)acc[i][j][e]) * (qr * cr[j]);
                if (live && s > bs) { bs = s; bi = col; }
            }
#pragma unroll
            for (uint32_t o = WT / 2u; o >= 1u; o >>= 1) {
                const double os = __shfl_xor(bs, (int)o);
                const uint32_t oi = (uint32_t)__shfl_xor((int)bi, (int)o);
                if (coh_better(os, oi, bs, bi)) { bs = os; bi = oi; }
            }
            if (lc == 0u) { sRs[wn][row] = bs; sRi[wn][row] = bi; }
        }
    __syncthreads();
    if (tid < kCohTile) {
        double bs = sRs[0][tid];
        uint32_t bi = sRi[0][tid];
        if (sRs[1][tid] > bs) { bs = sRs[1][tid]; bi = sRi[1][tid]; }
        const size_t p = (size_t)(qt * kCohTile + tid) * ntiles + bn;
        pscore[p] = bs;
        pidx[p] = bi;
    }
}

__global__ __launch_bounds__(256)
void k_coh_finish(const double* __restrict__ pscore, const uint32_t* __restrict__ pidx, uint32_t ntiles, uint32_t count,
                  double* __restrict__ mu, uint32_t* __restrict__ partner)
{
    const uint32_t lane = threadIdx.x & 63u, q = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (q >= count) return;
    double bs = -1.0;
    uint32_t bi = kCohNone;
    for (uint32_t t = lane; t < ntiles; t += 64u) {
        const double s = pscore[(size_t)q * ntiles + t];
        if (s > bs) { bs = s; bi = pidx[(size_t)q * ntiles + t]; }
    }
#pragma unroll
    for (uint32_t o = 32u; o >= 1u; o >>= 1) {
        const double os = __shfl_xor(bs, (int)o);
        const uint32_t oi = (uint32_t)__shfl_xor((int)bi, (int)o);
        if (coh_better(os, oi, bs, bi)) { bs = os; bi = oi; }
    }
    if (lane == 0) {
        mu[q] = bi == kCohNone ? 0.0 : bs;
        partner[q] = bi;
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------

// the call's pieces: the norms, the queries, a chunk's tile partials, the outputs
struct CohWork {
    double *rinv, *ps, *mud;
    uint32_t *qd, *pi, *ptd;
    void carve(Carver& cv, size_t n_pad, size_t Spad, size_t partials)
    {
        rinv = cv.take<double>(n_pad);
        qd = cv.take<uint32_t>(Spad);
        ps = cv.take<double>(partials);
        pi = cv.take<uint32_t>(partials);
        mud = cv.take<double>(Spad);
        ptd = cv.take<uint32_t>(Spad);
    }
};

template <typename T>
int coherence_impl(ss_hip_ctx* ctx, const uint32_t* cols, size_t S, double* mu, uint32_t* partner, char* err, size_t errlen)
{
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint32_t n = (uint32_t)ctx->n, n_pad = ctx->n_pad, ldm = ctx->ldm;
    const uint32_t ntiles = (n + kCohTile - 1u) / kCohTile;
    const size_t Spad = (S + kCohTile - 1) / kCohTile * kCohTile;

    // the queries on the host, checked before anything is written, then padded to whole tiles
    std::vector<uint32_t> q(Spad, kCohNone);
    if (!cols) std::iota(q.begin(), q.begin() + (ptrdiff_t)S, 0u);
    else if (on_device(cols)) {
        HIPCHK(hipMemcpyAsync(q.data(), cols, S * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    } else std::copy(cols, cols + S, q.begin());
    for (size_t s = 0; s < S; ++s)
        if (q[s] >= n) {
            set_err(err, errlen, "atom_coherence: cols[" + std::to_string(s) + "] names a column >= n");
            return SS_HIP_EINVAL;
        }

    CoherenceState* cs = state_of(ctx);
    const size_t chunk = std::min<size_t>(Spad, SS_HIP_COHERENCE_CHUNK);
    CohWork w;
    grow(cs->own, cs->buf, cs->bytes, carve_into(nullptr, w, n_pad, Spad, chunk * ntiles), "hipMalloc(coherence workspace)");
    carve_into(cs->buf, w, n_pad, Spad, chunk * ntiles);
    const T* At = static_cast<const T*>(ctx->At);
    HIPCHK(hipMemcpyAsync(w.qd, q.data(), Spad * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL((k_coh_norms<T>), dim3(n_pad / 4u), dim3(256), 0, st, At, ldm, (uint32_t)ctx->m, n, n_pad, w.rinv);
    HIPCHK(hipGetLastError());
    for (size_t s0 = 0; s0 < S; s0 += chunk) {
        const uint32_t Sc = (uint32_t)std::min(chunk, S - s0), qtiles = (Sc + kCohTile - 1u) / kCohTile;
        hipLaunchKernelGGL((k_coh_tile<T>), dim3(qtiles, ntiles), dim3(256), 0, st, At, ldm, (const uint32_t*)(w.qd + s0),
                           (const double*)w.rinv, ntiles, w.ps, w.pi);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_coh_finish, dim3((Sc + 3u) / 4u), dim3(256), 0, st, (const double*)w.ps, (const uint32_t*)w.pi, ntiles, Sc,
                           w.mud + s0, w.ptd + s0);
        HIPCHK(hipGetLastError());
    }
    if (mu) HIPCHK(hipMemcpyAsync(mu, w.mud, S * sizeof(double), hipMemcpyDefault, st));
    if (partner) HIPCHK(hipMemcpyAsync(partner, w.ptd, S * sizeof(uint32_t), hipMemcpyDefault, st));
    HIPCHK(hipStreamSynchronize(st));                    // (q is read by the upload until here)
    return SS_HIP_OK;
}

template <typename T>
int coherence_entry(ss_hip_ctx* ctx, const uint32_t* cols, size_t S, double* mu, uint32_t* partner, char* err, size_t errlen)
{
    static const char* who = "atom_coherence";
    if (!ctx) { set_err(err, errlen, "atom_coherence: null context"); return SS_HIP_EINVAL; }
    if (!mu && !partner) { set_err(err, errlen, "atom_coherence: mu and partner must not both be null"); return SS_HIP_EINVAL; }
    if (ctx->kind != 0) { set_err(err, errlen, "atom_coherence: this context was created for IRLS"); return SS_HIP_EINVAL; }
    if (ctx->colshard != nullptr) { set_err(err, errlen, "atom_coherence: not available on a column-sharded context"); return SS_HIP_EINVAL; }
    if (ctx->is_f64 != (sizeof(T) == 8)) { set_err(err, errlen, "atom_coherence: element type mismatch"); return SS_HIP_ETYPE; }
    if (!cols) S = ctx->n;
    if (S == 0) return SS_HIP_OK;                             // (every argument above was checked all the same)
    if (S >= 0x80000000ull) { set_err(err, errlen, "atom_coherence: S must stay below 2^31"); return SS_HIP_EINVAL; }
    return guarded(err, errlen, who, [&] { return coherence_impl<T>(ctx, cols, S, mu, partner, err, errlen); });
}

}  // namespace

template <typename T, bool SUM>
hipError_t coh_launch_norms(ss_hip_ctx* ctx, double* rinv)
{
    hipLaunchKernelGGL((k_coh_norms<T, SUM>), dim3(ctx->n_pad / 4u), dim3(256), 0, ctx->stream, static_cast<const T*>(ctx->At), ctx->ldm,
                       (uint32_t)ctx->m, (uint32_t)ctx->n, ctx->n_pad, rinv);
    return hipGetLastError();
}
template hipError_t coh_launch_norms<float>(ss_hip_ctx*, double*);
template hipError_t coh_launch_norms<double>(ss_hip_ctx*, double*);
template hipError_t coh_launch_norms<float, true>(ss_hip_ctx*, double*);
template hipError_t coh_launch_norms<double, true>(ss_hip_ctx*, double*);

}  // namespace sship

using namespace sship;

extern "C" {

int ss_hip_atom_coherence_f32(ss_hip_ctx* ctx, const uint32_t* cols, size_t S, double* mu, uint32_t* partner, char* err, size_t errlen)
{
    return coherence_entry<float>(ctx, cols, S, mu, partner, err, errlen);
}
int ss_hip_atom_coherence_f64(ss_hip_ctx* ctx, const uint32_t* cols, size_t S, double* mu, uint32_t* partner, char* err, size_t errlen)
{
    return coherence_entry<double>(ctx, cols, S, mu, partner, err, errlen);
}

}  // extern "C"
