// screen.hip — the SCREENED form of one fp32 signal: the subset form of subbatch.hip without G = A^T A.
//
// The default single-signal engine reads A three times per solve: c0 = A^T y, then two passes that form the Gram columns
// of the support over ALL n columns — and those two passes exist only so that every breakpoint the speculative
// iterations took on a column subset can be checked against the other ~65 000 columns (find_max_gamma and inf_norm run
// over all columns: /root/reference/src/solvers/homotopy-cpu.cpp:100-164, :236).  That check asks one question per
// (column i outside the subset, state k of the path): is |c_i| = |a_i . r_k| below lambda_k — by how much is irrelevant.
// Here it is answered by ONE pass over a half-precision copy of A with a rigorous error bound:
//
//   k_scr_first    (option screen_first16, the default) c~0 = A16^T y over the half-precision copy instead of the fp32 sweep: the
//                  ranking only — see the kernel's comment; state 0 is then certified like every other
//   k_sub_select   the 448 columns with the largest |c0| (subbatch.hip)
//   k_sgram_part / k_sgram_sum    Gs = A_S^T A_S of those columns from the fp32 A (v_mfma_f32_32x32x2_f32, 8 row chunks
//                  summed in a fixed order: deterministic); with k_scr_first: their exact fp32 c0 = a_j . y beside the sum
//   k_sub_solve    the whole path on the subset, all arithmetic in fp32 on Gs (subbatch.hip, gsub = 1): this is what is
//                  REPORTED — support, coefficients, iterations, lambda
//   k_scr_residuals   r_k = y - A_S x_S(k) for every logged state k >= 1, in fp32, then scaled by a power of two and
//                  rounded to fp16; ||r_k||^2
//   k_scr_gemm     C~ = A16^T [r16_1 .. r16_K] on v_mfma_f32_32x32x16_f16, 1.07 GB instead of two passes of 2.15 GB, and in
//                  its epilogue, for every column outside the subset and every state:
//                      |c~_ik| + eps_ik <= bound_k        eps_ik = 2^-9 ||a_i|| ||r_k|| (+ the flush terms)
//
// Why that is enough (exact arithmetic first).  Let lambda_k be the logged max |c| of state k.  If every column outside the
// subset has |c_i(k)| < lambda_k and |c_i(k+1)| < lambda_{k+1} then (a) lambda_k = max |c| over ALL columns is the
// subset's, and (b) the column's step-length candidates (homotopy-cpu.cpp:130-161) are t = (lambda_k -/+ c_i)/(1 -/+ q_i) with
// q_i = (c_i(k) - c_i(k+1)) / gamma_k: positive numerators; a non-positive denominator gives t <= 0 or no candidate, which
// the reference skips; a positive one gives t > gamma_k  <=>  +/- c_i(k+1) < lambda_{k+1}.  So the reference's scan over
// all n columns picks what the subset's scan picked, state after state.  The bound keeps a MARGIN (1/8 of lambda_k, and
// 1e-5 lambda_0 absolute) between "certified" and "equal", far above any fp32 rounding of the reference's own correlations
// (the columns that matter sit at ~0.4 lambda on a Gaussian dictionary; the subset holds the ones near lambda).  "lambda_{k+1}"
// above is where the step LEFT lambda, lambda_k - gamma_k: on a regular path that is the next max |c|, on a derailed one
// (the reference's first-step sign quirk) max |c| can sit above it — the bound takes the smaller of the two
// (tools/stress_screen.py found both this and the next point).  The state a path ENDS in by tolerance: if its last step
// landed on lambda = 0 within rounding (the least-squares jump of a noise-free path) every column's candidate ties with that
// step — whichever column the reference inserts there enters with x = 0 — and the state is certified against the
// tolerance itself: nothing out there keeps the path going.  A path that crosses the tolerance on a regular step (noise) has
// that step certified like any other.
//
// The error bound.  a16 = fl16(sA a), r16 = fl16(s_k r) with powers of two sA, s_k; round-to-nearest gives relative
// errors <= 2^-11 each in the normal range, the MFMA accumulates in fp32 (<= ldm 2^-24 relative to sum |a||r| at worst),
// so |c~ - c| <= (2^-10 + 2^-22 + ldm 2^-24) sum |a_ir||r_kr| <= 2^-9 ||a_i|| ||r_k|| for ldm <= 16384 (checked).  Entries
// below the fp16 normal range (and a possible flush of subnormal inputs by the matrix unit) add at most 2^-14 per entry in
// scaled units: 2^-14 sqrt(ldm) (||r_k|| / sA + ||a_i|| / s_k).  An fp16 overflow of a residual raises the failure flag.
//
// Nothing reported comes from the half-precision pass: a column it cannot certify makes the signal kStatusSubsetFail and
// the host solves it again in the default engine (exact fp32 passes over A) — like every declined signal of the subset form.
#include "ss_hip_internal.h"
#include "ss_hip_device.h"
#include "resident.h"
#include "subcheck.h"

#include <hip/hip_fp16.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <type_traits>

namespace sship {

typedef _Float16 scr_h8 __attribute__((ext_vector_type(8)));
typedef float scr_v16f __attribute__((ext_vector_type(16)));
typedef float scr_v4f __attribute__((ext_vector_type(4)));
typedef uint32_t scr_u4 __attribute__((ext_vector_type(4)));
typedef float scr_v2f __attribute__((ext_vector_type(2)));

constexpr uint32_t kScrRhs = 96;                 // right-hand sides of the screening pass: states 1 .. nlog - 1 (<= kSbLog - 1 = 79)
constexpr uint32_t kScrCols = 128;               // dictionary columns per workgroup of the pass
constexpr uint32_t kScrKc = 128;                 // rows per stage
constexpr uint32_t kScrPitchB = kScrKc * 2 + 16; // bytes per LDS row: 272 (16-byte reads of 8 consecutive rows: conflict-free)
constexpr uint32_t kScrWmax = 8192;              // floats of ScreenState::wmax (2 workgroups per CU x 8 waves)
constexpr uint32_t kScrMeta = 16;                // floats of ScreenState::meta ([8], [9]: the error model of the first pass that ran; [10], [11]: the fp8 copy's scale and its inverse)
constexpr uint32_t kScrTab = 4;                  // floats per state in the table: 1 / (sA s_k), bound_k, 1 / s_k, spare
constexpr uint32_t kSgSplit = 8;                 // row chunks of the subset Gram matrix (partials summed in order)
constexpr uint32_t kSgT = 64;                    // its tile: 64 x 64 outputs per workgroup, a 32 x 32 quadrant per wave
constexpr uint32_t kSgStep = 64;                 // rows staged per step
constexpr uint32_t kSgPitchF = kSgStep + 4;      // floats per LDS row
constexpr uint32_t kScrBatch = 64;               // slots of a batch chunk in the screened form
// (kScrFlCap — columns the half-precision certificate may leave to the exact re-check, per signal — is resident.h's: k_res_residuals64 clears the list)
constexpr uint32_t kScrRepCap = 64;              // columns that may be ahead of the subset's last step (candidates of the repair)
constexpr uint32_t kScrRescueCap = 64;             // columns a rescue may add to the subset (more: the signal goes back)
constexpr uint32_t kScrFlFail = kScrFlCap + 16 + 4 * kScrRepCap;    // the columns that FAILED the exact re-check (count at [cap + 14]): what a rescue adds to the subset
constexpr uint32_t kScrFlWords = kScrFlFail + kScrRescueCap; // (+ the first failure for SS_HIP_SUB_DEBUG at [cap + 4 ..], the repair's count at [cap + 12], its {column, -, step as a double} entries from [cap + 16])  // the list: [0] count, [1 .. cap] columns, [cap + 1] state 0 needs the re-check, [cap + 2] bits(bound_0), [cap + 3] bits(eps_0)
constexpr uint32_t kScrRecheckWgs = 240;         // workgroups of the re-check launch
constexpr uint32_t kS64Sub = 2048;               // fp64 form: columns of the sub-dictionary the path is solved on
constexpr uint32_t kS64Rhs = 192;                // ... states it can certify (two launches of the screening pass)
constexpr uint32_t kS64LogCap = 200, kS64LogK = 200;   // ... state log of the sub-context: states, coefficients per state
static_assert(kSbS % kSgT == 0, "subset Gram tiles");
static_assert(kSbLog - 1 <= kScrRhs, "screening pass: right-hand sides");

// One all-or-nothing preparation: device arrays from one owner, taken in the order written; after the first that does not fit nothing
// more is asked for (ok = false: the caller gives back what the owner holds)
struct Takes {
    Holdings& own;
    bool ok = true;
    template <typename P> Takes& operator()(P** p, size_t bytes) { if (ok && own.device(p, bytes) != hipSuccess) ok = false; return *this; }
};

// The residual block of a screening pass: always taken, cleared, filled (k_scr_residuals, k_s64_residuals, k_res_residuals64) and read
// (k_scr_gemm, k_scr_gemm_b) together.  With slots the kernels add the slot offsets themselves.
struct ResBlock {
    __half* r16 = nullptr;       // [slots][rhs][ldm] fl16(s_k * r_k)
    float* rn2p = nullptr;       // [slots][ldm / 64][rhs] partial sums of ||r_k||^2, one per workgroup of the residual kernel
    float* tab = nullptr;        // [slots][rhs][kScrTab]
    uint32_t rhs = 0;            // right-hand sides (states) per slot: the pitch of rn2p

    void take(Takes& t, uint32_t rhs_, uint32_t ldm, size_t slots = 1)
    {
        rhs = rhs_;
        t(&r16, slots * rhs * ldm * sizeof(__half))(&rn2p, slots * (ldm / 64u) * rhs * sizeof(float))(&tab, slots * rhs * kScrTab * sizeof(float));
    }
    // (rows no residual kernel writes are read by the pass as zeros)
    hipError_t clear(uint32_t ldm, size_t slots, hipStream_t s) const { return hipMemsetAsync(r16, 0, slots * rhs * ldm * sizeof(__half), s); }
    // one slot's block; the states from k0 on (same pitch)
    ResBlock slot(size_t b, uint32_t ldm) const { return { r16 + b * rhs * ldm, rn2p + b * (ldm / 64u) * rhs, tab + b * rhs * kScrTab, rhs }; }
    ResBlock from(uint32_t k0, uint32_t ldm) const { return { r16 + (size_t)k0 * ldm, rn2p + k0, tab + (size_t)k0 * kScrTab, rhs }; }
};

// buffers of an fp64 batch chunk in the resident tier (launch_screen64_batch)
constexpr uint32_t kS64Batch = 32;               // slots of a chunk
struct Screen64Batch {
    Holdings own;                // everything below
    __half* y16 = nullptr;       // [128][ldm] the chunk's signals in fp16 (rows beyond the chunk: zeros)
    float* ytab = nullptr;       // [128][kScrTab] 1 / (sA s_y) per signal (the writing mode's scale)
    float* ymeta = nullptr;      // [kS64Batch][4] {||y||^2, threshold of the selection, 1 / s_y, spare}
    float* cabs = nullptr;       // [kS64Batch][n_pad] |c~0|
    uint32_t* sub = nullptr;     // [kS64Batch][S] the subsets (+ 2 words of scratch behind the last)
    double* gs = nullptr;        // [kS64Batch][S][S]
    double* gs_part = nullptr;   // [kS64Batch][kSg64MaxSplit][S][S]
    uint32_t* hdr = nullptr; double* H = nullptr; uint32_t* pcol = nullptr; double* X = nullptr;     // the slots' logs
    ResBlock res;                // [kS64Batch] x kS64Rhs states
    float* zero = nullptr;       // [ldm / 64][128] zeros (the writing mode reads no residual norms)
    double* c0 = nullptr;        // [kS64Batch][n_pad] dense c0 of every slot: exact at its subset's columns
};

// a batch chunk in the screened form (kScrBatch slots): every slot its own residual block, subset Gram matrix, table — made by the first
// such batch, all or nothing (owned by `batch`: a failed preparation leaves a fresh ScrBatchBufs)
struct ScrBatchBufs {
    Holdings batch;
    ResBlock b_res;              // [kScrBatch] x kScrRhs states
    float* b_gs_part = nullptr;  // [kScrBatch][kSgSplit][kSbS][kSbS]
    float* b_gs = nullptr;       // [kScrBatch][kSbS][kSbS]
};

struct ScreenState : ScrBatchBufs {
    ~ScreenState() { if (sub) ss_hip_homotopy_destroy(sub); }      // (the sub-context first; then b64, then what `own` holds)
    Holdings own;                // every device array below, the context's hand-off block, the sub-context's state log and pass partials
    __half* a16 = nullptr;       // [n_pad][ldm] fl16(sA * A), column-contiguous like A
    float* rank = nullptr;       // [n_pad] the rescue's ranking vector (made on first use)
    uint32_t rescue_first = 1, rescue_count = 0, rescue_first2 = 1, rescue_count2 = 0;   // which pieces of the list the rescue takes: first word, length
    uint8_t* a8 = nullptr;       // [n_pad][ldm] fl8(sA8 * A) in OCP e4m3: the RANKING pass only (k_scr_first8; made on first use)
    bool a8_failed = false;      // its allocation did not fit: the half-precision first pass goes on
    float* anorm = nullptr;      // [n_pad] ||a_i||_2, rounded up
    float* amaxc = nullptr;      // [n_pad] max |a_i| per column: what meta[2] is the maximum of (a column replaced later re-derives it, dictupdate.hip)
    float* meta = nullptr;       // [0] sA  [1] 1 / sA  [2] bits(max |A|)  [3] headroom of the last solve (bits, as uint)
                                 // [4] max ||a_i||  [5] ||y||^2 (k_scr_first)  [6] what the columns left out of the subset stay below (selection)
                                 // [12] 2^-u  [13] 2^u, u = dict_unit_exp([4]): the units of an fp64 dictionary's columns (1, 1 in an fp32
                                 // context)  [14] 1 where [12], [13] follow [4] (fp64), 0 where they stay 1
    ResBlock res;                // one signal's: kScrRhs states (fp32), kS64Rhs (fp64)
    float* gs_part = nullptr;    // [kSgSplit][kSbS][kSbS]
    float* gs = nullptr;         // [kSbS][kSbS]
    float* wmax = nullptr;       // [kScrWmax] k_scr_first: largest |c~0| per wave of its launch (the selection's floor)
    uint32_t* fl = nullptr;      // [kScrFlWords] the columns the certificate could not vouch for: re-checked exactly (k_scr_recheck)
    int gemm_attr = -1;
    // fp64 form: the path is solved by a context of its own over a sub-dictionary of kS64Sub columns
    ss_hip_ctx* sub = nullptr;
    float* cabs = nullptr;       // [n_pad] float(|c0|): what the selection ranks
    uint32_t* sublist = nullptr; // [kS64Sub] the sub-dictionary's columns, ascending; then first pick + value (2 words)
    double* xsub = nullptr;      // [kS64Sub] the sub-context's solution
    double* xd = nullptr;        // [kS64LogK][kS64Rhs + 8] coefficients of the screened states over the final list of touched columns (transposed)
    uint32_t* ctl = nullptr;     // [8] device words: [0] failure raised while the certificate was prepared
    // fp64 resident tier (resident.hip): the path on the 256 columns with the largest |c~0|, in ONE workgroup
    uint32_t* sub256 = nullptr;  // [256] ascending, then first pick + value (2 words)
    double* gs64 = nullptr;      // [256][256] the subset's Gram matrix
    double* gs64_part = nullptr; // [kSg64MaxSplit][256][256] its row-chunk partials
    uint32_t* rl_hdr = nullptr;  // the resident solve's log: headers [160][8]
    double* rl_H = nullptr;      // ... {lambda, gamma} [160][2]
    uint32_t* rl_pcol = nullptr; // ... the positions' columns [144]
    double* rl_X = nullptr;      // ... x by position of every state [160][136]
    double* rl_D = nullptr;      // ... the direction by position likewise (the exact re-check's chain)
    std::unique_ptr<Screen64Batch> b64;   // the buffers of an fp64 batch chunk in the resident tier (made by the first such batch)
};
static_assert(kS64Rhs == 192, "the residual block of the fp64 forms (resident.hip: kR64Rhs)");
// ---- one-time preparation ---------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256)
void k_a16_stats(const T* __restrict__ At, uint32_t ldm, float* __restrict__ anorm, float* __restrict__ amaxc, float* __restrict__ meta)
{
    __shared__ float sv[16];
    const T* a = At + (size_t)blockIdx.x * ldm;
    float ss = 0.f, mx = 0.f;
    for (uint32_t r = threadIdx.x * 4u; r < ldm; r += 1024u) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { const float v = (float)a[r + (uint32_t)e]; ss = __builtin_fmaf(v, v, ss); mx = fmaxf(mx, fabsf(v)); }
    }
    ss = block_sum(ss, sv);
    __syncthreads();
    // (max over the workgroup through the same scratch)
    mx = fmaxf(mx, __shfl_xor(mx, 1)); mx = fmaxf(mx, __shfl_xor(mx, 2)); mx = fmaxf(mx, __shfl_xor(mx, 4));
    mx = fmaxf(mx, __shfl_xor(mx, 8)); mx = fmaxf(mx, __shfl_xor(mx, 16)); mx = fmaxf(mx, __shfl_xor(mx, 32));
    if ((threadIdx.x & 63u) == 0u) sv[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        mx = fmaxf(fmaxf(sv[0], sv[1]), fmaxf(sv[2], sv[3]));
        anorm[blockIdx.x] = sqrtf(ss) * 1.0001f;                       // (rounded up: it scales an upper bound; fp64 sources: the cast's 2^-24 is inside)
        amaxc[blockIdx.x] = mx;
        atomicMax(reinterpret_cast<uint32_t*>(meta) + 2, __float_as_uint(mx));
        atomicMax(reinterpret_cast<uint32_t*>(meta) + 4, __float_as_uint(sqrtf(ss) * 1.0001f));      // (non-negative floats order like their bits)
    }
}

__global__ void k_a16_scale(float* __restrict__ meta, int units)
{
    const float amax = __uint_as_float(reinterpret_cast<const uint32_t*>(meta)[2]);
    const int e = pow2_scale_exp(16384.f, amax);
    meta[0] = ldexpf(1.f, e);
    meta[1] = ldexpf(1.f, -e);
    // units (the fp64 forms): residuals and column norms of the certificate in the units of the dictionary's largest column norm
    const int u = units ? dict_unit_exp(meta[4]) : 0;
    meta[12] = ldexpf(1.f, -u);
    meta[13] = ldexpf(1.f, u);
    meta[14] = units ? 1.f : 0.f;
}

template <typename T>
__global__ __launch_bounds__(256)
void k_a16_convert(const T* __restrict__ At, size_t total8, const float* __restrict__ meta, __half* __restrict__ a16)
{
    // (fp64 sources: one rounding, double -> half, of the exactly scaled value)
    const T sA = (T)meta[0];
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < total8; i += (size_t)gridDim.x * 256u) {
        scr_h8 h;
#pragma unroll
        for (int e = 0; e < 8; ++e) h[e] = (_Float16)(At[8u * i + (size_t)e] * sA);
        *reinterpret_cast<scr_h8*>(a16 + 8u * i) = h;
    }
}

// the fp8 (OCP e4m3: 3 mantissa bits, normal range 2^-6 .. 448, subnormal spacing 2^-9) copy for the ranking pass: the largest |a| lands in
// (112, 224] — far from the format's 448, so nothing saturates — and an entry's rounding error is 2^-4 relative, or 2^-10 absolute (scaled
// units) below the normal range
__global__ void k_a8_scale(float* __restrict__ meta)
{
    const float amax = __uint_as_float(reinterpret_cast<const uint32_t*>(meta)[2]);
    const int e = pow2_scale_exp(224.f, amax);
    meta[10] = ldexpf(1.f, e);
    meta[11] = ldexpf(1.f, -e);
}

template <typename T>
__global__ __launch_bounds__(256)
void k_a8_convert(const T* __restrict__ At, size_t total16, const float* __restrict__ meta, uint8_t* __restrict__ a8)
{
    const T s8 = (T)meta[10];
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < total16; i += (size_t)gridDim.x * 256u) {
        scr_u4 w;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const T* a = At + 16u * i + 4u * (size_t)q;
            int p = 0;
            p = __builtin_amdgcn_cvt_pk_fp8_f32((float)(a[0] * s8), (float)(a[1] * s8), p, false);
            p = __builtin_amdgcn_cvt_pk_fp8_f32((float)(a[2] * s8), (float)(a[3] * s8), p, true);
            w[q] = (uint32_t)p;
        }
        *reinterpret_cast<scr_u4*>(a8 + 16u * i) = w;
    }
}

// ---- the FIRST pass in half precision: c~0 = A16^T y --------------------------------------------------------------
// What the subset form needs from A^T y over ALL columns is a ranking (which 448 columns are worth solving on) and the same
// question as every later state: does anything left out reach lambda_0?  Both are answered from the half-precision copy,
// 1.07 GB instead of the 2.15 GB of the fp32 sweep: this kernel writes c~0 (fp16 A, fp32 y, fp32 sums), the selection ranks
// |c~0| and reports a value T every column it left out stays below, k_sgram_sum forms the EXACT fp32 c0 of the chosen
// columns beside the subset Gram matrix — lambda_0, the first pick and the whole path come from those — and
// k_scr_residuals certifies state 0:   T + eps_0 <= 0.875 lambda_0 - slack,   eps_0 = 2^-9 max ||a_i|| ||y|| + the flush term
// (|c~0 - c0| <= (2^-11 + ldm 2^-24) sum |a||y| <= 2^-9 ||a|| ||y|| for ldm <= 16384; entries below the fp16 normal range:
// 2^-14 per entry in scaled units).  A signal whose state 0 is not certified goes back to the default engine like any other.
// Layout: sweep.hip's — a wave owns CPW columns and streams them with 16-byte loads (8 rows per lane, 512 rows per step);
// y sits in LDS, permuted so that the two 16-byte reads of a lane are conflict-free.  Every group of columns starts at a
// row step of its own and wraps around (the sum's order is free here): the HBM channel phases of the 16-KiB-strided columns.
template <typename TY, int CPW, int DEPTH>
__global__ __launch_bounds__(512, 2)
void k_scr_first(const __half* __restrict__ a16, uint32_t ldm, uint32_t n, uint32_t ngroups, const TY* __restrict__ y,
                 float* __restrict__ meta, float* __restrict__ c0h, uint32_t skew, float* __restrict__ wmax)
{
    // (TY = double: the fp64 form — y is rounded to fp32 on its way into LDS: 2^-24 per entry, inside the bound's 2^-9)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* ly = reinterpret_cast<float*>(smem);                  // [ldm]: rows 512 s + 8 l + 4 u + e  at  512 s + 256 u + 4 l + e
    float* sv = ly + ldm;                                        // [16] reduction scratch
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float ss = 0.f;
    for (uint32_t i = tid * 4u; i < ldm; i += 2048u) {
        scr_v4f v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (float)y[i + (uint32_t)e];
        const uint32_t wq = i & 511u;
        *reinterpret_cast<scr_v4f*>(&ly[(i & ~511u) + ((wq & 4u) << 6) + ((wq >> 3) << 2)]) = v;
#pragma unroll
        for (int e = 0; e < 4; ++e) ss = __builtin_fmaf(v[e], v[e], ss);
    }
    if (blockIdx.x == 0u) {
        ss = block_sum(ss, sv);
        // ([8], [9]: this pass's error model for the certificate of state 0 — |c~0 - c0| <= [8] ||a|| ||y|| + [9] sqrt(ldm) ||y||)
        if (tid == 0u) { meta[5] = ss; meta[8] = 0.0019726562f; meta[9] = 6.103515625e-05f * meta[1]; }
    }
    __syncthreads();
    const float inv_sA = meta[1];
    const uint32_t nsteps = ldm >> 9;
    float wmx = 0.f;                                             // largest |c~0| of this wave's columns: the selection's floor comes from these
    for (uint32_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const uint32_t col0 = g * (8u * CPW) + wave * CPW;
        const char* cb[CPW];
#pragma unroll
        for (int c = 0; c < CPW; ++c) cb[c] = reinterpret_cast<const char*>(a16 + (size_t)(col0 + c) * ldm) + lane * 16u;
        float acc[CPW];
#pragma unroll
        for (int c = 0; c < CPW; ++c) acc[c] = 0.f;
        const uint32_t ts0 = (g * skew + wave) % nsteps;
        scr_u4 a[DEPTH][CPW];
#define F16_ROW(T) ((ts0 + (T)) >= nsteps ? (ts0 + (T)) - nsteps : (ts0 + (T)))
#define F16_LOAD(STAGE, T)                                                                          \
        {                                                                                           \
            const uint32_t rr_ = F16_ROW(T);                                                        \
            _Pragma("unroll") for (int c = 0; c < CPW; ++c)                                         \
                a[STAGE][c] = __builtin_nontemporal_load(reinterpret_cast<const scr_u4*>(cb[c] + (size_t)rr_ * 1024u)); \
        }
#define F16_COMPUTE(STAGE, T)                                                                       \
        {                                                                                           \
            const uint32_t rr_ = F16_ROW(T);                                                        \
            const scr_v4f y0_ = *reinterpret_cast<const scr_v4f*>(&ly[(rr_ << 9) + 4u * lane]);     \
            const scr_v4f y1_ = *reinterpret_cast<const scr_v4f*>(&ly[(rr_ << 9) + 256u + 4u * lane]); \
            _Pragma("unroll") for (int c = 0; c < CPW; ++c) {                                       \
                const scr_h8 h_ = __builtin_bit_cast(scr_h8, a[STAGE][c]);                          \
                _Pragma("unroll") for (int e = 0; e < 4; ++e) acc[c] = __builtin_fmaf((float)h_[e], y0_[e], acc[c]);     \
                _Pragma("unroll") for (int e = 0; e < 4; ++e) acc[c] = __builtin_fmaf((float)h_[4 + e], y1_[e], acc[c]); \
            }                                                                                       \
        }
#pragma unroll
        for (int sidx = 0; sidx < DEPTH - 1; ++sidx)
            if ((uint32_t)sidx < nsteps) F16_LOAD(sidx, (uint32_t)sidx)
        uint32_t t = 0;
        for (; t + (2 * DEPTH - 1) <= nsteps; t += DEPTH) {
#pragma unroll
            for (int sidx = 0; sidx < DEPTH; ++sidx) {
                F16_LOAD((sidx + DEPTH - 1) % DEPTH, t + (uint32_t)(sidx + DEPTH - 1))
                F16_COMPUTE(sidx, t + (uint32_t)sidx)
            }
        }
        for (; t < nsteps; t += DEPTH) {
#pragma unroll
            for (int sidx = 0; sidx < DEPTH; ++sidx) {
                if (t + (uint32_t)(sidx + DEPTH - 1) < nsteps) F16_LOAD((sidx + DEPTH - 1) % DEPTH, t + (uint32_t)(sidx + DEPTH - 1))
                if (t + (uint32_t)sidx < nsteps) F16_COMPUTE(sidx, t + (uint32_t)sidx)
            }
        }
#undef F16_COMPUTE
#undef F16_LOAD
#undef F16_ROW
#pragma unroll
        for (int c = 0; c < CPW; ++c) {
            const float v = wave_sum(acc[c]) * inv_sA;
            const uint32_t col = col0 + (uint32_t)c;
            if (lane == 0u) c0h[col] = col < n ? v : 0.f;
            if (col < n) wmx = fmaxf(wmx, fabsf(v));
        }
    }
    if (wmax != nullptr && lane == 0u) wmax[blockIdx.x * 8u + wave] = wmx;
}

// ---- the first pass over the FP8 copy: c~0 = A8^T y — half the bytes again ---------------------------------------------------------
// What the first pass is for is a RANKING (which columns are worth solving on) and a bound T + eps_0 on what was left out; nothing it
// computes is reported.  e4m3 keeps three mantissa bits: |c~0 - c0| <= (2^-4 + ldm 2^-24) sum |a||y| <= 2^-4 x 1.02 ||a|| ||y|| (ldm <=
// 16384), plus 2^-10 per entry (scaled units) below the normal range — sixteen times the half-precision pass's eps_0, and still a
// fraction of lambda_0 on the signals this form is for (||y|| ~ 4 lambda_0: eps_0 ~ 0.25 lambda_0); where T + eps_0 does not stay below
// the bound, state 0 is left to the exact re-check's list like any column the certificate cannot clear, or the signal goes back.
// Layout as k_scr_first, 16 rows per lane and load: 1024 rows per step; y in LDS so that the four 16-byte reads of a lane are
// conflict-free: row 1024 s + 16 l + 4 q + e at 1024 s + 256 q + 4 l + e.
template <typename TY, int CPW, int DEPTH>
__global__ __launch_bounds__(512, 2)
void k_scr_first8(const uint8_t* __restrict__ a8, uint32_t ldm, uint32_t n, uint32_t ngroups, const TY* __restrict__ y,
                  float* __restrict__ meta, float* __restrict__ c0h, uint32_t skew, float* __restrict__ wmax,
                  long long incy, uint32_t ylen, LaResetArgs<float> reset)
{
    // (y: ylen entries incy apart, zeros beyond — the block the solve staged, incy = 1 and ylen = ldm, or the caller's own vector when
    // this launch is the first of an attempt.  reset: then its workgroups also share out what k_la_reset does, in front of their own work —
    // the clears, and y into the solve's two copies; nothing of that is read before the launch ends: y comes from the caller's pointer)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* ly = reinterpret_cast<float*>(smem);                  // [ldm]
    float* sv = ly + ldm;                                        // [16] reduction scratch
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (reset.x != nullptr) la_reset_share(reset, blockIdx.x * 512u + tid, gridDim.x * 512u);
    const bool packed = incy == 1 && ylen == ldm;                // (uniform)
    float ss = 0.f;
    for (uint32_t i = tid * 4u; i < ldm; i += 2048u) {
        scr_v4f v;
        if (packed) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (float)y[i + (uint32_t)e];
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = i + (uint32_t)e < ylen ? (float)y[(long long)(i + (uint32_t)e) * incy] : 0.f;
        }
        const uint32_t wq = i & 1023u;                           // = 16 l + 4 q
        *reinterpret_cast<scr_v4f*>(&ly[(i & ~1023u) + (((wq >> 2) & 3u) << 8) + ((wq >> 4) << 2)]) = v;
#pragma unroll
        for (int e = 0; e < 4; ++e) ss = __builtin_fmaf(v[e], v[e], ss);
    }
    if (blockIdx.x == 0u) {
        ss = block_sum(ss, sv);
        if (tid == 0u) { meta[5] = ss; meta[8] = 0.06375f; meta[9] = 9.765625e-04f * meta[11]; }
    }
    __syncthreads();
    const float inv_s8 = meta[11];
    const uint32_t nsteps = ldm >> 10;
    float wmx = 0.f;
    for (uint32_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const uint32_t col0 = g * (8u * CPW) + wave * CPW;
        const uint8_t* cb[CPW];
#pragma unroll
        for (int c = 0; c < CPW; ++c) cb[c] = a8 + (size_t)(col0 + c) * ldm + lane * 16u;
        float acc[CPW];
#pragma unroll
        for (int c = 0; c < CPW; ++c) acc[c] = 0.f;
        const uint32_t ts0 = (g * skew + wave) % nsteps;
        scr_u4 a[DEPTH][CPW];
#define F8_ROW(T) ((ts0 + (T)) >= nsteps ? (ts0 + (T)) - nsteps : (ts0 + (T)))
#define F8_LOAD(STAGE, T)                                                                           \
        {                                                                                           \
            const uint32_t rr_ = F8_ROW(T);                                                         \
            _Pragma("unroll") for (int c = 0; c < CPW; ++c)                                         \
                a[STAGE][c] = __builtin_nontemporal_load(reinterpret_cast<const scr_u4*>(cb[c] + (size_t)rr_ * 1024u)); \
        }
#define F8_COMPUTE(STAGE, T)                                                                        \
        {                                                                                           \
            const uint32_t rr_ = F8_ROW(T);                                                         \
            scr_v4f yq_[4];                                                                         \
            _Pragma("unroll") for (int q = 0; q < 4; ++q)                                           \
                yq_[q] = *reinterpret_cast<const scr_v4f*>(&ly[(rr_ << 10) + 256u * (uint32_t)q + 4u * lane]); \
            _Pragma("unroll") for (int c = 0; c < CPW; ++c) {                                       \
                _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                     \
                    const scr_v2f lo_ = __builtin_amdgcn_cvt_pk_f32_fp8((int)a[STAGE][c][q], false); \
                    const scr_v2f hi_ = __builtin_amdgcn_cvt_pk_f32_fp8((int)a[STAGE][c][q], true);  \
                    acc[c] = __builtin_fmaf(lo_[0], yq_[q][0], acc[c]);                             \
                    acc[c] = __builtin_fmaf(lo_[1], yq_[q][1], acc[c]);                             \
                    acc[c] = __builtin_fmaf(hi_[0], yq_[q][2], acc[c]);                             \
                    acc[c] = __builtin_fmaf(hi_[1], yq_[q][3], acc[c]);                             \
                }                                                                                   \
            }                                                                                       \
        }
#pragma unroll
        for (int sidx = 0; sidx < DEPTH - 1; ++sidx)
            if ((uint32_t)sidx < nsteps) F8_LOAD(sidx, (uint32_t)sidx)
        uint32_t t = 0;
        for (; t + (2 * DEPTH - 1) <= nsteps; t += DEPTH) {
#pragma unroll
            for (int sidx = 0; sidx < DEPTH; ++sidx) {
                F8_LOAD((sidx + DEPTH - 1) % DEPTH, t + (uint32_t)(sidx + DEPTH - 1))
                F8_COMPUTE(sidx, t + (uint32_t)sidx)
            }
        }
        for (; t < nsteps; t += DEPTH) {
#pragma unroll
            for (int sidx = 0; sidx < DEPTH; ++sidx) {
                if (t + (uint32_t)(sidx + DEPTH - 1) < nsteps) F8_LOAD((sidx + DEPTH - 1) % DEPTH, t + (uint32_t)(sidx + DEPTH - 1))
                if (t + (uint32_t)sidx < nsteps) F8_COMPUTE(sidx, t + (uint32_t)sidx)
            }
        }
#undef F8_COMPUTE
#undef F8_LOAD
#undef F8_ROW
#pragma unroll
        for (int c = 0; c < CPW; ++c) {
            const float v = wave_sum(acc[c]) * inv_s8;
            const uint32_t col = col0 + (uint32_t)c;
            if (lane == 0u) c0h[col] = col < n ? v : 0.f;
            if (col < n) wmx = fmaxf(wmx, fabsf(v));
        }
    }
    if (wmax != nullptr && lane == 0u) wmax[blockIdx.x * 8u + wave] = wmx;
}

// ---- Gs = A_S^T A_S of the 448 subset columns, from the fp32 A ------------------------------------------------------
// One workgroup per (64 x 64 tile on or above the diagonal, row chunk); a 32 x 32 quadrant per wave on v_mfma_f32_32x32x2_f32;
// the columns' rows staged through LDS 64 at a time (coalesced 256-byte runs per column), the next stage's loads in flight
// under the MFMAs.  Partials per row chunk; mirrored store.
__global__ __launch_bounds__(256)
void k_sgram_part(const float* __restrict__ At, uint32_t ldm, uint32_t n, const uint32_t* __restrict__ sub, uint32_t rows_per,
                  float* __restrict__ part)
{
    // (blockIdx.z = slot of a batch: its subset, its partials)
    sub += (size_t)blockIdx.z * kSbS;
    part += (size_t)blockIdx.z * gridDim.y * kSbS * kSbS;
    __shared__ __attribute__((aligned(16))) float sI[kSgT][kSgPitchF];
    __shared__ __attribute__((aligned(16))) float sJ[kSgT][kSgPitchF];
    constexpr uint32_t NT = kSbS / kSgT;                        // 7 tiles per side
    const uint32_t b = blockIdx.x;
    uint32_t t = (uint32_t)((__fsqrt_rn(8.f * (float)b + 1.f) - 1.f) * 0.5f);
    while (t * (t + 1u) / 2u > b) --t;
    while ((t + 1u) * (t + 2u) / 2u <= b) ++t;
    const uint32_t bj = t, bi = b - t * (t + 1u) / 2u;
    (void)NT;
    const uint32_t chunk = blockIdx.y;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const uint32_t wi = w >> 1, wj = w & 1u;
    const uint32_t sc = tid >> 4, sq = tid & 15u;               // staging: column sc (+16 p) of the 64, float4 sq of the 16 per step
    const float* gi[4];
    const float* gj[4];
    bool oki[4], okj[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const uint32_t ci = sub[bi * kSgT + sc + 16u * (uint32_t)p], cj = sub[bj * kSgT + sc + 16u * (uint32_t)p];
        oki[p] = ci < n; okj[p] = cj < n;
        gi[p] = At + (size_t)(oki[p] ? ci : 0u) * ldm + (size_t)chunk * rows_per + 4u * sq;
        gj[p] = At + (size_t)(okj[p] ? cj : 0u) * ldm + (size_t)chunk * rows_per + 4u * sq;
    }
    const scr_v4f zero4 = { 0.f, 0.f, 0.f, 0.f };
    scr_v4f vi[4], vj[4];
#define SGM_LOAD(R0)                                                                      \
    _Pragma("unroll") for (int p = 0; p < 4; ++p) {                                       \
        vi[p] = oki[p] ? *reinterpret_cast<const scr_v4f*>(gi[p] + (R0)) : zero4;         \
        vj[p] = okj[p] ? *reinterpret_cast<const scr_v4f*>(gj[p] + (R0)) : zero4;         \
    }
    SGM_LOAD(0u)
    scr_v16f acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    const uint32_t r = lane & 31u, h = lane >> 5;
    for (uint32_t r0 = 0; r0 < rows_per; r0 += kSgStep) {
        __syncthreads();
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            *reinterpret_cast<scr_v4f*>(&sI[sc + 16u * (uint32_t)p][4u * sq]) = vi[p];
            *reinterpret_cast<scr_v4f*>(&sJ[sc + 16u * (uint32_t)p][4u * sq]) = vj[p];
        }
        __syncthreads();
        if (r0 + kSgStep < rows_per) SGM_LOAD(r0 + kSgStep)
#pragma unroll
        for (uint32_t k8 = 0; k8 < kSgStep; k8 += 8) {
            const scr_v4f a = *reinterpret_cast<const scr_v4f*>(&sI[32u * wi + r][k8 + 4u * h]);
            const scr_v4f bb = *reinterpret_cast<const scr_v4f*>(&sJ[32u * wj + r][k8 + 4u * h]);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], bb[e], acc, 0, 0, 0);
        }
    }
#undef SGM_LOAD
    float* P = part + (size_t)chunk * kSbS * kSbS;
    const uint32_t gjj = bj * kSgT + 32u * wj + r;
    // (the mirrored tile goes through LDS so that it, too, is written in 256-byte runs: lane-per-row stores of a column would be
    // 4-byte writes 1792 bytes apart)
    float* sT = &sI[0][0];                                        // [64][65]
    constexpr uint32_t TP = kSgT + 1u;
    static_assert(kSgT * (kSgT + 1u) <= kSgT * kSgPitchF, "transpose tile fits the staging buffer");
    if (bi != bj) __syncthreads();                                // (uniform: the last step's operand reads are done)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const uint32_t li = 32u * wi + (uint32_t)(e & 3) + 8u * (uint32_t)(e >> 2) + 4u * h;
        P[(size_t)(bi * kSgT + li) * kSbS + gjj] = acc[e];
        if (bi != bj) sT[li * TP + 32u * wj + r] = acc[e];
    }
    if (bi != bj) {
        __syncthreads();
        for (uint32_t c = w; c < kSgT; c += 4u)
            P[(size_t)(bj * kSgT + c) * kSbS + bi * kSgT + lane] = sT[lane * TP + c];
    }
}

__global__ __launch_bounds__(256)
void k_sgram_sum(const float* __restrict__ part, uint32_t nsplit, float* __restrict__ gs, const float* __restrict__ At, uint32_t ldm,
                 const float* __restrict__ y, const uint32_t* __restrict__ sub, uint32_t n, float* __restrict__ c0)
{
    constexpr uint32_t NB = (kSbS * kSbS + 255u) / 256u;
    if (blockIdx.x >= NB) {
        // Workgroups beyond the sum (one signal whose first pass ran in half precision: k_scr_first): the EXACT fp32 c0 = a_j . y
        // of one subset column each — the tiles have just read those columns — written where k_sub_solve reads it.  A thread owns
        // the float4s 256 apart (8 loads in flight per round), the workgroup's sum in the fixed order of block_sum.
        __shared__ float sv[16];
        const uint32_t col = sub[blockIdx.x - NB];
        const float* a = At + (size_t)(col < n ? col : 0u) * ldm;
        float acc = 0.f;
        for (uint32_t r0 = 4u * threadIdx.x; r0 < ldm; r0 += 8u * 1024u) {
            scr_v4f av[8], yv[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const uint32_t r = r0 + 1024u * (uint32_t)q;
                av[q] = r < ldm ? *reinterpret_cast<const scr_v4f*>(a + r) : scr_v4f{ 0.f, 0.f, 0.f, 0.f };
                yv[q] = r < ldm ? *reinterpret_cast<const scr_v4f*>(y + r) : scr_v4f{ 0.f, 0.f, 0.f, 0.f };
            }
#pragma unroll
            for (int q = 0; q < 8; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc = __builtin_fmaf(av[q][e], yv[q][e], acc);
        }
        acc = block_sum(acc, sv);
        if (threadIdx.x == 0u && col < n) c0[col] = acc;
        return;
    }
    part += (size_t)blockIdx.y * nsplit * kSbS * kSbS;           // (blockIdx.y = slot of a batch)
    gs += (size_t)blockIdx.y * kSbS * kSbS;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= kSbS * kSbS) return;
    float s = part[i];
    for (uint32_t c = 1; c < nsplit; ++c) s += part[(size_t)c * kSbS * kSbS + i];
    gs[i] = s;
}

// ---- r_k = y - A_S x_S(k) of every logged state k >= 1, scaled and rounded to fp16 -----------------------------------
// One workgroup per 64 rows: the support's columns' 64 rows and the coefficient table (transposed: [position][state]) in
// LDS; a thread owns 4 rows x 4 states (two 16-byte LDS reads per 16 fmas), states beyond 64 in a second round.
// ||r_k||^2 leaves as one partial per (workgroup, state) — summed in a fixed order by the screening pass.  Workgroup 0
// also writes the per-state table.  (Positions >= P_k carry x = 0 in the log: every state runs over all positions.)
__device__ __forceinline__ float scr_state_scale(float lam_eff)
{
    int e = 12;
    if (lam_eff > 0.f && lam_eff < 3.0e38f) e = (int)floorf(log2f(4096.f / lam_eff));
    e = e < -100 ? -100 : (e > 100 ? 100 : e);
    return ldexpf(1.f, e);
}

__global__ __launch_bounds__(256)
void k_scr_residuals(const float* __restrict__ At, uint32_t ldm, uint32_t n, const float* __restrict__ y,
                     const uint32_t* __restrict__ hdr, const uint32_t* __restrict__ pcol,
                     const float* __restrict__ LX, float tol, const float* __restrict__ meta, __half* __restrict__ r16,
                     float* __restrict__ rn2p, float* __restrict__ tab, uint32_t* __restrict__ headroom, DevState* __restrict__ st,
                     int first16, uint32_t* __restrict__ fl, int omp = 0, int scan = 0)
{
    // scan (the RESCUE of a declined solve, launch_screen_rescue_scan): the log of a solve that was declined — it ran out of positions, or
    // a column outside the subset beat a state — is examined once more: the residuals of its states are formed as usual (irregular states
    // are switched off), nothing is written to the slot's state; k_scr_gemm (gate 3) then lists the columns the ranking missed.
    // fl (one signal, may be null): the list of columns left to the exact re-check (k_scr_recheck) — cleared here; a state 0 the
    // half-precision first pass cannot certify by its threshold alone is left to that list too (its columns are found by k_scr_gemm)
    __shared__ __attribute__((aligned(16))) float sAc[kSbRows][64];
    __shared__ __attribute__((aligned(16))) float sXt[kSbRows][kSbLog];
    __shared__ float sS[kSbLog];
    {   // (blockIdx.y = slot of a batch: its signal, its log, its block of residuals)
        const uint32_t slot = blockIdx.y;
        y += (size_t)slot * ldm;
        hdr += (size_t)slot * kSbLog * 8;
        pcol += (size_t)slot * kSbRows;
        LX += (size_t)slot * kSbLog * kSbRows;
        r16 += (size_t)slot * kScrRhs * ldm;
        rn2p += (size_t)slot * (ldm / 64u) * kScrRhs;
        tab += (size_t)slot * kScrRhs * kScrTab;
        st += slot;
    }
    // Everything this workgroup needs from the slot's state and log is requested in ONE burst, ahead of the first wait: the status and the
    // number of states, the columns of ALL of the thread's gather slots (positions at or beyond Pfin hold 0xffffffff or a stale column:
    // their rows are staged and never read), the scale's header words, the coefficient table.  The columns' rows and Pfin follow in a
    // second burst.  No load stands behind a condition on loaded data (the compiler would wait per load): addresses are clamped into the
    // slot's own buffers, values are selected afterwards.  Two dependent trips to memory where the gather loop made one per trip and load.
    const uint32_t tid = threadIdx.x;
    constexpr uint32_t kGather = (kSbRows + 15u) / 16u;                              // gather slots of a thread: positions (tid >> 4) + 16 t
    constexpr uint32_t kTabLoads = (kSbLog * kSbRows + 255u) / 256u;
    const uint32_t status = st->status;
    const uint32_t nlog = st->solo_nlog;
    uint32_t gcol[kGather];
#pragma unroll
    for (uint32_t t = 0; t < kGather; ++t) gcol[t] = pcol[min((tid >> 4) + 16u * t, kSbRows - 1u)];
    const uint32_t* const hh_own = hdr + (size_t)(min(tid, kSbLog - 2u) + 1u) * 8u;  // (the header of state tid + 1, read below by tid < nst)
    const uint32_t hh_flags = hh_own[1], hh_lam = hh_own[4];
    float tabv[kTabLoads];
#pragma unroll
    for (uint32_t t = 0; t < kTabLoads; ++t) tabv[t] = LX[(size_t)kSbRows + min(tid + 256u * t, (kSbLog - 1u) * kSbRows - 1u)];
    scr_v4f gv[kGather];
#pragma unroll
    for (uint32_t t = 0; t < kGather; ++t)
        gv[t] = *reinterpret_cast<const scr_v4f*>(At + (size_t)(gcol[t] < n ? gcol[t] : 0u) * ldm + blockIdx.x * 64u + 4u * (tid & 15u));
    const uint32_t Pfin = hdr[(size_t)(min(max(nlog, 1u), kSbLog) - 1u) * 8u];
    const scr_v4f yv = *reinterpret_cast<const scr_v4f*>(y + blockIdx.x * 64u + 4u * (tid & 15u));   // (rows m .. ldm - 1 of y and of A are zero)
    if (status != 0u && !scan) return;
    float ratio0 = 0.f;
    if (fl != nullptr && blockIdx.x == 0u && blockIdx.y == 0u && tid == 0u) {
        fl[0] = 0u; fl[kScrFlCap + 1u] = 0u; fl[kScrFlCap + 4u] = 0u;
        fl[kScrFlCap + 12u] = 0u;                                                   // (the last step's repair: no candidate yet)
        fl[kScrFlCap + 13u] = 0u;                                                   // (the rescue scan's second list)
        if (!scan) fl[kScrFlCap + 14u] = 0u;                                        // (the re-check's list of failed columns: a scan leaves the first attempt's alone)
    }
    if (first16 && !scan && blockIdx.x == 0u && tid == 0u) {
        // state 0 after a first pass in half precision (k_scr_first): every column left out of the subset has |c~0| < T, so
        // |c0| < T + eps_0 — certified against lambda_0 (the subset's exact max |c0|) with the margin of every other state
        const float lam0 = st->lambda0;
        const float yn = sqrtf(meta[5]) * 1.001f;
        const float eps0 = meta[8] * yn * meta[4] + meta[9] * sqrtf((float)ldm) * yn;          // (the first pass's own error model)
        const float bound0 = lam0 * 0.875f - 1e-5f * lam0;
        const float v0 = meta[6] + eps0;
        if (!(v0 <= bound0)) {
            if (fl != nullptr && bound0 > 0.f) { fl[kScrFlCap + 1u] = 1u; fl[kScrFlCap + 2u] = __float_as_uint(bound0); fl[kScrFlCap + 3u] = __float_as_uint(eps0); }
            else { __hip_atomic_store(&st->need_sweep, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); atomicOr(&st->sub_reason, kReasonFirstState); }
        }
        ratio0 = bound0 > 0.f && v0 == v0 ? v0 / bound0 : 3.0e38f;
    }
    if (nlog < 2u) {
        if (blockIdx.x == 0u && tid == 0u && blockIdx.y == 0u) *headroom = __float_as_uint(ratio0);
        return;
    }
    const uint32_t nst = nlog - 1u;
    const uint32_t r0 = blockIdx.x * 64u;
#pragma unroll
    for (uint32_t t = 0; t < kTabLoads; ++t) {
        const uint32_t e = tid + 256u * t;
        const uint32_t kk = e / kSbRows, p = e - kk * kSbRows;
        if (e < kSbLog * kSbRows) sXt[p][kk] = kk < nst ? tabv[t] : 0.f;       // (state k = kk + 1)
    }
    if (tid < kSbLog) {
        float sc = 1.f;
        if (tid < nst) {
            const float lam = __uint_as_float(hh_lam);
            const bool final_state = !(hh_flags & 1u);
            sc = scr_state_scale(final_state ? fmaxf(lam, tol) : lam);
        }
        sS[tid] = sc;
    }
#pragma unroll
    for (uint32_t t = 0; t < kGather; ++t) {
        const uint32_t p = (tid >> 4) + 16u * t;
        if (p < kSbRows) *reinterpret_cast<scr_v4f*>(&sAc[p][4u * (tid & 15u)]) = gcol[t] < n ? gv[t] : scr_v4f{ 0.f, 0.f, 0.f, 0.f };
    }
    __syncthreads();
    const uint32_t rg = tid & 15u, sgp = tid >> 4;
    bool ovf = false;
    for (uint32_t s0 = 4u * sgp; s0 < nst; s0 += 64u) {
        scr_v4f acc[4] = { yv, yv, yv, yv };
        for (uint32_t p = 0; p < Pfin; ++p) {
            const scr_v4f a4 = *reinterpret_cast<const scr_v4f*>(&sAc[p][4u * rg]);
            const scr_v4f x4 = *reinterpret_cast<const scr_v4f*>(&sXt[p][s0]);
#pragma unroll
            for (int si = 0; si < 4; ++si)
#pragma unroll
                for (int ri = 0; ri < 4; ++ri) acc[si][ri] = __builtin_fmaf(-x4[si], a4[ri], acc[si][ri]);
        }
#pragma unroll
        for (int si = 0; si < 4; ++si) {
            const uint32_t kk = s0 + (uint32_t)si;                    // (uniform over the 16 lanes of a state group)
            float ss = 0.f;
            const float sc = sS[kk < kSbLog ? kk : 0u];
            __half hv[4];
#pragma unroll
            for (int ri = 0; ri < 4; ++ri) {
                const float r = acc[si][ri];
                ss = __builtin_fmaf(r, r, ss);
                const float v = r * sc;
                if (kk < nst && !(fabsf(v) < 60000.f)) ovf = true;
                hv[ri] = __float2half_rn(v);
            }
            ss += __shfl_xor(ss, 1); ss += __shfl_xor(ss, 2); ss += __shfl_xor(ss, 4); ss += __shfl_xor(ss, 8);
            if (kk < nst) {
                *reinterpret_cast<uint2*>(r16 + (size_t)kk * ldm + r0 + 4u * rg) = *reinterpret_cast<const uint2*>(hv);
                if (rg == 0u) rn2p[(size_t)blockIdx.x * kScrRhs + kk] = ss;
            }
        }
    }
    if (ovf && !scan) { __hip_atomic_store(&st->need_sweep, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); atomicOr(&st->sub_reason, kReasonOverflow); }
    if (blockIdx.x == 0u) {
        const float lam0 = st->lambda0;
        if (tid == 0u && blockIdx.y == 0u) *headroom = __float_as_uint(ratio0);
        if (tid < nst) {
            const uint32_t* hh = hdr + (size_t)(tid + 1u) * 8u;
            const float lam = __uint_as_float(hh[4]);
            const bool final_state = !(hh[1] & 1u);
            const float slack = 1e-5f * lam0;
            // where the step INTO this state left lambda: lambda_{k-1} - gamma_{k-1}.  On a regular path that is lambda_k; on a
            // derailed one (the first-step sign quirk) max |c| can sit above it — and the candidate test of that step compares
            // the column's next correlation with lambda_{k-1} - gamma_{k-1}, not with max |c|: the smaller of the two counts
            const uint32_t* hp = hdr + (size_t)tid * 8u;
            const float lam_exp = __uint_as_float(hp[4]) - __uint_as_float(hp[5]);
            // The state a path ends in by tolerance.  If the last step landed on lambda = 0 within rounding (the least-squares jump
            // of a noise-free path) every column's candidate ties with it — whichever the reference inserts enters with x = 0
            //  — and what is left to certify is that nothing out there keeps the path going: |c| <= tolerance.
            // Otherwise (noise: the path crosses the tolerance on a regular step) that step is certified like any other.
            const bool ls_jump = final_state && !(lam > tol) && !(lam_exp > 2e-6f * lam0);
            float bound;
            if (omp) bound = (final_state && !(lam > tol) ? tol * 0.9375f : lam * 0.875f) - slack;      // (OMP: the pick is the largest |c| — nothing outside may reach it; the state it ends in: the tolerance)
            else if (ls_jump) bound = tol * 0.9375f - slack;
            else bound = fminf(lam, lam_exp) * 0.875f - slack;
            // only REGULAR paths are certified: every step inserts a column and lambda goes down.  On a path with removals, or one
            // the first-step sign quirk has derailed, steps of rounding size decide what is toggled next, and the subset's Gram
            // matrix is the default engine's only to rounding (see k_s64_dense): those go back to that engine
            const bool irregular = !omp && (hp[3] == 0u || lam > __uint_as_float(hp[4]) * 1.00001f);
            if (irregular && !scan) {
                bound = -1.f;
                atomicOr(&st->sub_reason, kReasonIrregular);
                __hip_atomic_store(&st->need_sweep, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // (the screening pass does not run for it)
            }
            if (scan && (irregular || final_state)) bound = 3.0e38f;
            const float inv_sk = 1.f / sS[tid];
            tab[tid * kScrTab + 0] = meta[1] * inv_sk;
            tab[tid * kScrTab + 1] = bound;
            tab[tid * kScrTab + 2] = inv_sk;
            tab[tid * kScrTab + 3] = lam;
        }
    }
}

// ---- the screening pass: C~ = A16^T R16 and the test of every (column outside the subset, state) -------------------
// Workgroup = 128 dictionary columns x up to 96 right-hand sides; wave = 32 columns x 2 or 3 MFMA tiles of 32 states (the
// third only when the path logged more than 64 states).  A stage is 128 rows: 32 KB of A16 and 16 / 24 KB of R16 (from
// L2) land in LDS by 16-byte stores of coalesced 256-byte runs; TWO stages of loads are in flight (two register sets)
// under the MFMAs of a third — no load of the stage loop stands behind a condition, or the compiler's waits drain them (see the loop).
// HBM-bound: 1.07 GB at 8192 x 65536.
template <int NT>
__global__ __launch_bounds__(256, 2)
void k_scr_gemm(const __half* __restrict__ a16, uint32_t ldm, uint32_t n, const __half* __restrict__ r16,
                const float* __restrict__ anorm, const float* __restrict__ rn2p, uint32_t rn_pitch, const float* __restrict__ tab,
                const uint32_t* __restrict__ sub, uint32_t nsub, const float* __restrict__ meta, DevState* __restrict__ st,
                uint32_t* __restrict__ headroom, uint32_t nst_fixed, uint32_t skew, uint32_t gate, uint32_t* __restrict__ fl = nullptr,
                const float* __restrict__ c0h = nullptr, float* __restrict__ out_abs = nullptr, uint32_t out_pitch = 0)
{
    // out_abs (the first pass of an fp64 BATCH, nst_fixed right-hand sides = signals rounded to fp16): no certificate — the launch writes
    // |c~| = |A16^T y16| / (sA s_y) of every (signal, column) to out_abs[signal * out_pitch + column]: the ranking of each signal's columns
    // fl (one fp32 signal, may be null): a column this pass cannot certify is APPENDED to the list of the exact re-check
    // (k_scr_recheck) instead of failing the signal; c0h: the half-precision first pass's c~0 — when state 0 was left to the list
    // (fl[cap + 1]) every column with |c~0| + eps_0 above the bound joins it
    // gate (states from the slot's log only): 1 = this launch only if the log holds <= 128 states, 2 = only if more (the fp64
    // resident form queues a four-tile and a five-tile launch without the host knowing the path's length)
    // grid = (slots, column tiles): the workgroups of one tile of A16 — one per slot of a batch — are neighbours in the launch
    // order, so the tile comes from HBM once and from L2 for the others (one slot: a plain 1 x tiles grid)
    {
        const uint32_t slot = blockIdx.x;
        r16 += (size_t)slot * kScrRhs * ldm;
        rn2p += (size_t)slot * (ldm / 64u) * rn_pitch;
        tab += (size_t)slot * kScrRhs * kScrTab;
        sub += (size_t)slot * nsub;
        st += slot;
    }
    // NT: tiles of 32 states a workgroup carries — 3 (two register sets of loads in flight), or 5 for the fp64 form's longer paths
    // (160 states in ONE pass over the fp16 copy; one register set).
    // nst_fixed = 0: the fp32 form — the number of states and the go-ahead come from the slot's state (k_sub_solve's log);
    // > 0: that many states (<= 32 NT) of the caller's block of right-hand sides (the fp64 form: r16, rn2p, tab point at it)
    constexpr int RH = 32 * NT, NPR = 2 * NT;
    constexpr bool TWO = NT <= 4;                               // (4 tiles: 128 states — configs[4] — with two register sets)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t nst = nst_fixed;
    if (nst_fixed == 0u || nst_fixed == 0xffffffffu) {
        // (gate = 3: the rescue's scan of a DECLINED solve's log — launch_screen_rescue_scan; nothing of the slot's state is read as a verdict or written)
        if (st->status != 0u && gate != 3u) return;
        if (fl != nullptr && st->need_sweep != 0u && gate != 3u) return;        // (already failed — an irregular path, an overflow: no pass for it)
        const uint32_t nlog = st->solo_nlog;
        if (nlog < 2u) return;
        nst = nlog - 1u;
        if (nst_fixed == 0xffffffffu && nst <= 64u) return;     // (batch chunk: k_scr_gemm_b carries the slots of up to 64 states)
        if ((gate == 1u && nst > 128u) || (gate == 2u && nst <= 128u)) return;
        if (nst > 32u * (uint32_t)NT && gate == 3u) nst = 32u * (uint32_t)NT;
        if (nst > 32u * (uint32_t)NT) {                           // (more states than this launch carries: nothing is certified)
            if (threadIdx.x == 0 && blockIdx.y == 0) { __hip_atomic_store(&st->need_sweep, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); atomicOr(&st->sub_reason, kReasonLog); }
            return;
        }
    }
    const uint32_t ntu = (nst + 31u) / 32u;                      // (uniform) tiles of states in use
    unsigned char* sA = smem;                                   // [128][272]
    unsigned char* sR = smem + (size_t)kScrCols * kScrPitchB;   // [32 NT][272]
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const uint32_t col0 = blockIdx.y * kScrCols;
    const uint32_t lc = tid >> 4, piece = tid & 15u;
    // Buffer loads: a load's address = a descriptor of the workgroup's 128 columns of A16 (of the slot's 32 NT rows of R16) plus a scalar
    // byte offset — row of 16 columns, stage — plus ONE 32-bit byte offset per thread, its column of the 16 and its 16-byte piece.  No
    // 64-bit address per load is kept in registers: with every load of the loop unconditional the compiler would hold all of them.
    const __amdgpu_buffer_rsrc_t ga = __builtin_amdgcn_make_buffer_rsrc(const_cast<__half*>(a16 + (size_t)col0 * ldm), 0, (int)(kScrCols * ldm * 2u), 0x00020000);
    const __amdgpu_buffer_rsrc_t gr = __builtin_amdgcn_make_buffer_rsrc(const_cast<__half*>(r16), 0, (int)(32u * (uint32_t)NT * ldm * 2u), 0x00020000);
    const uint32_t goff = 2u * (lc * ldm + 8u * piece);
    scr_u4 pa0[8], pr0[NPR], pa1[TWO ? 8 : 1], pr1[TWO ? NPR : 1];
    // (NTU_: the tiles in use where the macros stand — a constant of each body)
#define SCR_LOAD(PA, PR, R0)                                                                                      \
    {                                                                                                             \
        _Pragma("unroll") for (int i = 0; i < 8; ++i)                                                             \
            PA[i] = __builtin_bit_cast(scr_u4, __builtin_amdgcn_raw_buffer_load_b128(ga, goff, 2u * ((uint32_t)(16 * i) * ldm + (R0)), 2 /* nt */)); \
        _Pragma("unroll") for (int i = 0; i < NPR; ++i)                                                           \
            if ((uint32_t)(i / 2) < NTU_)                                                                         \
                PR[i] = __builtin_bit_cast(scr_u4, __builtin_amdgcn_raw_buffer_load_b128(gr, goff, 2u * ((uint32_t)(16 * i) * ldm + (R0)), 0)); \
    }
    scr_v16f acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
    const uint32_t r = lane & 31u, h = lane >> 5;
    const unsigned char* rdA = sA + (size_t)(32u * w + r) * kScrPitchB + 16u * h;
    const unsigned char* rdR = sR + (size_t)r * kScrPitchB + 16u * h;
    // (the barriers wait for LDS only: a set's loads are waited for where its registers go to LDS, and no sooner)
#define SCR_STAGE(PA, PR, RELOAD)                                                                                 \
    {                                                                                                             \
        __builtin_amdgcn_sched_barrier(0);      /* (no MFMA of the stage before is moved behind the barriers, in front of the reload) */ \
        lds_barrier();                                                                                            \
        _Pragma("unroll") for (int i = 0; i < 8; ++i)                                                             \
            *reinterpret_cast<scr_u4*>(sA + (size_t)(lc + 16u * (uint32_t)i) * kScrPitchB + 16u * piece) = PA[i]; \
        _Pragma("unroll") for (int i = 0; i < NPR; ++i)                                                           \
            if ((uint32_t)(i / 2) < NTU_)                                                                         \
                *reinterpret_cast<scr_u4*>(sR + (size_t)(lc + 16u * (uint32_t)i) * kScrPitchB + 16u * piece) = PR[i]; \
        lds_barrier();                                                                                            \
        RELOAD                                                                                                    \
        __builtin_amdgcn_sched_barrier(0);      /* (the loads go out in front of the MFMAs, not among them) */    \
        _Pragma("unroll") for (uint32_t ks = 0; ks < kScrKc / 16u; ++ks) {                                        \
            const scr_h8 bq = *reinterpret_cast<const scr_h8*>(rdA + 32u * ks);                                   \
            _Pragma("unroll") for (int t = 0; t < NT; ++t) {                                                      \
                if ((uint32_t)t < NTU_) {                                                                         \
                    const scr_h8 aq = *reinterpret_cast<const scr_h8*>(rdR + (size_t)(32 * t) * kScrPitchB + 32u * ks); \
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(aq, bq, acc[t], 0, 0, 0);                     \
                }                                                                                                 \
            }                                                                                                     \
        }                                                                                                         \
    }
#define SCR_NONE
    // (ldm is a multiple of 256: an even number of stages.)  Every workgroup starts at a row offset of its own and wraps
    // around — the sum's order is free here — so that the 512 workgroups do not walk the same 256-byte phase of their
    // 16-KiB-strided columns together (the HBM channels are selected by those address bits)
    const uint32_t nstage = ldm / kScrKc;
    const uint32_t sbase = (blockIdx.y * skew) % nstage;
#define SCR_ROW(S) ((sbase + (S) >= nstage ? sbase + (S) - nstage : sbase + (S)) * kScrKc)
    if constexpr (TWO) {
        // Two register sets, each reloaded for the stage two ahead as soon as it is in LDS.  No load of the loop stands behind a
        // condition — the tile count is a constant of the body (one uniform branch in front selects it) and the last two stages,
        // which reload nothing, are written out behind the loop — so a set is 8 + 2 NTU_ loads and the wait in front of its LDS
        // writes, vmcnt(2 (8 + 2 NTU_) - 1 .. 8 + 2 NTU_), leaves every load of the younger set in flight.
        auto stages = [&](auto ntu_c) __attribute__((always_inline)) {
            constexpr uint32_t NTU_ = decltype(ntu_c)::value;
            asm volatile("; k_scr_gemm: %0 tiles in use" :: "n"(NTU_));   // (keeps the bodies apart: their common first loads are not merged in front of the branch)
            SCR_LOAD(pa0, pr0, SCR_ROW(0u))
            SCR_LOAD(pa1, pr1, SCR_ROW(1u))
            for (uint32_t sidx = 0; sidx + 2u < nstage; sidx += 2u) {
                SCR_STAGE(pa0, pr0, SCR_LOAD(pa0, pr0, SCR_ROW(sidx + 2u)))
                SCR_STAGE(pa1, pr1, SCR_LOAD(pa1, pr1, SCR_ROW(sidx + 3u)))
            }
            SCR_STAGE(pa0, pr0, SCR_NONE)
            SCR_STAGE(pa1, pr1, SCR_NONE)
        };
        if (ntu <= 1u) stages(std::integral_constant<uint32_t, 1u>{});
        else if (ntu == 2u) stages(std::integral_constant<uint32_t, 2u>{});
        else if (NT == 3 || ntu == 3u) stages(std::integral_constant<uint32_t, 3u>{});
        else if constexpr (NT >= 4) stages(std::integral_constant<uint32_t, 4u>{});
    } else {
        // Five tiles: one register set — a second does not fit the registers of two workgroups per CU — reloaded behind its own stage
        // with the loop as it was: the tile count read in the loop, plain loads, __syncthreads().  (With the statements of the
        // bodies above this instantiation measured 7 % SLOWER, 118 against 110 us at 4096 x 16384 with 136 states.)
        const __half* ga5 = a16 + (size_t)(col0 + lc) * ldm + 8u * piece;
        const __half* gr5 = r16 + (size_t)lc * ldm + 8u * piece;
#define SCR5_LOAD(R0)                                                                                             \
    {                                                                                                             \
        _Pragma("unroll") for (int i = 0; i < 8; ++i)                                                             \
            pa0[i] = __builtin_nontemporal_load(reinterpret_cast<const scr_u4*>(ga5 + (size_t)(16 * i) * ldm + (R0))); \
        _Pragma("unroll") for (int i = 0; i < NPR; ++i)                                                           \
            if ((uint32_t)(i / 2) < ntu) pr0[i] = *reinterpret_cast<const scr_u4*>(gr5 + (size_t)(16 * i) * ldm + (R0)); \
    }
        SCR5_LOAD(SCR_ROW(0u))
        for (uint32_t sidx = 0; sidx < nstage; ++sidx) {
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 8; ++i)
                *reinterpret_cast<scr_u4*>(sA + (size_t)(lc + 16u * (uint32_t)i) * kScrPitchB + 16u * piece) = pa0[i];
#pragma unroll
            for (int i = 0; i < NPR; ++i)
                if ((uint32_t)(i / 2) < ntu)
                    *reinterpret_cast<scr_u4*>(sR + (size_t)(lc + 16u * (uint32_t)i) * kScrPitchB + 16u * piece) = pr0[i];
            __syncthreads();
            if (sidx + 1u < nstage) SCR5_LOAD(SCR_ROW(sidx + 1u))
#pragma unroll
            for (uint32_t ks = 0; ks < kScrKc / 16u; ++ks) {
                const scr_h8 bq = *reinterpret_cast<const scr_h8*>(rdA + 32u * ks);
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    if ((uint32_t)t < ntu) {
                        const scr_h8 aq = *reinterpret_cast<const scr_h8*>(rdR + (size_t)(32 * t) * kScrPitchB + 32u * ks);
                        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(aq, bq, acc[t], 0, 0, 0);
                    }
                }
            }
        }
#undef SCR5_LOAD
    }
#undef SCR_ROW
#undef SCR_NONE
#undef SCR_STAGE
#undef SCR_LOAD
    // ---- epilogue: the per-state table and the subset's columns into LDS, then every (column, state) of this wave ------
    __syncthreads();
    if (out_abs != nullptr) {
        const uint32_t colw = col0 + 32u * w + r;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const uint32_t kk = 32u * (uint32_t)t + (uint32_t)(e & 3) + 8u * (uint32_t)(e >> 2) + 4u * h;
                if (kk < nst) out_abs[(size_t)kk * out_pitch + colw] = colw < n ? fabsf(acc[t][e]) * tab[kk * kScrTab] : 0.f;
            }
        }
        return;
    }
    constexpr uint32_t PB = NT <= 3 ? 128u : 64u;               // workgroups' partials staged at a time
    float* sT = reinterpret_cast<float*>(smem);                 // [32 NT][4]: 1/(sA s_k), bound, eps factor 1 (x ||a||), eps term 2
    uint32_t* sSub = reinterpret_cast<uint32_t*>(smem) + (uint32_t)RH * 4u;   // [nsub] the subset's columns, ascending (0xffffffff: none)
    float* sPart = reinterpret_cast<float*>(smem) + (uint32_t)RH * 4u + nsub; // [PB][32 NT] partial sums of ||r_k||^2
    // (meta[12] = 2^-u, 1 in an fp32 context: rn2p and the table are in the units of 2^-u A — k_s64_residuals, k_res_residuals64)
    const float inv_sA = meta[1] * meta[12];
    const float sq_ldm = sqrtf((float)ldm);
    const uint32_t nblk = ldm / 64u;
    // (128 workgroups' partials in flight at once, summed per state in the order of the workgroups that wrote them: deterministic)
    float s2 = 0.f;
    for (uint32_t b0 = 0; b0 < nblk; b0 += PB) {
        const uint32_t nb = nblk - b0 < PB ? nblk - b0 : PB;
        for (uint32_t e = tid; e < nb * (uint32_t)RH; e += 256u) { const uint32_t b = e / (uint32_t)RH, k = e - b * (uint32_t)RH; sPart[e] = rn2p[(size_t)(b0 + b) * rn_pitch + k]; }
        __syncthreads();
        if (tid < nst)
            for (uint32_t b = 0; b < nb; ++b) s2 += sPart[(size_t)b * RH + tid];
        __syncthreads();
    }
    if (tid < (uint32_t)RH) {
        float f0 = 0.f, f1 = 0.f, f2 = 0.f, f3 = 0.f;
        if (tid < nst) {
            const float rn = sqrtf(s2) * 1.001f;
            const float inv_sk = tab[tid * kScrTab + 2];
            f0 = tab[tid * kScrTab + 0];
            f1 = tab[tid * kScrTab + 1];
            f2 = 0.0019726562f * rn + 6.103515625e-05f * sq_ldm * inv_sk;       // x ||a_i||:  2^-9 (+ 1 %) ||r_k|| + 2^-14 sqrt(ldm) / s_k
            f3 = 6.103515625e-05f * sq_ldm * rn * inv_sA;                        // 2^-14 sqrt(ldm) ||r_k|| / sA
        }
        sT[tid * 4 + 0] = f0; sT[tid * 4 + 1] = f1; sT[tid * 4 + 2] = f2; sT[tid * 4 + 3] = f3;
    }
    for (uint32_t e = tid; e < nsub; e += 256u) sSub[e] = sub[e];
    __syncthreads();
    const uint32_t col = col0 + 32u * w + r;
    // is the column in the subset (k_sub_solve dealt with those)?  lower bound in the ascending list
    uint32_t lo = 0, hi = nsub;
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (sSub[mid] < col) lo = mid + 1u; else hi = mid; }
    const bool mine = col < n && !(lo < nsub && sSub[lo] == col);
    const float an = anorm[col < n ? col : 0u] * meta[12];
    bool flag = false;
    float worst = 0.f, big = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const uint32_t kk = 32u * (uint32_t)t + (uint32_t)(e & 3) + 8u * (uint32_t)(e >> 2) + 4u * h;
            if (kk < nst) {
                const scr_v4f T4 = *reinterpret_cast<const scr_v4f*>(&sT[kk * 4u]);
                const float v = fabsf(acc[t][e]) * T4[0] + (an * T4[2] + T4[3]);
                big = fmaxf(big, fabsf(acc[t][e]) * T4[0]);
                if (!(v <= T4[1])) flag = true;
                const float ratio = T4[1] > 0.f ? v / T4[1] : 3.0e38f;
                worst = fmaxf(worst, ratio == ratio ? ratio : 3.0e38f);
            }
        }
    }
    // (the rescue's scan: a column the ranking MISSED beats a state's bound and, somewhere on the path, stands above everything that was
    // ranked out at state 0 — meta[6], the selection's threshold; a noise column that only beats the small bounds of the late states does not)
    if (gate == 3u) {
        // two lists: [1 .. cap / 2] the columns of that kind, [cap / 2 + 1 .. cap] every other column that beats a state (count at [cap + 13]): on a
        // noisy signal the columns of the noise floor that enter the reference's path near its end are of the second kind, and few
        if (mine && flag) {
            if (big >= meta[6]) { const uint32_t at = atomicAdd(&fl[0], 1u); if (at < kScrFlCap / 2u) fl[1u + at] = col; }
            else { const uint32_t at = atomicAdd(&fl[kScrFlCap + 13u], 1u); if (at < kScrFlCap / 2u) fl[1u + kScrFlCap / 2u + at] = col; }
        }
        return;
    }
    if (fl != nullptr && c0h != nullptr && fl[kScrFlCap + 1u] != 0u && mine) {
        const float v0 = fabsf(c0h[col]) + __uint_as_float(fl[kScrFlCap + 3u]);
        if (!(v0 <= __uint_as_float(fl[kScrFlCap + 2u]))) flag = true;
    }
    if (mine && flag) {
        if (fl != nullptr) {
            const uint32_t at = atomicAdd(&fl[0], 1u);
            if (at < kScrFlCap) fl[1u + at] = col;
        } else {
            __hip_atomic_store(&st->need_sweep, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (read by k_sub_finish)
            if (!(__hip_atomic_load(&st->sub_reason, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & kReasonColumn)) atomicOr(&st->sub_reason, kReasonColumn);
        }
    }
    if (!mine) worst = 0.f;
    worst = fmaxf(worst, __shfl_xor(worst, 1)); worst = fmaxf(worst, __shfl_xor(worst, 2)); worst = fmaxf(worst, __shfl_xor(worst, 4));
    worst = fmaxf(worst, __shfl_xor(worst, 8)); worst = fmaxf(worst, __shfl_xor(worst, 16)); worst = fmaxf(worst, __shfl_xor(worst, 32));
    if (lane == 0u && worst > 0.f && gate != 3u) atomicMax(headroom, __float_as_uint(worst));
}

// ---- the rescue's ranking: |c~0| of every column, the columns the scan listed on top ---------------------------------------------
__global__ __launch_bounds__(256)
void k_scr_rescue_rank(const float* __restrict__ c0h, const uint32_t* __restrict__ fl, uint32_t first, uint32_t cnt1, uint32_t first2, uint32_t cnt2,
                       uint32_t n, uint32_t n_pad, float* __restrict__ rank)
{
    // (two pieces of the list: [first, first + cnt1) and [first2, first2 + cnt2), together at most kScrRescueCap columns)
    __shared__ uint32_t sL[kScrRescueCap];
    cnt1 = cnt1 < kScrRescueCap ? cnt1 : kScrRescueCap;
    cnt2 = cnt1 + cnt2 <= kScrRescueCap ? cnt2 : kScrRescueCap - cnt1;
    const uint32_t cnt = cnt1 + cnt2;
    for (uint32_t e = threadIdx.x; e < cnt; e += 256u) sL[e] = e < cnt1 ? fl[first + e] : fl[first2 + (e - cnt1)];
    __syncthreads();
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n_pad; i += gridDim.x * 256u) {
        float v = i < n ? fabsf(c0h[i]) : 0.f;
        for (uint32_t e = 0; e < cnt; ++e) if (sL[e] == i) v = 3.0e38f;
        rank[i] = v;
    }
}



// ---- the exact re-check of the columns the half-precision certificate could not vouch for ---------------------------------------
// The certificate asks "is |c_i(k)| safely below the bound" with a margin (1/8 lambda_k) and an error term: a column it flags is
// usually NOT a column that changes the path — on noisy signals the columns of the noise floor come close to lambda at the late
// states.  Instead of handing the signal back, the few flagged columns (tens; the list holds 1024) are decided EXACTLY here, the way
// the subset form checks all columns on G (subbatch.hip: k_sub_verify): for column i the Gram values g_p = a_i . a_{col_p} with the
// path's positions and c0_i = a_i . y are formed from A in the solve's own precision, c_i(k) and q_i(k) of every logged state follow
// by the solve's own chain — c = fma(-x_p, g_p, c), q = fma(d_p, g_p, q) over the logged coefficients — and the reference's
// predicates decide (sub_check_v: |c| <= lambda, no candidate beats the logged step or ties it from the left; the state a path ends
// in: a larger |c| that leaves the tolerance test as it was is merged into the reported ||c||_inf).  Nothing approximate is left in
// the verdict of a re-checked column.  One workgroup per flagged column (a fixed grid walks the list); a wave forms the dot products
// of every fourth position.  fp32 (one signal of the screened form) and fp64 (the resident tier of the fp64 form).
//
// The LAST step of a path that ends by tolerance gets a treatment of its own.  On a noisy signal that step runs from the last planted
// column down to the noise floor, and the column that stops it — the first of the floor to reach lambda — has a small |c0|: it is not
// in the subset.  The subset's step is then too long, the coefficients overshoot, and the check rightly says so.  But such a column
// only SHORTENS the last step: the reference takes the smallest candidate m over all columns, x = x + m d, and stops (lambda - m <=
// tolerance); which column it was does not reach x (it enters with x = 0).  Every column whose candidate can be below the subset's
// step ends above the subset's final lambda and is therefore on this list.  So a column that beats the last step does not fail the
// signal: it POSTS its candidate (atomic min on the ordered bits, left-most on a tie) and k_scr_repair takes the step again with the
// smallest one.
template <typename T> struct ScrOrd;
template <> struct ScrOrd<float>  { static __device__ __forceinline__ unsigned long long pack(float m, uint32_t col) { return ((unsigned long long)__float_as_uint(m) << 32) | col; } };
// (the body of a workgroup, behind the launch's "is the signal still clean" test: k_scr_recheck, and k_scr_tail's first part.  fl and st
// are written by other workgroups of the same launch — no __restrict__ on them: nothing of theirs may travel the scalar path)
template <typename T>
__device__ __forceinline__
void scr_recheck_wg(const T* __restrict__ At, uint32_t ldm, uint32_t n, const T* __restrict__ y, const uint32_t* __restrict__ hdr, const T* __restrict__ LH,
                    const uint32_t* __restrict__ pcol, const T* __restrict__ LX, const T* __restrict__ LD, uint32_t* fl,
                    T tol, int tie_guard, DevState* st)
{
    constexpr uint32_t PCAP = ResCfg<T>::PCAP, LOGCAP = ResCfg<T>::LOGCAP;
    constexpr uint32_t VE = 16u / sizeof(T);                          // elements per 16-byte load
    typedef T vec_t __attribute__((ext_vector_type(16 / sizeof(T))));
    __shared__ uint32_t sH[LOGCAP * 8];
    __shared__ T sL[LOGCAP * 2];                                   // lambda, step of every state
    __shared__ T sG[PCAP + 1];                                     // g_p of the column in hand; [PCAP] = its c0
    const uint32_t nfl = fl[0];
    if (nfl == 0u) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (nfl > kScrFlCap) {
        if (blockIdx.x == 0u && tid == 0u) { __hip_atomic_store(&st->need_sweep, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); atomicOr(&st->sub_reason, kReasonColumn); }
        return;
    }
    if (blockIdx.x == 0u && tid == 0u) atomicOr(&st->sub_reason, kReasonRechecked);
    const uint32_t nlog = st->solo_nlog;
    if (nlog == 0u || nlog > LOGCAP) return;
    for (uint32_t e = tid; e < nlog * 8u; e += 256u) sH[e] = hdr[e];
    for (uint32_t e = tid; e < nlog; e += 256u) {
        if (LH != nullptr) { sL[2 * e] = LH[2 * e]; sL[2 * e + 1] = LH[2 * e + 1]; }
        else { sL[2 * e] = (T)__uint_as_float(hdr[e * 8u + 4u]); sL[2 * e + 1] = (T)__uint_as_float(hdr[e * 8u + 5u]); }
    }
    __syncthreads();
    const uint32_t Pfin = sH[(nlog - 1u) * 8u];
    const bool tol_stop = nlog >= 2u && !(sH[(nlog - 1u) * 8u + 1u] & 1u) && !(sL[2u * (nlog - 1u)] > tol);
    __shared__ uint32_t s_colfail;
    if (tid == 0u) s_colfail = 0u;
    bool fail_any = false, tie = false;
    for (uint32_t f = blockIdx.x; f < nfl; f += gridDim.x) {
        bool fail = false;                                            // (of THIS column)
        const uint32_t col = fl[1u + f];
        const T* ai = At + (size_t)(col < n ? col : 0u) * ldm;
        // wave w: the positions p = w, w + 4, ... (and c0 = a_i . y behind the last): a lane's 16-byte pieces of every 64, ascending, then the wave's sum
        for (uint32_t p = wave; p <= Pfin; p += 4u) {
            const bool isy = p == Pfin;
            const T* ap = isy ? y : At + (size_t)pcol[p] * ldm;
            T acc = T(0);
            for (uint32_t r = VE * lane; r < ldm; r += 64u * VE) {
                const vec_t a = *reinterpret_cast<const vec_t*>(ai + r), b = *reinterpret_cast<const vec_t*>(ap + r);
#pragma unroll
                for (uint32_t q = 0; q < VE; ++q) acc = sizeof(T) == 8 ? (T)__builtin_fma((double)a[q], (double)b[q], (double)acc) : (T)__builtin_fmaf((float)a[q], (float)b[q], (float)acc);
            }
            acc = wave_sum(acc);
            if (lane == 0u) sG[isy ? PCAP : p] = acc;
        }
        __syncthreads();
        if (tid < nlog && col < n) {
            auto chain = [&](uint32_t k, T& cv, T& qv) {
                const uint32_t Pk = sH[k * 8u];
                const T* xk = LX + (size_t)k * PCAP;
                const T* dk = LD + (size_t)k * PCAP;
                cv = sG[PCAP]; qv = T(0);
                for (uint32_t p = 0; p < Pk; ++p) {
                    const T g = sG[p];
                    if (sizeof(T) == 8) { cv = (T)__builtin_fma(-(double)xk[p], (double)g, (double)cv); qv = (T)__builtin_fma((double)dk[p], (double)g, (double)qv); }
                    else { cv = (T)__builtin_fmaf(-(float)xk[p], (float)g, (float)cv); qv = (T)__builtin_fmaf((float)dk[p], (float)g, (float)qv); }
                }
            };
            auto check = [&](uint32_t k, T cv, T qv) {
                const uint32_t* h = sH + k * 8u;
                const bool has_scan = (h[1] & 1u) != 0u;
                const T lam_end = k + 1u < nlog ? sL[2u * (k + 1u)] : T(0);
                const bool end_is_final = k + 1u < nlog && !(sH[(k + 1u) * 8u + 1u] & 1u);
                sub_check_v<T>(cv, qv, col, has_scan, sL[2u * k], sL[2u * k + 1u], h[2], h[7] != 0u, h[6], k + 2u == nlog, lam_end, end_is_final, tol,
                               tie_guard, st, fail, tie);
            };
            T cv, qv;
            chain(tid, cv, qv);
            const bool before = fail;
            if (tol_stop && tid + 2u == nlog) {
                const uint32_t* h = sH + tid * 8u;
                const T lam = sL[2u * tid], gam = sL[2u * tid + 1u];
                const uint32_t pick = h[2];
                const T ac = cv < T(0) ? -cv : cv;
                if (!(ac <= lam)) fail = true;
                const T dl = T(1) - qv, dr = T(1) + qv;
                T m = Lim<T>::max();
                if (dl != T(0)) { T t_ = (lam - cv) / dl; if (tie_guard && t_ == T(0) && dl > T(0)) t_ = Lim<T>::tiny(); if (t_ == T(0) && h[7] != 0u) tie = true; if (t_ > T(0) && t_ < m) m = t_; }
                if (dr != T(0)) { T t_ = (lam + cv) / dr; if (tie_guard && t_ == T(0) && dr > T(0)) t_ = Lim<T>::tiny(); if (t_ == T(0) && h[7] != 0u) tie = true; if (t_ > T(0) && t_ < m) m = t_; }
                if (better_min(m, col, gam, pick) && !(m >= gam * (sizeof(T) == 8 ? T(1) - T(1e-12) : T(0.99999)))) {
                    // (ahead of the subset's last step: a candidate for the repair — appended with its step; k_scr_repair takes the smallest)
                    if (lam - m <= tol) {
                        const uint32_t at = atomicAdd(&fl[kScrFlCap + 12u], 1u);
                        if (at < kScrRepCap) {
                            uint32_t* ent = fl + kScrFlCap + 16u + 4u * at;
                            ent[0] = col;
                            *reinterpret_cast<double*>(ent + 2) = (double)m;
                        } else fail = true;
                    } else fail = true;                                 // (the shorter step would not end the path: not this form's path)
                } else {
                    // (not ahead of the subset's step — or level with it within rounding, the tie of all columns at a least-squares jump:
                    // the usual predicates, and the state the path ends in)
                    check(tid, cv, qv);
                    T cf, qf;
                    chain(nlog - 1u, cf, qf);
                    check(nlog - 1u, cf, T(0));
                }
            } else if (!(tol_stop && tid + 1u == nlog)) {
                check(tid, cv, qv);
            }
            if (fail && !before && atomicCAS(&fl[kScrFlCap + 4u], 0u, 1u) == 0u) {        // (developer aid: the first failure)
                fl[kScrFlCap + 5u] = col; fl[kScrFlCap + 6u] = tid; fl[kScrFlCap + 7u] = __float_as_uint((float)cv); fl[kScrFlCap + 8u] = __float_as_uint((float)qv);
            }
            if (fail) { fail_any = true; s_colfail = 1u; }
        }
        __syncthreads();
        // (a column that beats a state of the path: listed for the rescue — the form once more with it in the subset, homotopy.hip)
        if (tid == 0u && s_colfail != 0u) {
            s_colfail = 0u;
            const uint32_t at = atomicAdd(&fl[kScrFlCap + 14u], 1u);
            if (at < kScrRescueCap) fl[kScrFlFail + at] = col;
        }
    }
    const bool fail = fail_any;
    if (fail) {
        __hip_atomic_store(&st->need_sweep, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (!(__hip_atomic_load(&st->sub_reason, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & kReasonColumn)) atomicOr(&st->sub_reason, kReasonColumn);
    }
    if (tie) __hip_atomic_store(&st->tie_stall, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <typename T>
__global__ __launch_bounds__(256)
void k_scr_recheck(const T* __restrict__ At, uint32_t ldm, uint32_t n, const T* __restrict__ y, const uint32_t* __restrict__ hdr, const T* __restrict__ LH,
                   const uint32_t* __restrict__ pcol, const T* __restrict__ LX, const T* __restrict__ LD, uint32_t* __restrict__ fl,
                   T tol, int tie_guard, DevState* __restrict__ st)
{
    if (st->status != 0u || st->need_sweep != 0u) return;
    scr_recheck_wg<T>(At, ldm, n, y, hdr, LH, pcol, LX, LD, fl, tol, tie_guard, st);
}

// ---- the last step again, with the smallest candidate the re-check found (see k_scr_recheck) -----------------------------------
// x = x_{K-1} + m d_{K-1} over the positions of the last scan state (homotopy-cpu.cpp:252), lambda = lambda_{K-1} - m, the column that
// stops the step in the lists and the trace instead of the subset's pick (either enters with x = 0: the coefficients do not see it).
// The winner's step is formed again here from its exact c and q (one workgroup: its Gram values with the positions, the chain).
// (scr_repair_wg: the workgroup's body behind the "still clean" test — k_scr_repair, and the last arriver of k_scr_tail, where the
// candidates were posted by other workgroups of the same launch: they are read with agent-scope atomic loads, never on the scalar path)
template <typename T>
__device__ __forceinline__
void scr_repair_wg(const T* __restrict__ At, uint32_t ldm, uint32_t n, const T* __restrict__ y, const uint32_t* __restrict__ hdr, const T* __restrict__ LH,
                   const uint32_t* __restrict__ pcol, const T* __restrict__ LX, const T* __restrict__ LD, const uint32_t* fl, T* x,
                   uint32_t* gam, uint32_t* tch, DevState* st, TraceEntry* trace, uint32_t trace_cap)
{
    constexpr uint32_t PCAP = ResCfg<T>::PCAP;
    constexpr uint32_t VE = 16u / sizeof(T);
    typedef T vec_t __attribute__((ext_vector_type(16 / sizeof(T))));
    __shared__ T sG[PCAP + 1];
    __shared__ T s_m;
    auto ld = [](const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    const uint32_t ncand = ld(&fl[kScrFlCap + 12u]);
    if (ncand == 0u) return;
    const uint32_t nlog = st->solo_nlog;
    if (nlog < 2u || ncand > kScrRepCap) return;                     // (an overflowing list failed the signal in k_scr_recheck)
    const uint32_t ks = nlog - 2u, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t col = 0xffffffffu;
    {
        double bm = 1.0e300;
        for (uint32_t i = 0; i < ncand; ++i) {                        // (uniform: every thread walks the short list)
            const uint32_t* ent = fl + kScrFlCap + 16u + 4u * i;
            const uint32_t ecol = ld(ent);
            const double mi = __longlong_as_double((long long)(((unsigned long long)ld(ent + 3) << 32) | ld(ent + 2)));
            if (mi < bm || (mi == bm && ecol < col)) { bm = mi; col = ecol; }
        }
    }
    const uint32_t Pk = hdr[ks * 8u], old_pick = hdr[ks * 8u + 2u];
    const T lam_k = LH != nullptr ? LH[2u * ks] : (T)__uint_as_float(hdr[ks * 8u + 4u]);
    // the winner's candidate in the solve's precision
    const T* ai = At + (size_t)(col < n ? col : 0u) * ldm;
    for (uint32_t p = wave; p <= Pk; p += 4u) {
        const bool isy = p == Pk;
        const T* ap = isy ? y : At + (size_t)pcol[p] * ldm;
        T acc = T(0);
        for (uint32_t r = VE * lane; r < ldm; r += 64u * VE) {
            const vec_t a = *reinterpret_cast<const vec_t*>(ai + r), b = *reinterpret_cast<const vec_t*>(ap + r);
#pragma unroll
            for (uint32_t q = 0; q < VE; ++q) acc = sizeof(T) == 8 ? (T)__builtin_fma((double)a[q], (double)b[q], (double)acc) : (T)__builtin_fmaf((float)a[q], (float)b[q], (float)acc);
        }
        acc = wave_sum(acc);
        if (lane == 0u) sG[isy ? PCAP : p] = acc;
    }
    __syncthreads();
    if (tid == 0u) {
        T cv = sG[PCAP], qv = T(0);
        for (uint32_t p = 0; p < Pk; ++p) {
            cv = cv - LX[(size_t)ks * PCAP + p] * sG[p];
            qv = qv + LD[(size_t)ks * PCAP + p] * sG[p];
        }
        const T dl = T(1) - qv, dr = T(1) + qv;
        T m = Lim<T>::max();
        if (dl != T(0)) { const T t_ = (lam_k - cv) / dl; if (t_ > T(0) && t_ < m) m = t_; }
        if (dr != T(0)) { const T t_ = (lam_k + cv) / dr; if (t_ > T(0) && t_ < m) m = t_; }
        s_m = m;
    }
    __syncthreads();
    const T m = s_m;
    if (tid < Pk) x[pcol[tid]] = LX[(size_t)ks * PCAP + tid] + m * LD[(size_t)ks * PCAP + tid];
    if (tid == 0u) {
        st->c_inf = (double)(lam_k - m);
        st->gamma = (double)m;
        st->idx = col;
        atomicOr(&st->sub_reason, kReasonRepaired);
        const uint32_t round = nlog - 1u;
        if (trace != nullptr && round < trace_cap) { trace[round].idx = col; trace[round].gamma = (double)m; }
        // the sorted lists: the subset's last pick out, the column that really stops the step in
        for (int which = 0; which < 2; ++which) {
            uint32_t* L = which == 0 ? gam : tch;
            const uint32_t cnt = which == 0 ? st->K : st->ntouched;
            uint32_t w = 0;
            for (uint32_t i = 0; i < cnt; ++i) if (L[i] != old_pick) L[w++] = L[i];
            uint32_t pos = w;
            while (pos > 0u && L[pos - 1u] > col) { L[pos] = L[pos - 1u]; --pos; }
            L[pos] = col;
        }
    }
}
template <typename T>
__global__ __launch_bounds__(256)
void k_scr_repair(const T* __restrict__ At, uint32_t ldm, uint32_t n, const T* __restrict__ y, const uint32_t* __restrict__ hdr, const T* __restrict__ LH,
                  const uint32_t* __restrict__ pcol, const T* __restrict__ LX, const T* __restrict__ LD, const uint32_t* __restrict__ fl, T* __restrict__ x,
                  uint32_t* __restrict__ gam, uint32_t* __restrict__ tch, DevState* __restrict__ st, TraceEntry* trace, uint32_t trace_cap)
{
    if (st->status != 0u || st->need_sweep != 0u) return;
    scr_repair_wg<T>(At, ldm, n, y, hdr, LH, pcol, LX, LD, fl, x, gam, tch, st, trace, trace_cap);
}

// ---- the tail of one screened fp32 solve in ONE launch: exact re-check, repair, verdict, state and x to the caller ------------------
// k_scr_recheck, k_scr_repair and k_epilogue (homotopy.hip) are three launches whose work is empty on a certified signal: two launch
// boundaries for nothing.  Here the kScrRecheckWgs workgroups take their share of the re-check (scr_recheck_wg: the same statements)
// and draw a ticket (arrive_last); the last arriver repairs (scr_repair_wg), applies the certificate's verdict and mirrors DevState to
// the mapped host block exactly as k_epilogue does.  The caller's device x receives the coefficients only of a certified path, as
// there: with nothing listed for the re-check (the common case) the verdict is final when the launch starts — every workgroup copies
// its share, workgroup 0 mirrors the state, and no ticket is drawn: the launch is k_epilogue's; with columns listed (noisy signals)
// the verdict is the last arriver's, and it alone copies (n words by one workgroup, on the rare path).
// st, fl and x change inside this launch: no __restrict__, and whatever another workgroup wrote is read with agent-scope atomic loads.
__global__ __launch_bounds__(256)
void k_scr_tail(const float* __restrict__ At, uint32_t ldm, uint32_t n, const float* __restrict__ y, const uint32_t* __restrict__ hdr,
                const uint32_t* __restrict__ pcol, const float* __restrict__ LX, const float* __restrict__ LD, uint32_t* fl, float tol, int tie_guard,
                DevState* st, float* x, uint32_t* gam, uint32_t* tch, TraceEntry* trace, uint32_t trace_cap,
                float* x_dst, long long incx, uint32_t* hs_mapped, uint32_t* ticket)
{
    __shared__ uint32_t s_go, s_nfl, s_last;
    const uint32_t tid = threadIdx.x;
    auto ld = [](const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    // DevState to the host, "a column was not certified" as the status (k_epilogue's statements)
    auto mirror = [&]() {
        constexpr uint32_t kWords = (uint32_t)(sizeof(DevState) / 4), kStatus = (uint32_t)(offsetof(DevState, status) / 4);
        const uint32_t* stw = reinterpret_cast<const uint32_t*>(st);
        const uint32_t flag = ld(&st->need_sweep);
        for (uint32_t i = tid; i < kWords; i += 256u) {
            uint32_t w = ld(stw + i);
            if (i == kStatus && w == 0u && flag != 0u) w = kStatusSubsetFail;
            __hip_atomic_store(&hs_mapped[i], w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    };
    // (one thread asks, the workgroup follows: a re-check elsewhere may raise need_sweep while this workgroup starts)
    if (tid == 0u) { s_go = (ld(&st->status) == 0u && ld(&st->need_sweep) == 0u) ? 1u : 0u; s_nfl = fl[0]; }
    __syncthreads();
    const bool go = s_go != 0u;
    if (s_nfl == 0u) {
        // nothing listed (the list's length does not change in this launch: every workgroup takes the same branch): nobody touches the
        // state here, the verdict stands — k_epilogue's work, no ticket
        if (go && x_dst != nullptr)
            for (uint32_t i = blockIdx.x * 256u + tid; i < n; i += gridDim.x * 256u) x_dst[(long long)i * incx] = x[i];
        if (blockIdx.x == 0u) mirror();
        return;
    }
    if (go) scr_recheck_wg<float>(At, ldm, n, y, hdr, nullptr, pcol, LX, LD, fl, tol, tie_guard, st);
    if (!arrive_last(ticket, gridDim.x, &s_last)) return;
    if (tid == 0u) s_go = (ld(&st->status) == 0u && ld(&st->need_sweep) == 0u) ? 1u : 0u;
    __syncthreads();
    if (s_go != 0u) {
        scr_repair_wg<float>(At, ldm, n, y, hdr, nullptr, pcol, LX, LD, fl, x, gam, tch, st, trace, trace_cap);
        // (the repair's plain stores to x and the state are read below by other waves, the state with loads that bypass L1: drained
        // before the barrier, as arrive_last does, so that the order holds by construction)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (x_dst != nullptr)
            for (uint32_t i = tid; i < n; i += 256u) x_dst[(long long)i * incx] = x[i];
    }
    mirror();
}

// ---- the screening pass of a batch chunk: FOUR slots per workgroup ----------------------------------------------------
// k_scr_gemm with a slot per workgroup re-stages every tile of A16 once per slot: 64 slots = 64 x 0.17 ms, whatever L2 holds
// — a workgroup's own pipeline (LDS staging, barriers) is what a launch takes.  Here a workgroup carries 128 columns x 4 slots
// x 64 states (8 MFMA tiles per wave: 128 accumulator registers; one workgroup per CU, one wave per SIMD): the A16 tile is
// staged once per stage for 256 right-hand sides, and the launch is MFMA-bound.  Slots whose path logged more than 64 states
// are left to k_scr_gemm<3> (launched beside this one; each kernel skips the other's slots).
constexpr uint32_t kScrSL = 4;                               // slots per workgroup
constexpr uint32_t kScrBS = 64;                              // states per slot here
__global__ __launch_bounds__(256, 1)
void k_scr_gemm_b(const __half* __restrict__ a16, uint32_t ldm, uint32_t n, const __half* __restrict__ r16_all,
                  const float* __restrict__ anorm, const float* __restrict__ rn2p_all, const float* __restrict__ tab_all,
                  const uint32_t* __restrict__ sub_all, const float* __restrict__ meta, DevState* __restrict__ st_all,
                  uint32_t* __restrict__ headroom, uint32_t nslots, uint32_t skew)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ uint32_t s_nst[kScrSL];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const uint32_t slot0 = blockIdx.x * kScrSL;
    if (tid < kScrSL) {
        uint32_t v = 0;
        const uint32_t sl = slot0 + tid;
        if (sl < nslots && st_all[sl].status == 0u) {
            const uint32_t nlog = st_all[sl].solo_nlog;
            if (nlog >= 2u && nlog - 1u <= kScrBS) v = nlog - 1u;
        }
        s_nst[tid] = v;
    }
    __syncthreads();
    uint32_t nst[kScrSL];
    bool any = false;
#pragma unroll
    for (uint32_t q = 0; q < kScrSL; ++q) { nst[q] = s_nst[q]; any = any || nst[q] != 0u; }
    if (!any) return;
    unsigned char* sA = smem;                                   // [128][272]
    unsigned char* sR = smem + (size_t)kScrCols * kScrPitchB;   // [4 x 64][272]
    const uint32_t col0 = blockIdx.y * kScrCols;
    const uint32_t lc = tid >> 4, piece = tid & 15u;
    const __half* ga = a16 + (size_t)(col0 + lc) * ldm + 8u * piece;
    // rows of the R tile: row = 64 q + state; thread (lc, piece) loads rows lc + 16 i, i < 16: slot q = i / 4
    const __half* gr[kScrSL];
#pragma unroll
    for (uint32_t q = 0; q < kScrSL; ++q) {
        const uint32_t sl = slot0 + q < nslots ? slot0 + q : slot0;
        gr[q] = r16_all + ((size_t)sl * kScrRhs + lc) * ldm + 8u * piece;
    }
    scr_u4 pa0[8], pr0[16], pa1[8], pr1[16];
#define SCB_LOAD(PA, PR, R0)                                                                                      \
    {                                                                                                             \
        _Pragma("unroll") for (int i = 0; i < 8; ++i)                                                             \
            PA[i] = __builtin_nontemporal_load(reinterpret_cast<const scr_u4*>(ga + (size_t)(16 * i) * ldm + (R0)));  \
        _Pragma("unroll") for (int i = 0; i < 16; ++i)                                                            \
            if (nst[i / 4] != 0u) PR[i] = *reinterpret_cast<const scr_u4*>(gr[i / 4] + (size_t)(16 * (i % 4)) * ldm + (R0)); \
    }
    scr_v16f acc[2 * kScrSL];
#pragma unroll
    for (int t = 0; t < (int)(2 * kScrSL); ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
    const uint32_t r = lane & 31u, h = lane >> 5;
    const unsigned char* rdA = sA + (size_t)(32u * w + r) * kScrPitchB + 16u * h;
    const unsigned char* rdR = sR + (size_t)r * kScrPitchB + 16u * h;
#define SCB_STAGE(PA, PR, MORE, RNEXT)                                                                            \
    {                                                                                                             \
        __syncthreads();                                                                                          \
        _Pragma("unroll") for (int i = 0; i < 8; ++i)                                                             \
            *reinterpret_cast<scr_u4*>(sA + (size_t)(lc + 16u * (uint32_t)i) * kScrPitchB + 16u * piece) = PA[i]; \
        _Pragma("unroll") for (int i = 0; i < 16; ++i)                                                            \
            if (nst[i / 4] != 0u)                                                                                 \
                *reinterpret_cast<scr_u4*>(sR + (size_t)(lc + 16u * (uint32_t)i) * kScrPitchB + 16u * piece) = PR[i]; \
        __syncthreads();                                                                                          \
        if (MORE) SCB_LOAD(PA, PR, (RNEXT))                                                                       \
        _Pragma("unroll") for (uint32_t ks = 0; ks < kScrKc / 16u; ++ks) {                                        \
            const scr_h8 bq = *reinterpret_cast<const scr_h8*>(rdA + 32u * ks);                                   \
            _Pragma("unroll") for (int t = 0; t < (int)(2 * kScrSL); ++t) {                                       \
                if (32u * (uint32_t)(t & 1) < nst[t / 2]) {                                                       \
                    const scr_h8 aq = *reinterpret_cast<const scr_h8*>(rdR + (size_t)(32 * t) * kScrPitchB + 32u * ks); \
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(aq, bq, acc[t], 0, 0, 0);                     \
                }                                                                                                 \
            }                                                                                                     \
        }                                                                                                         \
    }
    const uint32_t nstage = ldm / kScrKc;
    const uint32_t sbase = (blockIdx.y * skew) % nstage;
#define SCB_ROW(S) ((sbase + (S) >= nstage ? sbase + (S) - nstage : sbase + (S)) * kScrKc)
    SCB_LOAD(pa0, pr0, SCB_ROW(0u))
    SCB_LOAD(pa1, pr1, SCB_ROW(1u))
    for (uint32_t sidx = 0; sidx < nstage; sidx += 2u) {
        SCB_STAGE(pa0, pr0, sidx + 2u < nstage, SCB_ROW(sidx + 2u))
        SCB_STAGE(pa1, pr1, sidx + 3u < nstage, SCB_ROW(sidx + 3u))
    }
#undef SCB_ROW
#undef SCB_STAGE
#undef SCB_LOAD
    // ---- epilogue, slot by slot: its table, its subset, then this wave's (column, state) pairs ---------------------------
    float* sT = reinterpret_cast<float*>(smem);                 // [64][4]
    uint32_t* sSub = reinterpret_cast<uint32_t*>(smem) + kScrBS * 4u;          // [kSbS]
    float* sPart = reinterpret_cast<float*>(smem) + kScrBS * 4u + kSbS;        // [128][64]
    const float inv_sA = meta[1];
    const float sq_ldm = sqrtf((float)ldm);
    const uint32_t nblk = ldm / 64u;
    const uint32_t col = col0 + 32u * w + r;
    const float an = anorm[col < n ? col : 0u];
    float worst = 0.f;
#pragma unroll
    for (uint32_t q = 0; q < kScrSL; ++q) {
        const uint32_t ns = nst[q];
        if (ns == 0u) continue;                                   // (uniform)
        const uint32_t sl = slot0 + q;
        const float* rn2p = rn2p_all + (size_t)sl * nblk * kScrRhs;
        const float* tab = tab_all + (size_t)sl * kScrRhs * kScrTab;
        const uint32_t* sub = sub_all + (size_t)sl * kSbS;
        float s2 = 0.f;
        for (uint32_t b0 = 0; b0 < nblk; b0 += 128u) {
            const uint32_t nb = nblk - b0 < 128u ? nblk - b0 : 128u;
            __syncthreads();
            for (uint32_t e = tid; e < nb * kScrBS; e += 256u) { const uint32_t b = e / kScrBS, k = e - b * kScrBS; sPart[e] = rn2p[(size_t)(b0 + b) * kScrRhs + k]; }
            __syncthreads();
            if (tid < ns)
                for (uint32_t b = 0; b < nb; ++b) s2 += sPart[(size_t)b * kScrBS + tid];
        }
        __syncthreads();
        if (tid < kScrBS) {
            float f0 = 0.f, f1 = 0.f, f2 = 0.f, f3 = 0.f;
            if (tid < ns) {
                const float rn = sqrtf(s2) * 1.001f;
                const float inv_sk = tab[tid * kScrTab + 2];
                f0 = tab[tid * kScrTab + 0];
                f1 = tab[tid * kScrTab + 1];
                f2 = 0.0019726562f * rn + 6.103515625e-05f * sq_ldm * inv_sk;
                f3 = 6.103515625e-05f * sq_ldm * rn * inv_sA;
            }
            sT[tid * 4 + 0] = f0; sT[tid * 4 + 1] = f1; sT[tid * 4 + 2] = f2; sT[tid * 4 + 3] = f3;
        }
        for (uint32_t e = tid; e < kSbS; e += 256u) sSub[e] = sub[e];
        __syncthreads();
        uint32_t lo = 0, hi = kSbS;
        while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (sSub[mid] < col) lo = mid + 1u; else hi = mid; }
        const bool mine = col < n && !(lo < kSbS && sSub[lo] == col);
        bool flag = false;
        float wq = 0.f;
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const uint32_t kk = 32u * (uint32_t)tt + (uint32_t)(e & 3) + 8u * (uint32_t)(e >> 2) + 4u * h;
                if (kk < ns) {
                    const scr_v4f T4 = *reinterpret_cast<const scr_v4f*>(&sT[kk * 4u]);
                    const float v = fabsf(acc[2 * q + tt][e]) * T4[0] + (an * T4[2] + T4[3]);
                    if (!(v <= T4[1])) flag = true;
                    const float ratio = T4[1] > 0.f ? v / T4[1] : 3.0e38f;
                    wq = fmaxf(wq, ratio == ratio ? ratio : 3.0e38f);
                }
            }
        }
        if (mine && flag) {
            __hip_atomic_store(&st_all[sl].need_sweep, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (!(__hip_atomic_load(&st_all[sl].sub_reason, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & kReasonColumn)) atomicOr(&st_all[sl].sub_reason, kReasonColumn);
        }
        if (mine) worst = fmaxf(worst, wq);
    }
    worst = fmaxf(worst, __shfl_xor(worst, 1)); worst = fmaxf(worst, __shfl_xor(worst, 2)); worst = fmaxf(worst, __shfl_xor(worst, 4));
    worst = fmaxf(worst, __shfl_xor(worst, 8)); worst = fmaxf(worst, __shfl_xor(worst, 16)); worst = fmaxf(worst, __shfl_xor(worst, 32));
    if (lane == 0u && worst > 0.f) atomicMax(headroom, __float_as_uint(worst));
}

// ======== fp64: the same certificate around the launch-per-iteration engine ============================================
// No fp64 subset solve fits one workgroup's LDS (128 positions x 448 columns x 8 bytes).  The fp64 form therefore solves the
// path with the EXISTING fp64 engine on a sub-dictionary — the kS64Sub columns with the largest |c0|, gathered into a context
// of their own, where a pass over "A" is 268 MB instead of 16 GiB and an iteration touches 2048 columns instead of 131 072
// — and certifies every state of that path (k_la_iter logs them: DevState / ss_hip_ctx::slog) against all columns of the
// full dictionary with the same fp16 screening pass.  Reported values are the sub-context's fp64 arithmetic.

__global__ __launch_bounds__(256)
void k_s64_cabs(const double* __restrict__ c0, uint32_t n, uint32_t n_pad, float* __restrict__ cabs)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n_pad) cabs[i] = i < n ? (float)fabs(c0[i]) : 0.f;
}

// sub-dictionary: column j of dst = column sub[j] of src (16-byte copies; a missing entry leaves a zero column)
__global__ __launch_bounds__(256)
void k_s64_gather(const double* __restrict__ src, uint32_t ldm, uint32_t n, const uint32_t* __restrict__ sub, double* __restrict__ dst)
{
    const uint32_t j = blockIdx.x;
    const uint32_t col = sub[j];
    typedef double v2d __attribute__((ext_vector_type(2)));
    const v2d* s2 = reinterpret_cast<const v2d*>(src + (size_t)(col < n ? col : 0u) * ldm);
    v2d* d2 = reinterpret_cast<v2d*>(dst + (size_t)j * ldm);
    for (uint32_t r = threadIdx.x; r < ldm / 2u; r += 256u) d2[r] = col < n ? s2[r] : v2d{ 0.0, 0.0 };
}

// The states' coefficients over ONE list — the final list of touched columns (sub-indices, ascending: every earlier list is a
// subset of it) — transposed: xd[u][kk] = coefficient of list entry u in state kk + 1.  One workgroup per state.
__global__ __launch_bounds__(256)
void k_s64_dense(const unsigned char* __restrict__ slog, uint32_t T, double* __restrict__ xd, uint32_t* __restrict__ ctl, int omp)
{
    const uint32_t* l_cnt = reinterpret_cast<const uint32_t*>(slog);
    const double* l_lam = reinterpret_cast<const double*>(slog + (((size_t)kS64LogCap * 4 + 7) & ~(size_t)7));
    const uint32_t* l_cols = reinterpret_cast<const uint32_t*>(reinterpret_cast<const unsigned char*>(l_lam) + (size_t)2 * kS64LogCap * 8);
    const double* l_vals = reinterpret_cast<const double*>(reinterpret_cast<const unsigned char*>(l_cols) + ((((size_t)kS64LogCap * kS64LogK * 4) + 7) & ~(size_t)7));
    const uint32_t kk = blockIdx.x, t = kk + 1u;
    const uint32_t nfin = l_cnt[T], cnt = l_cnt[t];
    constexpr uint32_t pitch = kS64Rhs + 8u;
    if (nfin == 0xffffffffu || cnt == 0xffffffffu || cnt > nfin || nfin > kS64LogK) { if (threadIdx.x == 0) ctl[0] = 1u; return; }
    // Homotopy: only REGULAR paths are certified — every iteration inserts a column and lambda goes down.  On a path with removals or
    // one the first-step sign quirk has derailed, steps of rounding size (a support coefficient of 1e-16) decide what is toggled next,
    // and the sub-dictionary's Gram columns are the full engine's only to rounding (their rows are summed in chunks): such a signal goes
    // back to the engine whose roundings are the reference's to compare with (tools/dbg_screen224.py: iteration 47 of that path).
    if (!omp && (cnt != t + 1u || l_lam[t] > l_lam[t - 1u] * (1.0 + 1e-12))) { if (threadIdx.x == 0) ctl[0] = 1u; return; }
    const uint32_t* fin = l_cols + (size_t)T * kS64LogK;
    for (uint32_t u = threadIdx.x; u < kS64LogK; u += 256u) xd[(size_t)u * pitch + kk] = 0.0;
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < cnt; j += 256u) {
        const uint32_t col = l_cols[(size_t)t * kS64LogK + j];
        uint32_t lo = 0, hi = nfin;
        while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (fin[mid] < col) lo = mid + 1u; else hi = mid; }
        if (lo < nfin && fin[lo] == col) xd[(size_t)lo * pitch + kk] = l_vals[(size_t)t * kS64LogK + j];
        else ctl[0] = 1u;                                     // (a column that left the list: cannot happen, lists only grow)
    }
}

// r_k = y - A_sub[:, list] xd[:, k] in fp64, scaled and rounded to fp16; partial sums of ||r_k||^2; workgroup 0: the table.
// One workgroup per 64 rows, a thread owns 4 rows x 4 states x 3 rounds of 64 states; the list is walked 16 entries at a time.
__global__ __launch_bounds__(256)
void k_s64_residuals(const double* __restrict__ Asub, uint32_t ldm, const double* __restrict__ y, const unsigned char* __restrict__ slog,
                     uint32_t T, const double* __restrict__ xd, double tol, const float* __restrict__ meta,
                     __half* __restrict__ r16, float* __restrict__ rn2p, float* __restrict__ tab, uint32_t* __restrict__ ctl,
                     uint32_t* __restrict__ headroom, int first16)
{
    typedef double v2d __attribute__((ext_vector_type(2)));
    __shared__ __attribute__((aligned(16))) double sAc[16][64];
    __shared__ __attribute__((aligned(16))) double sXt[16][kS64Rhs + 8];
    __shared__ float sS[kS64Rhs];
    const uint32_t* l_cnt = reinterpret_cast<const uint32_t*>(slog);
    const double* l_lam = reinterpret_cast<const double*>(slog + (((size_t)kS64LogCap * 4 + 7) & ~(size_t)7));
    const double* l_exp = l_lam + kS64LogCap;
    const uint32_t* l_cols = reinterpret_cast<const uint32_t*>(reinterpret_cast<const unsigned char*>(l_exp) + (size_t)kS64LogCap * 8);
    if (ctl[0] != 0u) return;
    const uint32_t nst = T;                                      // states 1 .. T
    const uint32_t nfin = l_cnt[T];
    if (nfin == 0xffffffffu || nfin > kS64LogK) return;           // (k_s64_dense raised the flag)
    const uint32_t* fin = l_cols + (size_t)T * kS64LogK;
    constexpr uint32_t pitch = kS64Rhs + 8u;
    const uint32_t tid = threadIdx.x, r0 = blockIdx.x * 64u;
    if (tid < kS64Rhs) {
        float sc = 1.f;
        if (tid < nst) {
            const double lam = l_lam[tid + 1u];
            const bool final_state = tid + 1u == T;
            sc = scr_state_scale((float)(final_state ? fmax(lam, tol) : lam));
        }
        sS[tid] = sc;
    }
    const uint32_t rg = tid & 15u, sgp = tid >> 4;
    double acc[3][4][4];
    {
        const v2d y0 = *reinterpret_cast<const v2d*>(y + r0 + 4u * rg), y1 = *reinterpret_cast<const v2d*>(y + r0 + 4u * rg + 2u);
#pragma unroll
        for (int rd = 0; rd < 3; ++rd)
#pragma unroll
            for (int si = 0; si < 4; ++si) { acc[rd][si][0] = y0[0]; acc[rd][si][1] = y0[1]; acc[rd][si][2] = y1[0]; acc[rd][si][3] = y1[1]; }
    }
    for (uint32_t u0 = 0; u0 < nfin; u0 += 16u) {
        __syncthreads();
        {   // 16 list entries x 64 rows of the sub-dictionary, 16 x 192 coefficients
            const uint32_t p = tid >> 4, q4 = tid & 15u;
            const uint32_t u = u0 + p;
            const uint32_t col = u < nfin ? fin[u] : 0xffffffffu;
            v2d a0 = { 0.0, 0.0 }, a1 = { 0.0, 0.0 };
            if (col < kS64Sub) {
                a0 = *reinterpret_cast<const v2d*>(Asub + (size_t)col * ldm + r0 + 4u * q4);
                a1 = *reinterpret_cast<const v2d*>(Asub + (size_t)col * ldm + r0 + 4u * q4 + 2u);
            }
            *reinterpret_cast<v2d*>(&sAc[p][4u * q4]) = a0;
            *reinterpret_cast<v2d*>(&sAc[p][4u * q4 + 2u]) = a1;
            for (uint32_t e = tid; e < 16u * pitch; e += 256u) {
                const uint32_t pp = e / pitch, k = e - pp * pitch;
                sXt[pp][k] = (u0 + pp < nfin && k < nst) ? xd[(size_t)(u0 + pp) * pitch + k] : 0.0;
            }
        }
        __syncthreads();
#pragma unroll
        for (int rd = 0; rd < 3; ++rd) {
            const uint32_t s0 = 64u * (uint32_t)rd + 4u * sgp;
            if (s0 < nst) {                                           // (uniform over the 16 lanes of a state group)
#pragma unroll 4
                for (uint32_t p = 0; p < 16u; ++p) {
                    const v2d a0 = *reinterpret_cast<const v2d*>(&sAc[p][4u * rg]), a1 = *reinterpret_cast<const v2d*>(&sAc[p][4u * rg + 2u]);
                    const v2d x0 = *reinterpret_cast<const v2d*>(&sXt[p][s0]), x1 = *reinterpret_cast<const v2d*>(&sXt[p][s0 + 2u]);
                    const double av[4] = { a0[0], a0[1], a1[0], a1[1] }, xv[4] = { x0[0], x0[1], x1[0], x1[1] };
#pragma unroll
                    for (int si = 0; si < 4; ++si)
#pragma unroll
                        for (int ri = 0; ri < 4; ++ri) acc[rd][si][ri] = __builtin_fma(-xv[si], av[ri], acc[rd][si][ri]);
                }
            }
        }
    }
    // the residuals in the units of the dictionary's columns (meta[13] = 2^u: r_k of the dictionary 2^-u A, whose columns are of
    // ordinary size, is 2^u r_k): s_k is chosen from lambda_k for such columns, and ||r_k||^2 stays inside float
    const double units = (double)meta[13];
    bool ovf = false;
#pragma unroll
    for (int rd = 0; rd < 3; ++rd) {
#pragma unroll
        for (int si = 0; si < 4; ++si) {
            const uint32_t kk = 64u * (uint32_t)rd + 4u * sgp + (uint32_t)si;
            const float sc = sS[kk < kS64Rhs ? kk : 0u];
            float ss = 0.f;
            __half hv[4];
#pragma unroll
            for (int ri = 0; ri < 4; ++ri) {
                const float r = (float)(acc[rd][si][ri] * units);          // (2^u r: exact)
                ss = __builtin_fmaf(r, r, ss);
                const float v = r * sc;
                if (kk < nst && !(fabsf(v) < 60000.f)) ovf = true;
                hv[ri] = __float2half_rn(v);
            }
            ss += __shfl_xor(ss, 1); ss += __shfl_xor(ss, 2); ss += __shfl_xor(ss, 4); ss += __shfl_xor(ss, 8);
            if (kk < nst) {
                *reinterpret_cast<uint2*>(r16 + (size_t)kk * ldm + r0 + 4u * rg) = *reinterpret_cast<const uint2*>(hv);
                if (rg == 0u) rn2p[(size_t)blockIdx.x * kS64Rhs + kk] = ss * 1.0001f;     // (the cast of r to float: inside)
            }
        }
    }
    if (ovf) ctl[0] = 1u;
    if (blockIdx.x == 0u) {
        if (tid == 0u) {
            float ratio0 = 0.f;
            if (first16) {
                // state 0 after a first pass in half precision (k_scr_first; see k_scr_residuals): every column left out of the
                // sub-dictionary has |c~0| < T — certified against the sub-context's exact lambda_0
                const float lam0 = (float)l_lam[0] * 0.9999999f;
                const float yn = sqrtf(meta[5]) * 1.001f;
                const float eps0 = meta[8] * yn * meta[4] + meta[9] * sqrtf((float)ldm) * yn;
                const float bound0 = lam0 * 0.875f - 1e-12f * lam0;
                const float v0 = meta[6] + eps0;
                if (!(v0 <= bound0)) ctl[0] = 1u;
                ratio0 = bound0 > 0.f && v0 == v0 ? v0 / bound0 : 3.0e38f;
            }
            *headroom = __float_as_uint(ratio0);
        }
        if (tid < nst) {
            const float lam = (float)l_lam[tid + 1u];
            const bool final_state = tid + 1u == T;
            const float slack = 1e-12f * (float)l_lam[0];           // (state 0: x = 0, lambda_0 = ||A^T y||_inf; fp64: the reference's own rounding is 1e-16)
            float bound;
            // (the smaller of max |c| and lambda_prev - gamma_prev: see k_scr_residuals)
            const bool ls_jump = final_state && !((double)lam > tol) && !(l_exp[tid + 1u] > 1e-13 * l_lam[0]);
            if (ls_jump) bound = (float)tol * 0.9375f - slack;
            else bound = fminf(lam, (float)l_exp[tid + 1u]) * 0.875f - slack;
            const float inv_sk = 1.f / sS[tid];
            tab[tid * kScrTab + 0] = (meta[1] * meta[12]) * inv_sk;     // (r16 = fl16(s_k 2^u r_k))
            tab[tid * kScrTab + 1] = bound;
            tab[tid * kScrTab + 2] = inv_sk;
            tab[tid * kScrTab + 3] = lam;
        }
    }
}

// the sub-context's solution back onto the dictionary's columns, and the verdict into the slot's state
__global__ __launch_bounds__(256)
void k_s64_finish(const uint32_t* __restrict__ sub, const double* __restrict__ xsub, uint32_t n, double* __restrict__ x,
                  DevState* __restrict__ st, const uint32_t* __restrict__ ctl, uint32_t iter, double c_inf, uint32_t K)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j < kS64Sub) { const uint32_t col = sub[j]; if (col < n) x[col] = xsub[j]; }
    if (j == 0u) {
        const bool fail = ctl[0] != 0u || st->need_sweep != 0u;
        st->status = fail ? kStatusSubsetFail : 0u;
        st->need_sweep = 0u;
        st->iter = iter;
        st->K = K;
        st->c_inf = c_inf;
        st->done_round = iter + 1u;
        st->done = 1u;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------
// Every stage of the screened solve is launched from ONE function below (launch_* / scr_pass); the drivers behind them — the fp32 form,
// its rescue scan, the fp32 batch chunk, the fp64 sub-dictionary tier, the fp64 resident tier, its rescue scan, the fp64 batch chunk —
// say what they vary.  Launch results are dropped; each driver reads hipGetLastError() once at its end.
static ScreenState* scr_of(ss_hip_ctx* ctx) { return ctx->screen.as<ScreenState>(); }

// the headroom of the last solve (meta[3], a float's bits): the residual kernels reset it, the screening passes raise it
static uint32_t* scr_headroom(const ScreenState& S) { return reinterpret_cast<uint32_t*>(S.meta) + 3; }

// a preparation that did not fit: what it had obtained is given back, the form is not tried again on this context (-> false)
static bool screen_off(ss_hip_ctx* ctx)
{
    ctx->screen.reset();
    ctx->handoff = nullptr;
    ctx->screen_failed_alloc = 1;
    return false;
}

// ---- what a column replacement keeps current (dictupdate.hip) -------------------------------------------------------------------
ScreenCopies screen_copies(ss_hip_ctx* ctx)
{
    ScreenCopies c;
    if (ScreenState* S = scr_of(ctx)) { c.a16 = S->a16; c.a8 = S->a8; c.anorm = S->anorm; c.amaxc = S->amaxc; c.meta = S->meta; c.sub = S->sub; }
    return c;
}

// the fp16 / fp8 copy of the whole dictionary under the scales meta[0] / meta[10] hold now
static dim3 scr_convert_grid(size_t items) { return dim3((unsigned)std::min<size_t>((items + 255) / 256, 65536)); }
template <typename TA>
static void launch_a16_convert(ss_hip_ctx* ctx, const ScreenState& S)
{
    const size_t total8 = (size_t)ctx->n_pad * ctx->ldm / 8;
    hipLaunchKernelGGL((k_a16_convert<TA>), scr_convert_grid(total8), dim3(256), 0, ctx->stream, static_cast<const TA*>(ctx->At), total8, (const float*)S.meta, S.a16);
}
template <typename TA>
static void launch_a8_convert(ss_hip_ctx* ctx, const ScreenState& S)
{
    const size_t total16 = (size_t)ctx->n_pad * ctx->ldm / 16;
    hipLaunchKernelGGL((k_a8_convert<TA>), scr_convert_grid(total16), dim3(256), 0, ctx->stream, static_cast<const TA*>(ctx->At), total16, (const float*)S.meta, S.a8);
}

// ... again, after columns were replaced: the preparation's own conversion passes
hipError_t screen_reconvert(ss_hip_ctx* ctx, bool a16, bool a8)
{
    ScreenState* S = scr_of(ctx);
    if (S == nullptr) return hipErrorInvalidConfiguration;
    if (a16 && S->a16 != nullptr) { if (ctx->is_f64) launch_a16_convert<double>(ctx, *S); else launch_a16_convert<float>(ctx, *S); }
    if (a8 && S->a8 != nullptr) { if (ctx->is_f64) launch_a8_convert<double>(ctx, *S); else launch_a8_convert<float>(ctx, *S); }
    return hipGetLastError();
}

// (the main loop's two tiles; the epilogue's tables — 96 x 4 + 448 + 128 x 96 floats — fit inside)
// row offset of workgroup b = (b * skew) mod stages (29: any odd multiplier not near a divisor of the stage count does; 0 = no offsets was 0.61 of the HBM peak)
static uint32_t scr_skew()
{
    return 29u;
}

static size_t scr_gemm_lds(uint32_t nsub, uint32_t nt = 3)
{
    const size_t rh = 32 * (size_t)nt, pb = nt <= 3 ? 128 : 64;
    return std::max<size_t>((size_t)(kScrCols + rh) * kScrPitchB, (rh * 4 + nsub + pb * rh) * 4);
}

// ---- the screening pass ------------------------------------------------------------------------------------------------------------
// What one launch of k_scr_gemm varies.  The launcher supplies the rest: the fp16 copy, the norms, meta, the headroom word, the skew, one
// workgroup per 128 columns (and slot), the LDS size of (nsub, NT).
struct ScrPass {
    ResBlock res;                     // the states' residuals, norms and table (slot 0's: the kernel adds the slot offsets)
    const uint32_t* sub = nullptr;    // the subset whose columns the certificate leaves out, ...
    uint32_t nsub = 0;                // ... its size (0 in the writing mode: up to 2048 columns the LDS size is the main loop's tiles either way)
    DevState* st = nullptr;
    uint32_t slots = 1;
    uint32_t nst_fixed = 0;           // 0: as many states as the slot's log holds; a count; 0xffffffff: only the slots whose log passed 64 states
    uint32_t gate = 0;                // 0: always; 1 / 2: the log holds up to / more than 128 states; 3: the rescue's scan
    uint32_t* fl = nullptr;           // the list for the exact re-check (or the scan's lists)
    const float* c0h = nullptr;       // the first pass's c~0: state 0 is certified too
    float* out_abs = nullptr;         // writing mode (the ranking of an fp64 batch): |c~| of every (right-hand side, column), ...
    uint32_t out_pitch = 0;           // ... its pitch
};

// NT tiles of 32 states per workgroup
template <int NT>
static void scr_pass(const ss_hip_ctx* ctx, const ScreenState& S, const ScrPass& p)
{
    hipLaunchKernelGGL(k_scr_gemm<NT>, dim3(p.slots, ctx->n_pad / kScrCols), dim3(256), scr_gemm_lds(p.nsub, NT), ctx->stream, (const __half*)S.a16, ctx->ldm,
                       (uint32_t)ctx->n, (const __half*)p.res.r16, (const float*)S.anorm, (const float*)p.res.rn2p, p.res.rhs, (const float*)p.res.tab, p.sub, p.nsub,
                       (const float*)S.meta, p.st, scr_headroom(S), p.nst_fixed, scr_skew(), p.gate, p.fl, p.c0h, p.out_abs, p.out_pitch);
}
// (its dynamic LDS beyond 64 KiB: the ceiling of the largest subset any form passes)
template <int NT>
static hipError_t scr_pass_attr()
{
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&k_scr_gemm<NT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)scr_gemm_lds(kS64Sub, NT));
}

// ---- the other stages ----------------------------------------------------------------------------------------------------------------
// Gs = A_S^T A_S of every slot's subset from the fp32 dictionary: partials per row chunk, summed in a fixed order (the mirror of
// launch_sgram64).  One signal (y given): the sum's launch is handed the dictionary too, and with exact_c0 — its first pass ran in reduced
// precision — workgroups beyond the sum write the exact c0 = a_j . y of the subset's columns into c0.
static void launch_sgram32(const ss_hip_ctx* ctx, const uint32_t* sub, float* part, float* gs, uint32_t nslots = 1, const float* y = nullptr, float* c0 = nullptr,
                           bool exact_c0 = false)
{
    const float* At = static_cast<const float*>(ctx->At);
    const uint32_t ldm = ctx->ldm, n = (uint32_t)ctx->n;
    const uint32_t nsplit = (ldm % (kSgSplit * kSgStep) == 0) ? kSgSplit : 4u;        // (ldm is a multiple of 256)
    constexpr uint32_t NT = kSbS / kSgT;
    const bool one = y != nullptr;
    hipLaunchKernelGGL(k_sgram_part, dim3(NT * (NT + 1) / 2, nsplit, nslots), dim3(256), 0, ctx->stream, At, ldm, n, sub, ldm / nsplit, part);
    hipLaunchKernelGGL(k_sgram_sum, dim3((kSbS * kSbS + 255) / 256 + (exact_c0 ? kSbS : 0u), nslots), dim3(256), 0, ctx->stream, (const float*)part, nsplit, gs,
                       one ? At : (const float*)nullptr, one ? ldm : 0u, y, one ? sub : (const uint32_t*)nullptr, one ? n : 0u, c0);
}

// r_k = y - A_S x_S(k) of every logged state into the block, the states' table, the headroom word reset (scan: the rescue's look at a
// declined solve's log)
static void launch_scr_residuals(const ss_hip_ctx* ctx, const ScreenState& S, const float* y, const SubBufs& B, float tol, const ResBlock& res, DevState* st,
                                 uint32_t nslots, bool first16, uint32_t* fl, bool omp, bool scan = false)
{
    hipLaunchKernelGGL(k_scr_residuals, dim3(ctx->ldm / 64u, nslots), dim3(256), 0, ctx->stream, static_cast<const float*>(ctx->At), ctx->ldm, (uint32_t)ctx->n, y,
                       (const uint32_t*)B.hdr, (const uint32_t*)B.pcol, (const float*)B.LX, tol, (const float*)S.meta, res.r16, res.rn2p, res.tab, scr_headroom(S), st,
                       first16 ? 1 : 0, fl, omp ? 1 : 0, scan ? 1 : 0);
}

// the exact tail: the columns the pass left undecided re-checked with the reference's predicates, the last step repaired (an empty list:
// the launches return at once)
template <typename T>
static void launch_scr_exact_tail(const ss_hip_ctx* ctx, Workspace<T>& ws, const T* y, const ResLog<T>& log, uint32_t* fl, T tol)
{
    const T* At = static_cast<const T*>(ctx->At);
    const uint32_t ldm = ctx->ldm, n = (uint32_t)ctx->n;
    hipLaunchKernelGGL((k_scr_recheck<T>), dim3(kScrRecheckWgs), dim3(256), 0, ctx->stream, At, ldm, n, y, (const uint32_t*)log.hdr, (const T*)log.H,
                       (const uint32_t*)log.pcol, (const T*)log.X, (const T*)log.D, fl, tol, ctx->tie_guard, ws.st);
    hipLaunchKernelGGL((k_scr_repair<T>), dim3(1), dim3(256), 0, ctx->stream, At, ldm, n, y, (const uint32_t*)log.hdr, (const T*)log.H, (const uint32_t*)log.pcol,
                       (const T*)log.X, (const T*)log.D, (const uint32_t*)fl, ws.x, ws.gam, ws.touched, ws.st, ws.trace, ws.trace_cap);
}

// the rescue's ranking: c~0 with the columns the scan chose on top, into S.rank
static void launch_scr_rescue_rank(const ss_hip_ctx* ctx, const ScreenState& S, const float* c0h)
{
    const uint32_t np = ctx->n_pad;
    hipLaunchKernelGGL(k_scr_rescue_rank, dim3(std::min<uint32_t>((np + 255u) / 256u, 1024u)), dim3(256), 0, ctx->stream, c0h, (const uint32_t*)S.fl, S.rescue_first,
                       S.rescue_count, S.rescue_first2, S.rescue_count2, (uint32_t)ctx->n, np, S.rank);
}

// What a rescue scan listed, read back (one synchronisation, on the rare path), and which of the three lists the rescue takes
// -> *count_out columns.  In this order: the columns that stand above everything ranked out at state 0 (planted columns the ranking
// missed); if there is none, the columns the declined attempt's exact re-check found beating a state (from_recheck); if there is
// neither, whatever else beats a state, where that is a handful.  (On a path that went astray early the re-check's failures and the
// other violators are mostly the noise columns of its late states — hundreds; the first kind names what went wrong.)
static hipError_t scr_rescue_readback(ScreenState& S, hipStream_t s, bool from_recheck, uint32_t* count_out)
{
    uint32_t cnt = 0, tail[3] = { 0u, 0u, 0u };                  // [cap + 12 .. + 14]: repair's count, the scan's second list, the re-check's failures
    hipError_t e = hipMemcpyAsync(&cnt, S.fl, sizeof(cnt), hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) return e;
    e = hipMemcpyAsync(tail, S.fl + kScrFlCap + 12u, sizeof(tail), hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) return e;
    e = hipStreamSynchronize(s);
    if (e != hipSuccess) return e;
    const uint32_t cnt2 = tail[1], cntf = from_recheck ? tail[2] : 0u;
    S.rescue_first2 = 1u; S.rescue_count2 = 0u;
    if (cnt != 0u) { S.rescue_first = 1u; S.rescue_count = cnt; }
    else if (cntf != 0u) { S.rescue_first = kScrFlFail; S.rescue_count = cntf; }
    else { S.rescue_first = 1u + kScrFlCap / 2u; S.rescue_count = cnt2; }
    *count_out = S.rescue_count + S.rescue_count2;
    return hipSuccess;
}

// ---- the preparations ----------------------------------------------------------------------------------------------------------------
// What the fp32 and the fp64 form share: the fp16 copy of A (half of A's bytes again), the column norms and maxima, meta, the residual
// block of one signal ...
static void scr_take_front(Takes& t, ScreenState& S, uint32_t np, uint32_t ldm, uint32_t rhs)
{
    t(&S.a16, (size_t)np * ldm * sizeof(__half))(&S.anorm, (size_t)np * sizeof(float))(&S.amaxc, (size_t)np * sizeof(float))(&S.meta, kScrMeta * sizeof(float));
    S.res.take(t, rhs, ldm);
}
// ... and, behind the form's own memsets, the block cleared, the statistics, the scale (units: fp64 — the columns' unit exponent), the copy
template <typename TA>
static bool scr_fill_front(ss_hip_ctx* ctx, ScreenState& S, int units)
{
    hipStream_t s = ctx->stream;
    (void)S.res.clear(ctx->ldm, 1, s);
    hipLaunchKernelGGL((k_a16_stats<TA>), dim3(ctx->n_pad), dim3(256), 0, s, static_cast<const TA*>(ctx->At), ctx->ldm, S.anorm, S.amaxc, S.meta);
    hipLaunchKernelGGL(k_a16_scale, dim3(1), dim3(1), 0, s, S.meta, units);
    launch_a16_convert<TA>(ctx, S);
    return hipGetLastError() == hipSuccess;
}

// Shape / option test, and — the first time it says yes — the preparation.  A failed allocation switches the form off for this context
// (the default engine goes on as before).
bool screen_form_usable(ss_hip_ctx* ctx)
{
    if (ctx->screen_single == 0 || ctx->is_f64 || ctx->kind != 0 || ctx->screen_failed_alloc) return false;
    if (ctx->colshard != nullptr) return false;
    const uint32_t ldm = ctx->ldm, np = ctx->n_pad;
    // the bound's accumulation term assumes ldm <= 16384; tiles: 128 columns, 128 rows; subset Gram: 4 or 8 chunks of 64-row steps
    if (ldm % kScrKc != 0 || np % kScrCols != 0 || ldm > 16384u || ctx->n < kSbS) return false;
    // where it pays: the pass over the fp16 copy replaces two fp32 passes — dictionaries of at least 16 Mi entries (option 2: any shape)
    if (ctx->screen_single < 2 && ((size_t)ctx->m * ctx->n < ((size_t)16 << 20) || ctx->n < 8192u)) return false;
    if (!sub_form_usable(ctx)) return false;
    if (ctx->screen != nullptr) return true;
    ScreenState* S = &part<ScreenState>(ctx->screen);
    // (the hand-off block: tickets and the selection's shared histogram in front — k_la_reset clears those at the start of every attempt —,
    // then the selection workgroups' counts and entries)
    const size_t ho_words = (size_t)kHoEnt + (np <= kHoSelCols ? (size_t)np + 4u * kHoSelWgs : 0u);
    Takes t{ S->own };
    scr_take_front(t, *S, np, ldm, kScrRhs);
    t(&S->gs_part, (size_t)kSgSplit * kSbS * kSbS * sizeof(float))(&S->gs, (size_t)kSbS * kSbS * sizeof(float))(&S->wmax, (size_t)kScrWmax * sizeof(float))
     (&S->fl, (size_t)kScrFlWords * sizeof(uint32_t))(&ctx->handoff, ho_words * sizeof(uint32_t));
    if (t.ok && scr_pass_attr<3>() != hipSuccess) { (void)hipGetLastError(); t.ok = false; }
    if (!t.ok) return screen_off(ctx);
    hipStream_t s = ctx->stream;
    (void)hipMemsetAsync(S->meta, 0, kScrMeta * sizeof(float), s);
    (void)hipMemsetAsync(S->fl, 0, (size_t)kScrFlWords * sizeof(uint32_t), s);
    (void)hipMemsetAsync(ctx->handoff, 0, ho_words * sizeof(uint32_t), s);
    return scr_fill_front<float>(ctx, *S, 0) || screen_off(ctx);
}

// r = y in ws.rhs (block 0); c0 = A^T y in ws.c0 — or, first16, nothing yet: the first pass runs here, over the fp16 copy
// (k_scr_first; ws.c0 then holds c~0 with the subset's entries exact).  Everything on the context's stream.  Profiling events:
// `first` around the half-precision first pass, `screen` around the screening pass, `path` around the path kernel.
// (y in LDS: 4 ldm bytes + the reduction scratch — beyond 64 KiB the kernel's dynamic-LDS ceiling is raised first)
template <typename TY>
static bool scr_first_attr()
{
    static const bool ok = [] {
        const bool r = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_scr_first<TY, 4, 3>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           16384 * (int)sizeof(float) + 64) == hipSuccess;
        if (!r) (void)hipGetLastError();
        return r;
    }();
    return ok;
}

bool screen_first16_usable(const ss_hip_ctx* ctx)
{
    if (ctx->screen_first16 == 0 || ctx->ldm % 512u != 0u || ctx->ldm > 16384u) return false;
    if ((size_t)ctx->ldm * sizeof(float) + 64 <= 65536) return true;
    return ctx->is_f64 ? scr_first_attr<double>() : scr_first_attr<float>();
}

// The fp8 copy for the ranking pass (option screen_first8, default 1): made the first time a first pass is launched on a context whose
// rows allow it (ldm a multiple of 1024); a failed allocation leaves the half-precision pass in place.
template <typename TA>
static bool screen_first8_ready(ss_hip_ctx* ctx, ScreenState* S)
{
    if (ctx->screen_first8 == 0 || ctx->ldm % 1024u != 0u || S->a8_failed) return false;
    if (S->a8 != nullptr) return true;
    size_t free_b = 0, total_b = 0;
    const size_t bytes = (size_t)ctx->n_pad * ctx->ldm;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || bytes + ((size_t)2 << 30) > free_b || S->own.device(&S->a8, bytes) != hipSuccess) {
        (void)hipGetLastError();
        S->a8_failed = true;
        return false;
    }
    hipLaunchKernelGGL(k_a8_scale, dim3(1), dim3(1), 0, ctx->stream, S->meta);
    launch_a8_convert<TA>(ctx, *S);
    if (hipGetLastError() != hipSuccess) { (void)S->own.drop(S->a8); S->a8_failed = true; return false; }
    return true;
}
template <typename TY> static bool scr_first8_attr()
{
    static const bool ok = [] {
        const bool a = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_scr_first8<TY, 4, 3>), hipFuncAttributeMaxDynamicSharedMemorySize, 65536 + 64) == hipSuccess;
        if (!a) (void)hipGetLastError();
        return a;
    }();
    return ok;
}

// c~0 = A16^T y / sA (or A8^T y / sA8) into c0h ([n_pad] floats), ||y||^2 into meta[5], the pass's error model into meta[8], meta[9]
// the ranking pass over the fp8 copy can be launched: the copy is there (made now, if this is the first time) and y fits the kernel's LDS
template <typename TY>
static bool scr_first8_launchable(ss_hip_ctx* ctx, ScreenState* S)
{
    return screen_first8_ready<TY>(ctx, S) && ((size_t)ctx->ldm * sizeof(float) + 64 <= 65536u || scr_first8_attr<TY>());
}

// (reset: the clears of k_la_reset ride in the fp8 pass's prologue, which then reads the caller's y — or the staged copy — itself; the
// caller has asked screen_first8_folds.  Should the fp8 pass not be launchable after all, k_la_reset is launched here, in front of the
// pass that does run: no attempt goes without one of the two.)
template <typename TY>
static hipError_t launch_scr_first(ss_hip_ctx* ctx, ScreenState* S, const TY* y, float* c0h, float* wmax = nullptr, uint32_t* nwmax = nullptr,
                                   const LaResetArgs<float>* reset = nullptr)
{
    const uint32_t ldm = ctx->ldm, np = ctx->n_pad;
    const size_t lds = (size_t)ldm * sizeof(float) + 64;
    const bool fold = reset != nullptr && reset->x != nullptr;
    const bool first8 = (lds <= 65536u || scr_first_attr<TY>()) && scr_first8_launchable<TY>(ctx, S);
    if (fold && !first8) {
        const hipError_t er = launch_la_reset_args<float>(ctx, *reset);
        if (er != hipSuccess) return er;
    }
    if (lds > 65536u && !scr_first_attr<TY>()) return hipErrorInvalidConfiguration;
    const uint32_t grid = std::min<uint32_t>(np / 32u, (uint32_t)ctx->num_cus * 2u);
    if (grid * 8u > kScrWmax) wmax = nullptr;
    if (first8) {
        const TY* ysrc = y;
        long long incy = 1;
        uint32_t ylen = ldm;
        if constexpr (std::is_same<TY, float>::value) {
            if (fold && reset->y_user != nullptr) { ysrc = reset->y_user; incy = reset->incy; ylen = reset->m; }
            else if (fold) ysrc = reset->y;
        }
        hipLaunchKernelGGL((k_scr_first8<TY, 4, 3>), dim3(grid), dim3(512), lds, ctx->stream, (const uint8_t*)S->a8, ldm, (uint32_t)ctx->n, np / 32u, ysrc,
                           S->meta, c0h, scr_skew() == 0u ? 0u : 5u, wmax, incy, ylen, fold ? *reset : LaResetArgs<float>{});
        if (nwmax != nullptr) *nwmax = wmax != nullptr ? grid * 8u : 0u;
        ctx->first_pass_elem_bytes = 1;
        return hipGetLastError();
    }
    ctx->first_pass_elem_bytes = 2;
    hipLaunchKernelGGL((k_scr_first<TY, 4, 3>), dim3(grid), dim3(512), lds, ctx->stream, (const __half*)S->a16, ldm, (uint32_t)ctx->n, np / 32u, y,
                       S->meta, c0h, scr_skew() == 0u ? 0u : 5u, wmax);
    if (nwmax != nullptr) *nwmax = wmax != nullptr ? grid * 8u : 0u;
    return hipGetLastError();
}

bool screen_first8_folds(ss_hip_ctx* ctx)
{
    ScreenState* S = scr_of(ctx);
    return S != nullptr && !ctx->is_f64 && screen_first16_usable(ctx) && scr_first8_launchable<float>(ctx, S);
}

hipError_t launch_screen_form(ss_hip_ctx* ctx, Workspace<float>& ws, float tol, uint32_t max_iter, bool first16, bool finish, EventPair first,
                              EventPair screen, EventPair path, bool omp, bool rescue, ScrHandoff* ho)
{
    // (ho: the hand-offs inside launches of the route a single Homotopy solve takes by default — first attempt, resident path kernel, ranking
    // pass over a reduced copy, state mirrored to mapped host memory; every other route keeps the launches below as they were)
    // (rescue: the second attempt on a signal the first one declined — no first pass; the selection ranks S->rank, where the columns the
    // scan of the first attempt's log found missing sit on top: launch_screen_rescue_scan)
    // (omp: orthogonal matching pursuit on the same subset — k_res_solve<float, OMP> logs its states the same way, the certificate reads
    // "nothing outside the subset reaches the pick's |c|"; the exact re-check decides Homotopy's predicates and stays out)
    if (omp && !(ctx->screen_resident && res_solve_usable<float>())) return hipErrorInvalidConfiguration;
    ScreenState* S = scr_of(ctx);
    if (S == nullptr || ctx->sub_buf == nullptr) return hipErrorInvalidConfiguration;
    uint32_t* const fl = (ctx->screen_recheck && !omp) ? S->fl : nullptr;
    const SubBufs B = sub_bufs(ctx, 1);
    hipStream_t s = ctx->stream;
    const uint32_t ldm = ctx->ldm, n = (uint32_t)ctx->n, np = ctx->n_pad;
    const float* At = static_cast<const float*>(ctx->At);
    uint32_t nwmax = 0;
    // (ho->reset: the caller left this attempt's k_la_reset to the ranking pass — which is the first launch below, or the reset is launched here)
    const LaResetArgs<float>* const reset = ho != nullptr && ho->reset.x != nullptr ? &ho->reset : nullptr;
    if (reset != nullptr && !(first16 && !rescue)) { const hipError_t er = launch_la_reset_args<float>(ctx, *reset); if (er != hipSuccess) return er; }
    if (first16 && !rescue) {
        if (first.a) (void)hipEventRecord(first.a, s);
        { const hipError_t ef = launch_scr_first<float>(ctx, S, (const float*)ws.rhs, ws.c0, S->wmax, &nwmax, reset); if (ef != hipSuccess) return ef; }
        if (first.b) (void)hipEventRecord(first.b, s);
    }
    if (rescue) {
        if (S->rank == nullptr || !first16) return hipErrorInvalidConfiguration;
        launch_scr_rescue_rank(ctx, *S, (const float*)ws.c0);
    }
    const bool ho_route = ho != nullptr && !omp && !rescue && first16 && nwmax != 0u && ctx->handoff != nullptr && ctx->hs_mapped != nullptr &&
                          ctx->screen_resident && res_solve_usable<float>();
    if (ho_route && (ho->mask & 2u) && np <= kHoSelCols)
        (void)launch_sub_select_wide(ctx, B, (const float*)ws.c0, S->meta + 6, (const float*)S->wmax, nwmax);
    else
        (void)launch_sub_select(ctx, B, 1, rescue ? (const float*)S->rank : (const float*)ws.c0, first16 ? S->meta + 6 : nullptr,
                                nwmax != 0u ? (const float*)S->wmax : nullptr, nwmax);
    launch_sgram32(ctx, (const uint32_t*)B.sub, S->gs_part, S->gs, 1, (const float*)ws.rhs, ws.c0, first16);
    // the path on the subset: the resident kernel (resident.hip: Gram values in registers, four barriers per iteration) or, option
    // screen_resident = 0, k_sub_solve (subbatch.hip) — the same log either way (path: profiling events around it)
    const ResLog<float> log{ B.hdr, nullptr, B.pcol, B.LX, B.LD };
    if (path.a) (void)hipEventRecord(path.a, s);
    if (ctx->screen_resident && res_solve_usable<float>())
        (void)launch_res_solve<float>(ctx, 1, (const float*)S->gs, kSbS, 0, (const float*)ws.c0, 0, (const uint32_t*)B.sub, tol, max_iter, ws.dims.kcap, log, ws.x, 0,
                                      ws.gam, ws.touched, ws.st, ws.trace, ws.trace_cap, omp);
    else
        (void)launch_sub_solve(ctx, ws, B, 1, (const float*)S->gs, kSbS, first16 ? 2 : 1, ws.c0, tol, max_iter);
    if (path.b) (void)hipEventRecord(path.b, s);
    launch_scr_residuals(ctx, *S, (const float*)ws.rhs, B, tol, S->res, ws.st, 1, first16, fl, omp);
    if (screen.a) (void)hipEventRecord(screen.a, s);
    ScrPass pass;
    pass.res = S->res; pass.sub = B.sub; pass.nsub = kSbS; pass.st = ws.st;
    pass.fl = fl; pass.c0h = first16 ? (const float*)ws.c0 : nullptr;
    scr_pass<3>(ctx, *S, pass);
    if (screen.b) (void)hipEventRecord(screen.b, s);
    if (ho_route && (ho->mask & 1u) && fl != nullptr) {
        // ... and the verdict, the state and x to the caller behind them, in the same launch (the caller then queues no k_epilogue)
        uint32_t* const hw = static_cast<uint32_t*>(ctx->handoff);
        hipLaunchKernelGGL(k_scr_tail, dim3(kScrRecheckWgs), dim3(256), 0, s, At, ldm, n, (const float*)ws.rhs, (const uint32_t*)B.hdr, (const uint32_t*)B.pcol,
                           (const float*)B.LX, (const float*)B.LD, S->fl, tol, ctx->tie_guard, ws.st, ws.x, ws.gam, ws.touched, ws.trace, ws.trace_cap,
                           ho->x_dst, ho->incx, static_cast<uint32_t*>(ctx->hs_mapped), hw + kHoTicketTail);
        ho->tail_fused = true;
        return hipGetLastError();
    }
    // the columns that pass left undecided, exactly
    if (fl != nullptr) launch_scr_exact_tail<float>(ctx, ws, (const float*)ws.rhs, log, fl, tol);
    // (finish = false: the caller's epilogue launch turns "a column was not certified" into the status the host reads)
    if (finish) (void)launch_sub_finish(ctx, ws, 1);
    return hipGetLastError();
}

// The rescue of a declined solve (one fp32 signal, Homotopy; option screen_rescue).  A planted column whose |c0| drowns in the noise of the
// other planted columns is not among the 448 best-ranked: the subset's path then goes wrong where that column should have entered — it runs
// out of positions, or the certificate finds the column far above a state's bound.  Its log still says WHICH column: at the early states
// (k_scr_residuals, scan) no column that was ranked out for a good reason can reach 7/8 lambda_k, so whatever the certificate pass lists
// there is a column the ranking missed.  This queues that scan over the declined solve's log and reads the list's length back (one
// synchronisation, on the rare path); the caller then repeats the screened form with those columns forced into the subset.
// -> the number of columns found (0: nothing to rescue; > kScrRescueCap: too many)
hipError_t launch_screen_rescue_scan(ss_hip_ctx* ctx, Workspace<float>& ws, float tol, bool from_recheck, uint32_t* count_out)
{
    ScreenState* S = scr_of(ctx);
    *count_out = 0;
    if (S == nullptr || ctx->sub_buf == nullptr || S->fl == nullptr) return hipErrorInvalidConfiguration;
    const SubBufs B = sub_bufs(ctx, 1);
    if (S->rank == nullptr && S->own.device(&S->rank, (size_t)ctx->n_pad * sizeof(float)) != hipSuccess) return hipErrorOutOfMemory;
    launch_scr_residuals(ctx, *S, (const float*)ws.rhs, B, tol, S->res, ws.st, 1, true, S->fl, false, true);
    ScrPass pass;
    pass.res = S->res; pass.sub = B.sub; pass.nsub = kSbS; pass.st = ws.st;
    pass.gate = 3u; pass.fl = S->fl;
    scr_pass<3>(ctx, *S, pass);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return scr_rescue_readback(*S, ctx->stream, from_recheck, count_out);
}
uint32_t screen_rescue_cap() { return kScrRescueCap; }

static size_t scr_gemm_b_lds()
{
    return std::max<size_t>((size_t)(kScrCols + kScrSL * kScrBS) * kScrPitchB, ((size_t)kScrBS * 4 + kSbS + (size_t)128 * kScrBS) * 4);
}

// ---- a batch chunk in the screened form ------------------------------------------------------------------------------------
// The same six steps with a slot dimension: selection and the subset solves one workgroup per slot (the subset form's batch
// kernels), one subset Gram matrix per slot, and ONE screening launch whose workgroups of a tile of A16 — one per slot — are
// neighbours in the launch order: the tile comes from HBM once.  c0 of every slot comes from the batch GEMM (8.6 us per signal
// instead of a 330-us sweep each).
uint32_t screen_batch_cap() { return kScrBatch; }

hipError_t launch_screen_batch(ss_hip_ctx* ctx, Workspace<float>& ws, uint32_t nslots, const float* c0_all, float tol, uint32_t max_iter, bool omp)
{
    // (omp: the batch callers make sure the resident kernel runs — k_sub_solve has no OMP statement)
    if (omp && !(ctx->screen_resident && res_solve_usable<float>())) return hipErrorInvalidConfiguration;
    ScreenState* S = scr_of(ctx);
    if (S == nullptr || ctx->sub_buf == nullptr || nslots == 0 || nslots > kScrBatch) return hipErrorInvalidConfiguration;
    const uint32_t ldm = ctx->ldm, n = (uint32_t)ctx->n, np = ctx->n_pad;
    if (S->b_res.r16 == nullptr) {
        Takes t{ S->batch };
        S->b_res.take(t, kScrRhs, ldm, kScrBatch);
        t(&S->b_gs_part, (size_t)kScrBatch * kSgSplit * kSbS * kSbS * sizeof(float))(&S->b_gs, (size_t)kScrBatch * kSbS * kSbS * sizeof(float));
        if (!t.ok || S->b_res.clear(ldm, kScrBatch, ctx->stream) != hipSuccess) {
            static_cast<ScrBatchBufs&>(*S) = ScrBatchBufs();
            (void)hipGetLastError();
            return hipErrorOutOfMemory;
        }
    }
    const SubBufs B = sub_bufs(ctx, nslots);
    hipStream_t s = ctx->stream;
    (void)launch_sub_select(ctx, B, nslots, c0_all);
    launch_sgram32(ctx, (const uint32_t*)B.sub, S->b_gs_part, S->b_gs, nslots);
    if (ctx->screen_resident && res_solve_usable<float>()) {
        const ResLog<float> log{ B.hdr, nullptr, B.pcol, B.LX, B.LD };
        (void)launch_res_solve<float>(ctx, nslots, (const float*)S->b_gs, kSbS, (size_t)kSbS * kSbS, c0_all, np, (const uint32_t*)B.sub, tol, max_iter, ws.dims.kcap, log,
                                      ws.x, np, ws.gam, ws.touched, ws.st, ws.trace, ws.trace_cap, omp);
    } else
        (void)launch_sub_solve(ctx, ws, B, nslots, (const float*)S->b_gs, kSbS, 1, c0_all, tol, max_iter, kSbS * kSbS);
    launch_scr_residuals(ctx, *S, (const float*)ws.y, B, tol, S->b_res, ws.st, nslots, false, nullptr, omp);
    static const bool b_attr = [] {
        const bool ok = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_scr_gemm_b), hipFuncAttributeMaxDynamicSharedMemorySize, (int)scr_gemm_b_lds()) == hipSuccess;
        if (!ok) (void)hipGetLastError();
        return ok;
    }();
    if (b_attr) {
        hipLaunchKernelGGL(k_scr_gemm_b, dim3((nslots + kScrSL - 1) / kScrSL, np / kScrCols), dim3(256), scr_gemm_b_lds(), s, (const __half*)S->a16, ldm, n,
                           (const __half*)S->b_res.r16, (const float*)S->anorm, (const float*)S->b_res.rn2p, (const float*)S->b_res.tab, (const uint32_t*)B.sub,
                           (const float*)S->meta, ws.st, scr_headroom(*S), nslots, scr_skew());
    }
    // (slots whose path logged more than 64 states — and every slot, should the wide kernel's LDS request be refused)
    ScrPass pass;
    pass.res = S->b_res; pass.sub = B.sub; pass.nsub = kSbS; pass.st = ws.st;
    pass.slots = nslots; pass.nst_fixed = b_attr ? 0xffffffffu : 0u;
    scr_pass<3>(ctx, *S, pass);
    (void)launch_sub_finish(ctx, ws, nslots);
    return hipGetLastError();
}

// ---- fp64 form, host side ------------------------------------------------------------------------------------------------
static size_t s64_log_bytes()
{
    size_t b = ((size_t)kS64LogCap * 4 + 7) & ~(size_t)7;
    b += (size_t)2 * kS64LogCap * 8;
    b += (((size_t)kS64LogCap * kS64LogK * 4) + 7) & ~(size_t)7;
    b += (size_t)kS64LogCap * kS64LogK * 8;
    return b;
}

// Shape / option test and the one-time preparation: the fp16 copy of A, the column norms, the sub-context (created over the
// first kS64Sub columns: every solve gathers its own into it).
bool screen64_usable(ss_hip_ctx* ctx)
{
    if (ctx->screen_single == 0 || !ctx->is_f64 || ctx->kind != 0 || ctx->screen_failed_alloc || ctx->colshard != nullptr) return false;
    const uint32_t ldm = ctx->ldm, np = ctx->n_pad;
    if (ldm % kScrKc != 0 || np % kScrCols != 0 || ldm > 16384u) return false;
    // where it pays: a dictionary many times the sub-dictionary (option 2: from 4 x)
    if (ctx->n < (ctx->screen_single >= 2 ? 4u : 16u) * kS64Sub) return false;
    if (ctx->screen_single < 2 && (size_t)ctx->m * ctx->n < ((size_t)64 << 20)) return false;
    if (ctx->screen != nullptr) return true;
    ScreenState* S = &part<ScreenState>(ctx->screen);
    typedef ResCfg<double> RC;
    Takes t{ S->own };
    scr_take_front(t, *S, np, ldm, kS64Rhs);
    t(&S->cabs, (size_t)np * sizeof(float))(&S->sublist, ((size_t)kS64Sub + 2) * sizeof(uint32_t))(&S->xsub, (size_t)kS64Sub * sizeof(double))
     (&S->xd, (size_t)kS64LogK * (kS64Rhs + 8) * sizeof(double))(&S->ctl, 8 * sizeof(uint32_t))
     (&S->sub256, ((size_t)RC::S + 2) * sizeof(uint32_t))(&S->gs64, (size_t)RC::S * RC::S * sizeof(double))
     (&S->gs64_part, (size_t)kSg64MaxSplit * RC::S * RC::S * sizeof(double))(&S->rl_hdr, (size_t)RC::LOGCAP * 8 * sizeof(uint32_t))
     (&S->rl_H, (size_t)RC::LOGCAP * 2 * sizeof(double))(&S->rl_pcol, (size_t)RC::PCAP * sizeof(uint32_t))
     (&S->rl_X, (size_t)RC::LOGCAP * RC::PCAP * sizeof(double))(&S->rl_D, (size_t)RC::LOGCAP * RC::PCAP * sizeof(double))
     (&S->fl, (size_t)kScrFlWords * sizeof(uint32_t));
    if (t.ok) (void)hipMemsetAsync(S->fl, 0, (size_t)kScrFlWords * sizeof(uint32_t), ctx->stream);
    if (t.ok) {
        const hipError_t e = scr_pass_attr<3>(), e5 = scr_pass_attr<5>(), e4 = scr_pass_attr<4>();
        if (e != hipSuccess || e5 != hipSuccess || e4 != hipSuccess) { (void)hipGetLastError(); t.ok = false; }
    }
    if (t.ok) {
        char err[256];
        S->sub = ss_hip_homotopy_create_f64(static_cast<const double*>(ctx->At), ctx->m, kS64Sub, 1, (ptrdiff_t)ldm, ctx->device, err, sizeof(err));
        if (S->sub == nullptr) t.ok = false;
        else {
            S->sub->screen_single = 0;
            (void)hipSetDevice(ctx->device);
            t(&S->sub->slog, s64_log_bytes());
            S->sub->slog_cap = kS64LogCap;
            S->sub->slog_kmax = kS64LogK;
            // its passes: 8 column tiles only — the rows split 16 (32) ways fill the chip
            uint32_t ks = 32;
            while (ks > 1 && (ldm % (ks * 16u) != 0 || ldm / ks < 256u)) ks >>= 1;
            if (ks > 1 && S->own.device(&S->sub->pass_part, (size_t)ks * 64 * S->sub->n_pad * sizeof(double)) == hipSuccess) S->sub->pass_ksplit = (int)ks;
            else S->sub->pass_ksplit = 0;
        }
    }
    if (!t.ok) return screen_off(ctx);
    (void)hipMemsetAsync(S->meta, 0, kScrMeta * sizeof(float), ctx->stream);
    return scr_fill_front<double>(ctx, *S, 1) || screen_off(ctx);
}

// The fp64 tiers' launches of the screening pass (defined behind screen64_usable: the instantiations of k_scr_gemm keep the order the
// device code was always emitted in).  The sub-dictionary tier's choice: `states` of them in one launch — three tiles up to 96, four up to 128, five up to 160
static void scr_pass_tiles(uint32_t states, const ss_hip_ctx* ctx, const ScreenState& S, const ScrPass& p)
{
    if (states <= kScrRhs) scr_pass<3>(ctx, S, p);
    else if (states <= 128u) scr_pass<4>(ctx, S, p);
    else scr_pass<5>(ctx, S, p);
}
// the resident tier's pair: four tiles where the log holds up to 128 states, five beyond — both are queued, each looks at the log's length
static void scr_pass_gated(const ss_hip_ctx* ctx, const ScreenState& S, ScrPass p)
{
    p.gate = 1u; scr_pass<4>(ctx, S, p);
    p.gate = 2u; scr_pass<5>(ctx, S, p);
}

ss_hip_ctx* screen64_sub(ss_hip_ctx* ctx) { return scr_of(ctx) ? scr_of(ctx)->sub : nullptr; }
double* screen64_xsub(ss_hip_ctx* ctx) { return scr_of(ctx) ? scr_of(ctx)->xsub : nullptr; }

// c0 = A^T y is in c0 (device): the kS64Sub columns with the largest |c0|, gathered into the sub-context's dictionary
// (c0 == nullptr: the first pass runs here, over the fp16 copy — y = the signal (device, ldm entries): k_scr_first ranks the columns,
// the selection reports what the columns left out stay below (meta[6]), k_s64_residuals certifies state 0)
hipError_t screen64_gather(ss_hip_ctx* ctx, const double* c0, const double* y, EventPair first)
{
    ScreenState* S = scr_of(ctx);
    if (S == nullptr || S->sub == nullptr) return hipErrorInvalidConfiguration;
    hipStream_t s = ctx->stream;
    const uint32_t n = (uint32_t)ctx->n, np = ctx->n_pad;
    if (c0 != nullptr) hipLaunchKernelGGL(k_s64_cabs, dim3((np + 255) / 256), dim3(256), 0, s, c0, n, np, S->cabs);
    else {
        if (first.a) (void)hipEventRecord(first.a, s);
        const hipError_t ef = launch_scr_first<double>(ctx, S, y, S->cabs);
        if (ef != hipSuccess) return ef;
        if (first.b) (void)hipEventRecord(first.b, s);
    }
    (void)launch_select_top(ctx, S->cabs, n, np, kS64Sub, S->sublist, S->sublist + kS64Sub, reinterpret_cast<float*>(S->sublist + kS64Sub + 1),
                            c0 == nullptr ? S->meta + 6 : nullptr);
    hipLaunchKernelGGL(k_s64_gather, dim3(kS64Sub), dim3(256), 0, s, static_cast<const double*>(ctx->At), ctx->ldm, n,
                       (const uint32_t*)S->sublist, static_cast<double*>(S->sub->At));
    return hipGetLastError();
}

// After the sub-context's solve (T iterations, synchronised): the certificate of its T states against all columns, the
// solution scattered into x, the verdict into the slot's state.  y = the signal (device, ldm entries, zero padded).
hipError_t screen64_certify(ss_hip_ctx* ctx, Workspace<double>& ws, const double* y, uint32_t T, double tol, double c_inf, uint32_t K,
                            EventPair screen, bool omp, bool first16)
{
    ScreenState* S = scr_of(ctx);
    if (S == nullptr || S->sub == nullptr || T == 0u || T > kS64Rhs) return hipErrorInvalidConfiguration;
    hipStream_t s = ctx->stream;
    const uint32_t ldm = ctx->ldm, n = (uint32_t)ctx->n;
    (void)hipMemsetAsync(S->ctl, 0, 8 * sizeof(uint32_t), s);
    const unsigned char* slog = static_cast<const unsigned char*>(S->sub->slog);
    hipLaunchKernelGGL(k_s64_dense, dim3(T), dim3(256), 0, s, slog, T, S->xd, S->ctl, omp ? 1 : 0);
    hipLaunchKernelGGL(k_s64_residuals, dim3(ldm / 64u), dim3(256), 0, s, static_cast<const double*>(S->sub->At), ldm, y, slog, T,
                       (const double*)S->xd, tol, (const float*)S->meta, S->res.r16, S->res.rn2p, S->res.tab, S->ctl, scr_headroom(*S),
                       first16 ? 1 : 0);
    if (screen.a) (void)hipEventRecord(screen.a, s);
    // (up to 160 states in ONE pass over the fp16 copy — five tiles of 32 per workgroup, four up to 128: two register sets of loads in
    // flight —, the rest in passes of 96)
    ScrPass pass;
    pass.sub = S->sublist; pass.nsub = kS64Sub; pass.st = ws.st;
    for (uint32_t k0 = 0, cnt = 0; k0 < T; k0 += cnt) {
        const uint32_t left = T - k0;
        cnt = std::min<uint32_t>(left > kScrRhs ? 160u : kScrRhs, left);
        pass.res = S->res.from(k0, ldm);
        pass.nst_fixed = cnt;
        scr_pass_tiles(left, ctx, *S, pass);
    }
    if (screen.b) (void)hipEventRecord(screen.b, s);
    hipLaunchKernelGGL(k_s64_finish, dim3((kS64Sub + 255) / 256), dim3(256), 0, s, (const uint32_t*)S->sublist, (const double*)S->xsub, n, ws.x,
                       ws.st, (const uint32_t*)S->ctl, T, c_inf, K);
    return hipGetLastError();
}

// ---- fp64, resident tier (resident.hip) ---------------------------------------------------------------------------------------
// The whole solve queued in one go: the first pass over the fp16 copy (or, first16 = false, the caller's fp64 sweep in ws.c0) ranks
// the columns, the 256 best become the subset, Gs = A_S^T A_S and the exact c0 of its columns from the fp64 dictionary (MFMA),
// k_res_solve<double> runs the path in ONE workgroup — this is what is reported —, k_res_residuals64 rounds the states' residuals
// to fp16 and the screening pass certifies every state against all columns (four tiles of 32 states up to 128, five beyond: both
// launches are queued, each looks at the log's length).  The verdict reaches the host through the epilogue launch
// (DevState::need_sweep -> kStatusSubsetFail); a path that leaves the kernel's common path arrives as kStatusSubsetDecline.
bool screen64_resident_usable(ss_hip_ctx* ctx)
{
    ScreenState* S = scr_of(ctx);
    return S != nullptr && S->sub256 != nullptr && ctx->n >= 4u * (uint32_t)ResCfg<double>::S && res_solve_usable<double>();
}

// the resident solve's log of one signal
static ResLog<double> res64_log(const ScreenState& S) { return { S.rl_hdr, S.rl_H, S.rl_pcol, S.rl_X, S.rl_D }; }

// The rescue in the fp64 resident tier (see launch_screen_rescue_scan): the declined solve's log scanned by the five-tile certificate pass
// (up to 160 states in one launch), the same three lists, the same order of preference.
hipError_t launch_screen64_rescue_scan(ss_hip_ctx* ctx, Workspace<double>& ws, double tol, bool from_recheck, uint32_t* count_out)
{
    typedef ResCfg<double> RC;
    ScreenState* S = scr_of(ctx);
    *count_out = 0;
    if (S == nullptr || S->sub256 == nullptr || S->fl == nullptr) return hipErrorInvalidConfiguration;
    if (S->rank == nullptr && S->own.device(&S->rank, (size_t)ctx->n_pad * sizeof(float)) != hipSuccess) return hipErrorOutOfMemory;
    (void)launch_res_residuals64(ctx, (const double*)ws.rhs, res64_log(*S), tol, S->meta, S->res.r16, S->res.rn2p, S->res.tab, scr_headroom(*S), ws.st, true, false, 1,
                                 nullptr, S->fl, true);
    ScrPass pass;
    pass.res = S->res; pass.sub = S->sub256; pass.nsub = (uint32_t)RC::S; pass.st = ws.st;
    pass.gate = 3u; pass.fl = S->fl;
    scr_pass<5>(ctx, *S, pass);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return scr_rescue_readback(*S, ctx->stream, from_recheck, count_out);
}

hipError_t launch_screen64_resident(ss_hip_ctx* ctx, Workspace<double>& ws, double tol, uint32_t max_iter, bool first16, bool omp, EventPair first,
                                    EventPair screen, EventPair path, bool rescue)
{
    typedef ResCfg<double> RC;
    ScreenState* S = scr_of(ctx);
    if (S == nullptr || S->sub256 == nullptr) return hipErrorInvalidConfiguration;
    hipStream_t s = ctx->stream;
    const uint32_t n = (uint32_t)ctx->n, np = ctx->n_pad;
    const double* y = ws.rhs;                                     // (r = y: the caller's reset put it there)
    if (rescue) {
        // (the second attempt on a signal the tier declined: no first pass — S->cabs still holds |c~0| —, the columns the scan named on top of the ranking)
        if (S->rank == nullptr || !first16) return hipErrorInvalidConfiguration;
        launch_scr_rescue_rank(ctx, *S, (const float*)S->cabs);
    } else if (first16) {
        if (first.a) (void)hipEventRecord(first.a, s);
        const hipError_t ef = launch_scr_first<double>(ctx, S, y, S->cabs);
        if (ef != hipSuccess) return ef;
        if (first.b) (void)hipEventRecord(first.b, s);
    } else {
        hipLaunchKernelGGL(k_s64_cabs, dim3((np + 255) / 256), dim3(256), 0, s, (const double*)ws.c0, n, np, S->cabs);
    }
    (void)launch_select_top(ctx, rescue ? (const float*)S->rank : (const float*)S->cabs, n, np, (uint32_t)RC::S, S->sub256, S->sub256 + RC::S,
                            reinterpret_cast<float*>(S->sub256 + RC::S + 1), first16 ? S->meta + 6 : nullptr);
    { const hipError_t eg = launch_sgram64(ctx, S->sub256, y, S->gs64_part, S->gs64, ws.c0); if (eg != hipSuccess) return eg; }
    const ResLog<double> log = res64_log(*S);
    if (path.a) (void)hipEventRecord(path.a, s);
    { const hipError_t es = launch_res_solve<double>(ctx, 1, S->gs64, (uint32_t)RC::S, 0, ws.c0, 0, S->sub256, tol, max_iter, ws.dims.kcap, log, ws.x, 0, ws.gam,
                                                     ws.touched, ws.st, ws.trace, ws.trace_cap, omp);
      if (es != hipSuccess) return es; }
    if (path.b) (void)hipEventRecord(path.b, s);
    uint32_t* fl = (ctx->screen_recheck && !omp) ? S->fl : nullptr;      // (the exact re-check decides Homotopy's predicates: not OMP's)
    (void)launch_res_residuals64(ctx, y, log, tol, S->meta, S->res.r16, S->res.rn2p, S->res.tab, scr_headroom(*S), ws.st, first16, omp, 1, nullptr, fl);
    if (screen.a) (void)hipEventRecord(screen.a, s);
    ScrPass pass;
    pass.res = S->res; pass.sub = S->sub256; pass.nsub = (uint32_t)RC::S; pass.st = ws.st;
    pass.fl = fl; pass.c0h = first16 ? (const float*)S->cabs : nullptr;
    scr_pass_gated(ctx, *S, pass);
    if (screen.b) (void)hipEventRecord(screen.b, s);
    // the columns those passes left undecided, exactly, in fp64
    if (fl != nullptr) launch_scr_exact_tail<double>(ctx, ws, y, log, fl, tol);
    return hipGetLastError();
}

// ---- fp64 BATCHES in the resident tier -----------------------------------------------------------------------------------------
// Signals that share the dictionary share its passes and run their paths side by side:
//   k_y16_prep      every signal rounded to fp16 (scaled by a power of two), its norm, its table entry
//   k_scr_gemm<4>   ONE pass over the fp16 copy of A for up to 128 signals: |c~0| of every (signal, column) — the rankings (writing mode)
//   k_sub_select1w  the 256 best columns of each signal and what the columns left out stay below
//   k_sgram64_*     the subsets' Gram matrices and exact fp64 c0, one launch for the chunk
//   k_res_solve     the chunk's paths in as many workgroups, side by side (one signal alone leaves 255 compute units idle for 1 ms)
//   k_res_residuals64, then per signal the screening pass (its 128 states fill a launch: 0.96 ms each — what a batch costs per signal)
// What a slot's certificate does not cover is solved again, alone, through every tier (homotopy.hip: solve_batch_res64).

__global__ __launch_bounds__(256)
void k_y16_prep(const double* __restrict__ Y, uint32_t ldm, uint32_t nslots, const float* __restrict__ meta, __half* __restrict__ y16,
                float* __restrict__ ytab, float* __restrict__ ymeta)
{
    __shared__ float sv[16];
    __shared__ float s_sc;
    const uint32_t slot = blockIdx.x, tid = threadIdx.x;
    __half* out = y16 + (size_t)slot * ldm;
    if (slot >= nslots) {                                         // (rows of the 128-row block beyond the chunk)
        for (uint32_t i = tid; i < ldm; i += 256u) out[i] = __float2half_rn(0.f);
        if (tid == 0u) ytab[slot * kScrTab] = 0.f;
        return;
    }
    const double* y = Y + (size_t)slot * ldm;
    float ss = 0.f, mx = 0.f;
    for (uint32_t i = tid; i < ldm; i += 256u) { const float v = (float)y[i]; ss = __builtin_fmaf(v, v, ss); mx = fmaxf(mx, fabsf(v)); }
    ss = block_sum(ss, sv);
    __syncthreads();
    mx = fmaxf(mx, __shfl_xor(mx, 1)); mx = fmaxf(mx, __shfl_xor(mx, 2)); mx = fmaxf(mx, __shfl_xor(mx, 4));
    mx = fmaxf(mx, __shfl_xor(mx, 8)); mx = fmaxf(mx, __shfl_xor(mx, 16)); mx = fmaxf(mx, __shfl_xor(mx, 32));
    if ((tid & 63u) == 0u) sv[tid >> 6] = mx;
    __syncthreads();
    if (tid == 0u) {
        mx = fmaxf(fmaxf(sv[0], sv[1]), fmaxf(sv[2], sv[3]));
        int e = 0;
        if (mx > 0.f && mx < 3.0e38f) e = (int)floorf(log2f(4096.f / mx));      // (max |y| -> 2^11 .. 2^12: far from the fp16 ceiling)
        e = e < -100 ? -100 : (e > 100 ? 100 : e);
        const float sc = ldexpf(1.f, e);
        s_sc = sc;
        ytab[slot * kScrTab + 0] = meta[1] * ldexpf(1.f, -e);
        ytab[slot * kScrTab + 1] = 0.f; ytab[slot * kScrTab + 2] = ldexpf(1.f, -e); ytab[slot * kScrTab + 3] = 0.f;
        ymeta[slot * 4u + 0] = ss * 1.0001f;                         // (the casts of y to float: inside)
        ymeta[slot * 4u + 2] = ldexpf(1.f, -e);
    }
    __syncthreads();
    const float sc = s_sc;
    for (uint32_t i = tid; i < ldm; i += 256u) out[i] = __float2half_rn((float)y[i] * sc);
}

static Screen64Batch* s64b_of(ScreenState* S) { return S->b64.get(); }

bool screen64_batch_usable(ss_hip_ctx* ctx)
{
    return ctx->is_f64 && screen64_usable(ctx) && screen64_resident_usable(ctx) && screen_first16_usable(ctx);
}
uint32_t screen64_batch_cap() { return kS64Batch; }

// the chunk's signals are in ws.y ([nslots][ldm], zero padded), x / states / lists of the slots in ws; returns with everything queued
hipError_t launch_screen64_batch(ss_hip_ctx* ctx, Workspace<double>& ws, uint32_t nslots, double tol, uint32_t max_iter, bool omp)
{
    typedef ResCfg<double> RC;
    ScreenState* S = scr_of(ctx);
    if (S == nullptr || nslots == 0 || nslots > kS64Batch) return hipErrorInvalidConfiguration;
    const uint32_t ldm = ctx->ldm, n = (uint32_t)ctx->n, np = ctx->n_pad;
    Screen64Batch* Bq = s64b_of(S);
    if (Bq == nullptr) {
        std::unique_ptr<Screen64Batch> fresh(new (std::nothrow) Screen64Batch());
        if (!fresh) return hipErrorOutOfMemory;
        Bq = fresh.get();
        Takes t{ Bq->own };
        t(&Bq->y16, (size_t)128 * ldm * sizeof(__half))(&Bq->ytab, (size_t)128 * kScrTab * sizeof(float))(&Bq->ymeta, (size_t)kS64Batch * 4 * sizeof(float))
         (&Bq->cabs, (size_t)kS64Batch * np * sizeof(float))(&Bq->sub, ((size_t)kS64Batch * RC::S + 2) * sizeof(uint32_t))
         (&Bq->gs, (size_t)kS64Batch * RC::S * RC::S * sizeof(double))(&Bq->gs_part, (size_t)kS64Batch * kSg64MaxSplit * RC::S * RC::S * sizeof(double))
         (&Bq->hdr, (size_t)kS64Batch * RC::LOGCAP * 8 * sizeof(uint32_t))(&Bq->H, (size_t)kS64Batch * RC::LOGCAP * 2 * sizeof(double))
         (&Bq->pcol, (size_t)kS64Batch * RC::PCAP * sizeof(uint32_t))(&Bq->X, (size_t)kS64Batch * RC::LOGCAP * RC::PCAP * sizeof(double));
        Bq->res.take(t, kS64Rhs, ldm, kS64Batch);
        t(&Bq->zero, (size_t)(ldm / 64u) * 128 * sizeof(float))(&Bq->c0, (size_t)kS64Batch * np * sizeof(double));
        if (!t.ok || Bq->res.clear(ldm, kS64Batch, ctx->stream) != hipSuccess ||
            hipMemsetAsync(Bq->zero, 0, (size_t)(ldm / 64u) * 128 * sizeof(float), ctx->stream) != hipSuccess) {
            (void)hipGetLastError();
            return hipErrorOutOfMemory;      // (`fresh` gives back what it obtained)
        }
        S->b64 = std::move(fresh);
    }
    const double* Y = ws.y;
    // the signals in fp16, ONE pass over the fp16 copy for the whole chunk: |c~0| of every (signal, column)
    hipLaunchKernelGGL(k_y16_prep, dim3(128), dim3(256), 0, ctx->stream, Y, ldm, nslots, (const float*)S->meta, Bq->y16, Bq->ytab, Bq->ymeta);
    ScrPass rank;
    rank.res = ResBlock{ Bq->y16, Bq->zero, Bq->ytab, 128u };     // (the signals as right-hand sides; the writing mode reads no residual norms)
    rank.sub = Bq->sub; rank.nsub = 0u; rank.st = ws.st;
    rank.nst_fixed = nslots; rank.out_abs = Bq->cabs; rank.out_pitch = np;
    scr_pass<4>(ctx, *S, rank);
    // each signal's 256 best columns and what the columns it left out stay below
    for (uint32_t b = 0; b < nslots; ++b)
        (void)launch_select_top(ctx, Bq->cabs + (size_t)b * np, n, np, (uint32_t)RC::S, Bq->sub + (size_t)b * RC::S, S->sublist + kS64Sub,
                                reinterpret_cast<float*>(S->sublist + kS64Sub + 1), Bq->ymeta + (size_t)b * 4 + 1);
    { const hipError_t eg = launch_sgram64(ctx, Bq->sub, Y, Bq->gs_part, Bq->gs, Bq->c0, nslots, np); if (eg != hipSuccess) return eg; }
    const ResLog<double> log{ Bq->hdr, Bq->H, Bq->pcol, Bq->X, nullptr };
    { const hipError_t es = launch_res_solve<double>(ctx, nslots, Bq->gs, (uint32_t)RC::S, (size_t)RC::S * RC::S, Bq->c0, np, Bq->sub, tol, max_iter, ws.dims.kcap, log,
                                                     ws.x, np, ws.gam, ws.touched, ws.st, (TraceEntry*)nullptr, 0u, omp);
      if (es != hipSuccess) return es; }
    (void)launch_res_residuals64(ctx, Y, log, tol, S->meta, Bq->res.r16, Bq->res.rn2p, Bq->res.tab, scr_headroom(*S), ws.st, true, omp, nslots, Bq->ymeta);
    // (one slot per launch: the pass is handed the slot's block, subset and state)
    for (uint32_t b = 0; b < nslots; ++b) {
        ScrPass pass;
        pass.res = Bq->res.slot(b, ldm); pass.sub = Bq->sub + (size_t)b * RC::S; pass.nsub = (uint32_t)RC::S; pass.st = ws.st + b;
        scr_pass_gated(ctx, *S, pass);
    }
    (void)launch_sub_finish_st(ctx, ws.st, nslots);
    return hipGetLastError();
}

// developer aid (SS_HIP_SUB_DEBUG): the first (column, state) the exact re-check of the last screened solve failed, with the log around it
void screen_debug_recheck(ss_hip_ctx* ctx)
{
    ScreenState* S = scr_of(ctx);
    if (S == nullptr || S->fl == nullptr || ctx->sub_buf == nullptr) return;
    uint32_t w[kScrFlWords];
    if (hipMemcpy(w, S->fl, sizeof(w), hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return; }
    std::fprintf(stderr, "[screened form] columns left to the exact re-check: %u (state 0 among the questions: %u)\n", w[0], w[kScrFlCap + 1]);
    if (w[kScrFlCap + 4] == 0u) return;
    const SubBufs B = sub_bufs(ctx, 1);
    uint32_t hdr[kSbLog * 8];
    if (hipMemcpy(hdr, B.hdr, sizeof(hdr), hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return; }
    const uint32_t k = w[kScrFlCap + 6];
    if (k >= kSbLog) return;                                     // (the list was not written in this attempt: the solve declined before its residuals)
    float cv, qv, lam, gam, lam1 = 0.f;
    std::memcpy(&cv, &w[kScrFlCap + 7], 4); std::memcpy(&qv, &w[kScrFlCap + 8], 4);
    std::memcpy(&lam, &hdr[k * 8 + 4], 4); std::memcpy(&gam, &hdr[k * 8 + 5], 4);
    if (k + 1 < kSbLog) std::memcpy(&lam1, &hdr[(k + 1) * 8 + 4], 4);
    std::fprintf(stderr, "    first failure: column %u at state %u (P = %u, flags %u, pick %u): c = %.9g, q = %.9g, lambda = %.9g, step = %.9g, next lambda = %.9g (next flags %u); "
                 "candidates (lambda - c) / (1 - q) = %.9g, (lambda + c) / (1 + q) = %.9g\n", w[kScrFlCap + 5], k, hdr[k * 8], hdr[k * 8 + 1], hdr[k * 8 + 2], cv, qv, lam, gam,
                 lam1, k + 1 < kSbLog ? hdr[(k + 1) * 8 + 1] : 0u, (lam - cv) / (1.f - qv), (lam + cv) / (1.f + qv));
}

double screen_read_headroom(ss_hip_ctx* ctx)
{
    ScreenState* S = scr_of(ctx);
    if (S == nullptr) return 0.0;
    uint32_t bits = 0;
    if (hipMemcpy(&bits, scr_headroom(*S), sizeof(bits), hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return 0.0; }
    float f;
    std::memcpy(&f, &bits, sizeof(f));
    return (double)f;
}

}  // namespace sship
