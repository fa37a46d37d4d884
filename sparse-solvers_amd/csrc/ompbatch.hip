// ompbatch.hip — orthogonal matching pursuit for BATCHES of signals in the Gram form (G = A^T A resident in HBM).
//
// Per chunk of slots (the host side is solve_omp_batch_f32 in homotopy.hip):
//   c0          = A^T y of every slot, by the batch GEMM (gemm.hip), into c0_all [nslots][n_pad]
//   k_sub_select  the 448 columns with the largest |c0| of every slot (subbatch.hip)
//   k_omp_sgather the subset's Gram matrix gathered from G: 448 x 448 entries per slot (no pass over A)
//   k_res_solve<float, OMP>  the path on the subset, one workgroup per slot; every state's x by position is logged (resident.hip)
//   k_omp_gverify the certificate: for every slot, logged state k and column j outside the subset
//                   c_k(j) = c0_j - sum_p X_k[p] G[col_p][j]
//                 on v_mfma_f32_32x32x2_f32 (states x positions against positions x 32 columns), with a rigorous bound on the
//                 rounding of that evaluation; a slot with any (state, column) pair above its bound is declined.
//                 What is certified is the Gram-form statement on the stored c0 and G — the quantity the default OMP engine
//                 (k_la_omp) evaluates — as the screened form certifies against the fp32 residual its engine forms.
//   k_sub_finish  the verdicts into the slots' status words
#include "ss_hip_internal.h"
#include "resident.h"

namespace sship {

namespace {

constexpr uint32_t kOgWaveCols = 32;                       // columns of one MFMA tile
constexpr uint32_t kOgGroups = 4;                          // 32-column groups a wave walks through
constexpr uint32_t kOgCols = 4 * kOgWaveCols * kOgGroups;  // columns per workgroup (four waves)
constexpr uint32_t kOgTiles = 3;                           // 32-state tiles: the log holds at most kSbLog - 1 = 79 states
constexpr uint32_t kOgStates = 32 * kOgTiles;
constexpr uint32_t kOgXPitch = kSbRows + 1;                // (odd pitch: the 32 rows of an A operand fall in distinct banks)
constexpr uint32_t kOgSteps = kSbRows / 2;                 // k-steps of two positions
static_assert(kSbLog - 1 <= kOgStates, "every logged state must fit a state tile");
static_assert(kSbRows % 2 == 0, "positions come in k-steps of two");

typedef float og_f32x16 __attribute__((ext_vector_type(16)));

}  // namespace

constexpr uint32_t kOmpGramChunk = 256;                    // slots per chunk of the Gram form

// column norms ||a_j|| in fp64, rounded up into fp32 (the error bound's scale); padding columns 0.  One wave per column.
__global__ __launch_bounds__(256)
void k_omp_colnorm(const float* __restrict__ At, uint32_t ldm, uint32_t n, uint32_t np, float* __restrict__ norm,
                   const uint32_t* __restrict__ list, uint32_t nlist)
{
    // (list: only those columns — the ones a replacement rewrote)
    const uint32_t w = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (list != nullptr && w >= nlist) return;
    const uint32_t j = list != nullptr ? list[w] : w;
    if (j >= np) return;
    double s = 0.0;
    if (j < n)
        for (uint32_t i = lane; i < ldm; i += 64u) { const double a = At[(size_t)j * ldm + i]; s += a * a; }
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0u) norm[j] = j < n ? (float)sqrt(s) * (1.f + 1.0e-6f) : 0.f;
}

// the subset's Gram matrix from G: Gs[slot][i][j] = G[sub_i][sub_j] (row i of a slot per workgroup)
__global__ __launch_bounds__(256)
void k_omp_sgather(const float* __restrict__ G, uint32_t gpitch, uint32_t n, const uint32_t* __restrict__ sub_all, float* __restrict__ gs_all)
{
    const uint32_t slot = blockIdx.y, i = blockIdx.x;
    const uint32_t* sub = sub_all + (size_t)slot * kSbS;
    float* gs = gs_all + ((size_t)slot * kSbS + i) * kSbS;
    const uint32_t ci = sub[i];
    for (uint32_t jj = threadIdx.x; jj < kSbS; jj += 256u) {
        const uint32_t cj = sub[jj];
        gs[jj] = (ci < n && cj < n) ? G[(size_t)ci * gpitch + cj] : 0.f;
    }
}

// The certificate of the Gram form.  Workgroup = 512 columns of one slot (four waves, each walks four groups of 32); per group the
// P rows of G at the slot's positions are loaded once (one value per lane and k-step, all in flight together) and serve every
// state tile: acc[t] += X[32t + i][p] * G[col_p][j] on v_mfma_f32_32x32x2_f32.  A state tile stops at the positions its states use
// (state k holds k positions).  The test, per (state k, column j outside the subset):
//     |c0_j - acc| + eps <= bound_k,   eps = gamma * (|c0_j| + 1.01 ||a_j|| S_k),   S_k = sum_p |X_k[p]| ||a_p||
// with gamma = 1.01 (P + 2) 2^-24 (an fma chain of P terms and the subtraction; |G_pj| <= (1 + 2^-10) ||a_p|| ||a_j|| for the stored
// G of any ldm <= 16384) and bound_k that of k_scr_residuals in OMP mode (7/8 lambda_k, the final state 15/16 tol).
__global__ __launch_bounds__(256)
void k_omp_gverify(const float* __restrict__ G, uint32_t gpitch, uint32_t n, uint32_t ldm, const float* __restrict__ c0_all, uint32_t c0_stride,
                   const float* __restrict__ norm, const uint32_t* __restrict__ sub_all,
                   const uint32_t* __restrict__ hdr_all, const uint32_t* __restrict__ pcol_all, const float* __restrict__ LX_all, float tol,
                   DevState* __restrict__ st_all)
{
    __shared__ float sX[kOgStates][kOgXPitch];
    __shared__ float sBound[kOgStates], sS[kOgStates], sN[kSbRows];
    __shared__ uint32_t sCol[kSbRows], sPt[kOgTiles], sIn[kOgCols / 32];
    __shared__ uint32_t sFail;
    const uint32_t slot = blockIdx.y, tid = threadIdx.x;
    DevState* st = st_all + slot;
    if (st->status != 0u) return;                                   // (declined by the path kernel)
    const uint32_t nlog = st->solo_nlog;
    if (nlog < 2u) return;                                          // (no state after the first: the selection covers state 0)
    const uint32_t nst = nlog - 1u;
    const uint32_t* hdr = hdr_all + (size_t)slot * kSbLog * 8u;
    const uint32_t* pcol = pcol_all + (size_t)slot * kSbRows;
    const float* LX = LX_all + (size_t)slot * kSbLog * kSbRows;
    const uint32_t* sub = sub_all + (size_t)slot * kSbS;
    const float* c0 = c0_all + (size_t)slot * c0_stride;
    const uint32_t Pfin = min(hdr[(size_t)nst * 8u], kSbRows);
    const uint32_t j0 = blockIdx.x * kOgCols;

    if (tid < kOgCols / 32) sIn[tid] = 0u;
    if (tid == 0u) sFail = 0u;
    for (uint32_t p = tid; p < kSbRows; p += 256u) {
        const uint32_t col = p < Pfin ? pcol[p] : 0u;
        sCol[p] = col < n ? col : 0u;
        sN[p] = (p < Pfin && col < n) ? norm[col] : 0.f;
    }
    for (uint32_t e = tid; e < kOgStates * kSbRows; e += 256u) {
        const uint32_t kk = e / kSbRows, p = e - kk * kSbRows;      // (row kk = state kk + 1)
        float v = 0.f;
        if (kk < nst && p < hdr[(size_t)(kk + 1u) * 8u]) v = LX[(size_t)(kk + 1u) * kSbRows + p];
        sX[kk][p] = v;
    }
    __syncthreads();
    for (uint32_t i = tid; i < kSbS; i += 256u) {
        const uint32_t d = sub[i] - j0;                             // (unsigned: columns left of the tile wrap around)
        if (d < kOgCols) atomicOr(&sIn[d >> 5], 1u << (d & 31u));
    }
    if (tid < kOgStates) {
        const uint32_t kk = tid;
        float bound = 3.0e38f, s = 0.f;
        if (kk < nst) {
            const uint32_t* hh = hdr + (size_t)(kk + 1u) * 8u;
            const float lam = __uint_as_float(hh[4]);
            const bool final_state = !(hh[1] & 1u);
            const float slack = 1e-5f * st->lambda0;
            bound = (final_state && !(lam > tol) ? tol * 0.9375f : lam * 0.875f) - slack;
            for (uint32_t p = 0; p < Pfin; ++p) s = __builtin_fmaf(fabsf(sX[kk][p]), sN[p], s);
            s *= 1.f + 1.0e-4f;                                     // (the sum's own rounding: at most 72 terms)
        }
        sBound[kk] = bound;
        sS[kk] = s;
    }
    if (tid < kOgTiles) {
        uint32_t pm = 0u;
        for (uint32_t kk = 32u * tid; kk < 32u * tid + 32u && kk < nst; ++kk) pm = max(pm, min(hdr[(size_t)(kk + 1u) * 8u], kSbRows));
        sPt[tid] = pm;
    }
    __syncthreads();

    const uint32_t lane = tid & 63u, wave = tid >> 6, li = lane & 31u, half = lane >> 5;
    const uint32_t ntiles = (nst + 31u) / 32u;
    const float gam = 1.01f * (float)(Pfin + 2u) * 5.9604645e-8f;
    bool fail = false;
    for (uint32_t g = 0; g < kOgGroups; ++g) {
        const uint32_t jw = j0 + (wave * kOgGroups + g) * kOgWaveCols;
        if (jw >= n) break;                                          // (wave-uniform)
        const uint32_t j = jw + li;
        float bv[kOgSteps];
#pragma unroll
        for (uint32_t s = 0; s < kOgSteps; ++s) {
            const uint32_t p = 2u * s + half;
            bv[s] = (p < Pfin && j < n) ? G[(size_t)sCol[p] * gpitch + j] : 0.f;
        }
        og_f32x16 acc[kOgTiles];
#pragma unroll
        for (uint32_t t = 0; t < kOgTiles; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
#pragma unroll
        for (uint32_t s = 0; s < kOgSteps; ++s) {
            if (2u * s >= Pfin) break;                               // (uniform)
#pragma unroll
            for (uint32_t t = 0; t < kOgTiles; ++t) {
                if (t < ntiles && 2u * s < sPt[t]) {                 // (uniform: the tile's states use these positions)
                    const float a = sX[32u * t + li][2u * s + half];
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv[s], acc[t], 0, 0, 0);
                }
            }
        }
        const uint32_t d = j - j0;
        const bool outside = j < n && !((sIn[d >> 5] >> (d & 31u)) & 1u);
        if (outside) {
            const float c0j = c0[j], nj = norm[j];
#pragma unroll
            for (uint32_t t = 0; t < kOgTiles; ++t) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const uint32_t kk = 32u * t + (uint32_t)((r & 3) + 8 * (r >> 2)) + 4u * half;   // (C/D row of register r)
                    if (t < ntiles && kk < nst) {
                        const float av = acc[t][r];
                        const float c = c0j - av;
                        const float eps = gam * (fabsf(c0j) + 1.01f * nj * sS[kk]);
                        if (!(fabsf(c) + eps <= sBound[kk])) fail = true;
                    }
                }
            }
        }
    }
    if (fail) sFail = 1u;
    __syncthreads();
    if (tid == 0u && sFail != 0u) {
        __hip_atomic_store(&st->need_sweep, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // (read by k_sub_finish)
        atomicOr(&st->sub_reason, kReasonColumn);
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
bool omp_gram_usable(ss_hip_ctx* ctx)
{
    // (ldm <= 16384: the bound on the stored G's entries above)
    return !ctx->is_f64 && ctx->kind == 0 && ctx->colshard == nullptr && ctx->gram_full != nullptr && ctx->n >= kSbS && ctx->ldm <= 16384u &&
           sub_form_usable(ctx) && res_solve_usable<float>();
}

uint32_t omp_gram_cap() { return kOmpGramChunk; }

hipError_t launch_omp_gram_batch(ss_hip_ctx* ctx, Workspace<float>& ws, uint32_t nslots, const float* c0_all, float tol, uint32_t max_iter)
{
    if (ctx->gram_full == nullptr || ctx->sub_buf == nullptr || nslots == 0 || nslots > kOmpGramChunk) return hipErrorInvalidConfiguration;
    const uint32_t ldm = ctx->ldm, n = (uint32_t)ctx->n, np = ctx->n_pad;
    hipStream_t s = ctx->stream;
    if (ctx->omp_gs == nullptr) {
        // (both or neither: omp_gs is what says the pair exists)
        if (ctx->own.device(&ctx->omp_gs, (size_t)kOmpGramChunk * kSbS * kSbS * sizeof(float)) != hipSuccess) return hipErrorOutOfMemory;
        if (ctx->own.device(&ctx->omp_norm, (size_t)np * sizeof(float)) != hipSuccess) { (void)ctx->own.drop(ctx->omp_gs); return hipErrorOutOfMemory; }
        hipLaunchKernelGGL(k_omp_colnorm, dim3((np + 3u) / 4u), dim3(256), 0, s, static_cast<const float*>(ctx->At), ldm, n, np, ctx->omp_norm,
                           (const uint32_t*)nullptr, 0u);
    }
    const SubBufs B = sub_bufs(ctx, nslots);
    (void)launch_sub_select(ctx, B, nslots, c0_all);
    hipLaunchKernelGGL(k_omp_sgather, dim3(kSbS, nslots), dim3(256), 0, s, (const float*)ctx->gram_full, ctx->gram_pitch, n, (const uint32_t*)B.sub, ctx->omp_gs);
    const ResLog<float> log{ B.hdr, nullptr, B.pcol, B.LX, B.LD };
    { const hipError_t es = launch_res_solve<float>(ctx, nslots, (const float*)ctx->omp_gs, kSbS, (size_t)kSbS * kSbS, c0_all, np, (const uint32_t*)B.sub, tol,
                                                    max_iter, ws.dims.kcap, log, ws.x, np, ws.gam, ws.touched, ws.st, (TraceEntry*)nullptr, 0u, true);
      if (es != hipSuccess) return es; }
    hipLaunchKernelGGL(k_omp_gverify, dim3((n + kOgCols - 1u) / kOgCols, nslots), dim3(256), 0, s, (const float*)ctx->gram_full, ctx->gram_pitch, n, ldm,
                       c0_all, np, (const float*)ctx->omp_norm, (const uint32_t*)B.sub, (const uint32_t*)B.hdr,
                       (const uint32_t*)B.pcol, (const float*)B.LX, tol, ws.st);
    (void)launch_sub_finish_st(ctx, ws.st, nslots);
    return hipGetLastError();
}

hipError_t omp_norm_refresh(ss_hip_ctx* ctx, const uint32_t* cols_dev, uint32_t S)
{
    if (ctx->omp_norm == nullptr || S == 0) return hipSuccess;
    hipLaunchKernelGGL(k_omp_colnorm, dim3((S + 3u) / 4u), dim3(256), 0, ctx->stream, static_cast<const float*>(ctx->At), ctx->ldm, (uint32_t)ctx->n, ctx->n_pad,
                       ctx->omp_norm, cols_dev, S);
    return hipGetLastError();
}

}  // namespace sship
