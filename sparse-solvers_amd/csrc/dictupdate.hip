// dictupdate.hip — a few columns of a live context's dictionary replaced in place (ss_hip_homotopy_replace_columns_*).
//
// A context keeps more than its column-contiguous copy At of A: the screened forms' fp16 and fp8 copies with the column norms and the
// two global power-of-two scales (screen.hip), the OMP certificate's norms (ompbatch.hip), G = A^T A (homotopy.hip).  Afterwards
// every one of them is, word for word, what a context created from the updated matrix holds (DESIGN.md §3.13c lists them):
//
//   k_du_columns   one workgroup per replaced column: reads the new column once from the caller's strided view (a host V was staged
//                  by one upload), writes the At column with 16-byte stores (rows >= m: zeros), forms the column's sum of squares and
//                  max |a| from the same registers — the statements and the reduction order of k_a16_stats, so the norm is the same
//                  word — and writes the fp16 / fp8 columns under the CURRENT scales where those copies exist
//   k_du_scales    one workgroup: max |A| and max ||a_i|| again from the per-column arrays (a maximum made by atomicMax cannot go
//                  down; n floats each), the two scale exponents from them, and a flag per copy whose exponent moved — only then
//                  does the host queue the preparation's own conversion pass over that copy
//   G              the tiles of the symmetric build that meet a replaced column (gemm.hip: the same kernel, the same chains), or the
//                  whole build into the existing allocation when every tile holds one (the refresh is never more tiles than the build)
//
// No floating-point atomics: every sum is a per-thread chain and a fixed tree.
#include "ss_hip_internal.h"
#include "ss_hip_device.h"
#include "host_common.h"

#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

namespace sship {

typedef float du_f4 __attribute__((ext_vector_type(4)));
typedef double du_d2 __attribute__((ext_vector_type(2)));
typedef _Float16 du_h4 __attribute__((ext_vector_type(4)));

// V(i, s) = V[i * rs + s * cs]; column cols[s] of At (and of a16, a8 where they exist: null = not made yet)
template <typename T>
__global__ __launch_bounds__(256)
void k_du_columns(const T* __restrict__ V, long long rs, long long cs, const uint32_t* __restrict__ cols, uint32_t m, uint32_t ldm,
                  T* __restrict__ At, _Float16* __restrict__ a16, uint8_t* __restrict__ a8, float* __restrict__ anorm,
                  float* __restrict__ amaxc, const float* __restrict__ meta)
{
    __shared__ float sv[16];
    const uint32_t s = blockIdx.x, col = cols[s];
    const T* v = V + (long long)s * cs;
    T* at = At + (size_t)col * ldm;
    const T sA = a16 != nullptr ? (T)meta[0] : T(0), s8 = a8 != nullptr ? (T)meta[10] : T(0);
    float ss = 0.f, mx = 0.f;
    // (k_a16_stats: a thread's rows are 4 * tid .. + 3, then 1024 further on)
    for (uint32_t r = threadIdx.x * 4u; r < ldm; r += 1024u) {
        T a[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) a[e] = (r + (uint32_t)e < m) ? v[(long long)(r + (uint32_t)e) * rs] : T(0);
        if constexpr (sizeof(T) == 4) {
            *reinterpret_cast<du_f4*>(at + r) = du_f4{ a[0], a[1], a[2], a[3] };
        } else {
            *reinterpret_cast<du_d2*>(at + r) = du_d2{ a[0], a[1] };
            *reinterpret_cast<du_d2*>(at + r + 2u) = du_d2{ a[2], a[3] };
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) { const float f = (float)a[e]; ss = __builtin_fmaf(f, f, ss); mx = fmaxf(mx, fabsf(f)); }
        if (a16 != nullptr) {
            // (k_a16_convert: the product in T, one rounding to half)
            du_h4 h;
#pragma unroll
            for (int e = 0; e < 4; ++e) h[e] = (_Float16)(a[e] * sA);
            *reinterpret_cast<du_h4*>(a16 + (size_t)col * ldm + r) = h;
        }
        if (a8 != nullptr) {
            // (k_a8_convert)
            int p = 0;
            p = __builtin_amdgcn_cvt_pk_fp8_f32((float)(a[0] * s8), (float)(a[1] * s8), p, false);
            p = __builtin_amdgcn_cvt_pk_fp8_f32((float)(a[2] * s8), (float)(a[3] * s8), p, true);
            *reinterpret_cast<uint32_t*>(a8 + (size_t)col * ldm + r) = (uint32_t)p;
        }
    }
    if (anorm == nullptr) return;           // (uniform: no screened copies, nobody reads the statistics)
    ss = block_sum(ss, sv);
    __syncthreads();
    mx = fmaxf(mx, __shfl_xor(mx, 1)); mx = fmaxf(mx, __shfl_xor(mx, 2)); mx = fmaxf(mx, __shfl_xor(mx, 4));
    mx = fmaxf(mx, __shfl_xor(mx, 8)); mx = fmaxf(mx, __shfl_xor(mx, 16)); mx = fmaxf(mx, __shfl_xor(mx, 32));
    if ((threadIdx.x & 63u) == 0u) sv[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        anorm[col] = sqrtf(ss) * 1.0001f;
        amaxc[col] = fmaxf(fmaxf(sv[0], sv[1]), fmaxf(sv[2], sv[3]));
    }
}

// meta[2] = max |A|, meta[4] = max ||a_i|| from the per-column arrays (non-negative floats order like their bits: the order
// atomicMax gave them in k_a16_stats), the scales from them; moved[0] / moved[1] = 1 where the fp16 / fp8 scale changed
__global__ __launch_bounds__(1024)
void k_du_scales(const float* __restrict__ amaxc, const float* __restrict__ anorm, uint32_t np, float* __restrict__ meta, int have8,
                 uint32_t* __restrict__ moved)
{
    __shared__ uint32_t sa[16], sn[16];
    uint32_t ma = 0u, mn = 0u;
    for (uint32_t i = threadIdx.x; i < np; i += 1024u) {
        ma = max(ma, __float_as_uint(amaxc[i]));
        mn = max(mn, __float_as_uint(anorm[i]));
    }
    for (int o = 32; o >= 1; o >>= 1) { ma = max(ma, (uint32_t)__shfl_xor((int)ma, o)); mn = max(mn, (uint32_t)__shfl_xor((int)mn, o)); }
    if ((threadIdx.x & 63u) == 0u) { sa[threadIdx.x >> 6] = ma; sn[threadIdx.x >> 6] = mn; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < 16; ++w) { ma = max(ma, sa[w]); mn = max(mn, sn[w]); }
    uint32_t* mw = reinterpret_cast<uint32_t*>(meta);
    mw[2] = ma;
    mw[4] = mn;
    if (meta[14] != 0.f) {                  // (k_a16_scale: the units of an fp64 dictionary's columns follow max ||a_i||)
        const int u = dict_unit_exp(__uint_as_float(mn));
        meta[12] = ldexpf(1.f, -u);
        meta[13] = ldexpf(1.f, u);
    }
    const float amax = __uint_as_float(ma);
    const int e16 = pow2_scale_exp(16384.f, amax);
    const float s16 = ldexpf(1.f, e16);
    moved[0] = s16 != meta[0] ? 1u : 0u;
    meta[0] = s16;
    meta[1] = ldexpf(1.f, -e16);
    moved[1] = 0u;
    if (have8) {
        const int e8 = pow2_scale_exp(224.f, amax);
        const float s8 = ldexpf(1.f, e8);
        moved[1] = s8 != meta[10] ? 1u : 0u;
        meta[10] = s8;
        meta[11] = ldexpf(1.f, -e8);
    }
}

namespace {

// the step-aside windows and failure counts were learned on another dictionary (the call counters stay: they count calls)
void reset_routing(ss_hip_ctx* ctx)
{
    ctx->sub_aside.reset();
    ctx->res_aside.reset();
    ctx->sub_off_chunks = 0;
    ctx->solo_off_solves = 0;
    ctx->solo_seen = 0;
    ctx->solo_failed = 0;
}

// the body of replace_columns_device (file-local: the lambda it hands to guarded stays out of the library's symbols)
template <typename T>
int replace_device_impl(ss_hip_ctx* ctx, const uint32_t* dcols, const std::vector<uint32_t>& hc, const T* dV, long long drs, long long dcs,
                        char* err, size_t errlen)
{
    const size_t S = hc.size();
    if (S == 0) return SS_HIP_OK;
    DeviceBuf scratch_buf;       // (freed after the last synchronisation, or on the way out with an error)
    return guarded(err, errlen, "replace_columns", [&]() -> int {
        HIPCHK(hipSetDevice(ctx->device));
        const size_t m = ctx->m;
        const uint32_t ldm = ctx->ldm, np = ctx->n_pad, ntiles = np / kGramTile;
        // ---- G: which 128-column tiles hold a replaced column ([0 .. ntiles) flags, then the list) ----
        const bool with_g = ctx->gram_full != nullptr && np % kGramTile == 0;
        std::vector<uint32_t> tiles;
        uint32_t ntouched = 0;
        bool g_full = false;
        if (ctx->gram_full != nullptr && !with_g) g_full = true;
        if (with_g) {
            tiles.assign(ntiles, 0u);
            for (uint32_t c : hc) tiles[c / kGramTile] = 1u;
            for (uint32_t t = 0; t < ntiles; ++t) if (tiles[t]) tiles.push_back(t);
            ntouched = (uint32_t)tiles.size() - ntiles;
            // (the refresh forms ntouched * ntiles - ntouched (ntouched - 1) / 2 of the build's ntiles (ntiles + 1) / 2 tiles: as many
            // only when every tile holds a replaced column — then the build itself runs)
            g_full = ntouched == ntiles;
        }
        // ---- one scratch allocation: the tile table, the two flags ----
        auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
        const size_t off_flag = up(tiles.size() * sizeof(uint32_t));
        scratch_buf.alloc(off_flag + 256, "hipMalloc(&scratch, off_flag + 256)");
        unsigned char* scratch = scratch_buf.get<unsigned char>();
        hipStream_t st = ctx->stream;
        if (!tiles.empty()) HIPCHK(hipMemcpyAsync(scratch, tiles.data(), tiles.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        uint32_t* dmoved = reinterpret_cast<uint32_t*>(scratch + off_flag);
        // ---- the columns, their statistics, the reduced-precision columns ----
        const ScreenCopies sc = screen_copies(ctx);
        hipLaunchKernelGGL((k_du_columns<T>), dim3((uint32_t)S), dim3(256), 0, st, dV, drs, dcs, dcols, (uint32_t)m, ldm, static_cast<T*>(ctx->At),
                           static_cast<_Float16*>(sc.a16), sc.a8, sc.anorm, sc.amaxc, (const float*)sc.meta);
        HIPCHK(hipGetLastError());
        if (sc.anorm != nullptr) {
            hipLaunchKernelGGL(k_du_scales, dim3(1), dim3(1024), 0, st, (const float*)sc.amaxc, (const float*)sc.anorm, np, sc.meta, sc.a8 != nullptr ? 1 : 0, dmoved);
            HIPCHK(hipGetLastError());
            uint32_t moved[2] = { 0u, 0u };
            HIPCHK(hipMemcpyAsync(moved, dmoved, sizeof(moved), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));                       // (the one host read: is a whole copy due again?)
            if (moved[0] || moved[1]) HIPCHK(screen_reconvert(ctx, moved[0] != 0u, moved[1] != 0u));
        }
        HIPCHK(omp_norm_refresh(ctx, dcols, (uint32_t)S));
        // ---- G ----
        if (ctx->gram_full != nullptr) {
            if (g_full) {
                HIPCHK(ctx->gram_symmetric ? launch_gemm_sym_f32(ctx, ctx->gram_full, ctx->gram_pitch)
                                           : launch_gemm_tn_f32(ctx, static_cast<const float*>(ctx->At), np, ldm, ctx->gram_full, ctx->gram_pitch, nullptr, false));
            } else {
                HIPCHK(launch_gemm_sym_tiles_f32(ctx, ctx->gram_full, ctx->gram_pitch, reinterpret_cast<const uint32_t*>(scratch), ntouched));
            }
        }
        // ---- Gram columns cached in the workspace: a solve clears the slot map before it caches anything (k_la_reset), the column
        // form's table and the early form's subset are made per call — nothing of them outlives a call; the map is cleared all the same
        if (ctx->ws != nullptr) {
            int32_t* slot_of = ctx->is_f64 ? ctx->ws.as<Workspace<double>>()->slot_of : ctx->ws.as<Workspace<float>>()->slot_of;
            if (slot_of != nullptr) HIPCHK(hipMemsetAsync(slot_of, 0xff, (size_t)np * sizeof(int32_t), st));
        }
        HIPCHK(hipStreamSynchronize(st));
        reset_routing(ctx);
        if (sc.sub != nullptr) reset_routing(sc.sub);
        return SS_HIP_OK;
    });
}

}  // namespace

// The update itself, for a validated list (distinct columns < n; hc = its host copy) and columns that are on the device already:
// V(i, s) = V[i * rs + s * cs].  What ss_hip_homotopy_replace_columns_* runs after its validation and staging, and what the
// atom update of dictionary learning (dictlearn.hip) applies its changed atoms with.  Returns when the update is complete.
template <typename T>
int replace_columns_device(ss_hip_ctx* ctx, const uint32_t* dcols, const std::vector<uint32_t>& hc, const T* dV, long long drs, long long dcs,
                           char* err, size_t errlen)
{
    return replace_device_impl<T>(ctx, dcols, hc, dV, drs, dcs, err, errlen);
}

template int replace_columns_device<float>(ss_hip_ctx*, const uint32_t*, const std::vector<uint32_t>&, const float*, long long, long long, char*, size_t);
template int replace_columns_device<double>(ss_hip_ctx*, const uint32_t*, const std::vector<uint32_t>&, const double*, long long, long long, char*, size_t);

namespace {

template <typename T>
int replace_impl(ss_hip_ctx* ctx, const uint32_t* cols, size_t S, const T* V, ptrdiff_t rs, ptrdiff_t cs, char* err, size_t errlen)
{
    if (!ctx) { set_err(err, errlen, "replace_columns: null context"); return SS_HIP_EINVAL; }
    if (ctx->kind != 0) { set_err(err, errlen, "replace_columns: an IRLS context holds the factorised matrix (not supported)"); return SS_HIP_EINVAL; }
    if (ctx->colshard != nullptr) { set_err(err, errlen, "replace_columns: column-sharded contexts are not supported"); return SS_HIP_EINVAL; }
    if (ctx->is_f64 != (sizeof(T) == 8)) { set_err(err, errlen, "replace_columns: element type of the call does not match the context"); return SS_HIP_ETYPE; }
    if (S == 0) return SS_HIP_OK;
    if (!cols || !V) { set_err(err, errlen, "replace_columns: null argument"); return SS_HIP_EINVAL; }
    if (S > ctx->n) { set_err(err, errlen, "replace_columns: more columns than the dictionary has (a column is named twice)"); return SS_HIP_EINVAL; }
    DeviceBuf scratch_buf;
    return guarded(err, errlen, "replace_columns", [&]() -> int {
        HIPCHK(hipSetDevice(ctx->device));
        const size_t m = ctx->m, n = ctx->n;
        const bool cols_dev = on_device(cols), v_dev = on_device(V);
        // ---- validation, on a host copy of the list: nothing has been written when it fails ----
        std::vector<uint32_t> hc(S);
        if (cols_dev) HIPCHK(hipMemcpy(hc.data(), cols, S * sizeof(uint32_t), hipMemcpyDeviceToHost));
        else std::memcpy(hc.data(), cols, S * sizeof(uint32_t));
        {
            std::vector<uint32_t> sorted(hc);
            std::sort(sorted.begin(), sorted.end());
            if (sorted.back() >= n) { set_err(err, errlen, "replace_columns: column index out of range"); return SS_HIP_EINVAL; }
            if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) { set_err(err, errlen, "replace_columns: a column is named twice"); return SS_HIP_EINVAL; }
        }
        // ---- the list and a host V staged on the device (one allocation), then the update itself ----
        auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
        const size_t off_v = up(S * sizeof(uint32_t));
        hipStream_t st = ctx->stream;
        const uint32_t* dcols = cols;
        const T* dV = V;
        long long drs = rs, dcs = cs;
        std::vector<T> pack;
        if (!cols_dev || !v_dev) scratch_buf.alloc(off_v + (v_dev ? 0 : S * m * sizeof(T)), "hipMalloc(&scratch, off_v + (v_dev ? 0 : S * m * sizeof(T)))");
        unsigned char* scratch = scratch_buf.get<unsigned char>();
        if (!cols_dev) {
            HIPCHK(hipMemcpyAsync(scratch, hc.data(), S * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            dcols = reinterpret_cast<const uint32_t*>(scratch);
        }
        if (!v_dev) {
            // the S new columns, contiguous, through one upload of S * m elements
            pack.resize(S * m);
            for (size_t s = 0; s < S; ++s)
                for (size_t i = 0; i < m; ++i) pack[s * m + i] = V[(ptrdiff_t)i * rs + (ptrdiff_t)s * cs];
            HIPCHK(hipMemcpyAsync(scratch + off_v, pack.data(), S * m * sizeof(T), hipMemcpyHostToDevice, st));
            dV = reinterpret_cast<const T*>(scratch + off_v);
            drs = 1;
            dcs = (long long)m;
        }
        return replace_columns_device<T>(ctx, dcols, hc, dV, drs, dcs, err, errlen);
    });
}

}  // namespace
}  // namespace sship

extern "C" {

int ss_hip_homotopy_replace_columns_f32(ss_hip_ctx* ctx, const uint32_t* cols, size_t S, const float* V, ptrdiff_t stride_row, ptrdiff_t stride_col,
                                        char* err, size_t errlen)
{
    return sship::replace_impl<float>(ctx, cols, S, V, stride_row, stride_col, err, errlen);
}

int ss_hip_homotopy_replace_columns_f64(ss_hip_ctx* ctx, const uint32_t* cols, size_t S, const double* V, ptrdiff_t stride_row, ptrdiff_t stride_col,
                                        char* err, size_t errlen)
{
    return sship::replace_impl<double>(ctx, cols, S, V, stride_row, stride_col, err, errlen);
}

}  // extern "C"
