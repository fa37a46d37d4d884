// homotopy.hip — the C-ABI of libss_hip.so (include/ss_hip.h): context creation (upload +
// re-layout of the sensing matrix), the host side of the device-resident Homotopy loop,
// the standalone sweep entry and the measurement hooks.
//
// Reference being replaced (paths under /root/reference):
//   ss::solver<T,P>::solver / homotopy_policy state   include/ss/ss.h:98-105, policies.h:42
//   solve_homotopy::op<mode,T> / run_solver<T>         src/solvers/homotopy.h:27-38,
//                                                      src/solvers/homotopy-cpu.cpp:186-275
//
// Execution model: one HIP stream per context.  A solve enqueues, per homotopy
// iteration ("round"), one fused sweep kernel and five small kernels; termination is
// decided ON THE DEVICE (k_select raises DevState::done, after which every kernel is a
// no-op), the host only polls a copy of that flag `lookahead` rounds behind the queue
// head, so the GPU never waits for the host between iterations.
#include "ss_hip_internal.h"
#include "host_common.h"
#include "resident.h"

#include <algorithm>
#include <cfloat>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <limits>
#include <new>
#include <thread>

using namespace sship;

namespace sship {

void set_err(char* err, size_t errlen, const std::string& msg)
{
    if (!err || errlen == 0) return;
    const size_t k = std::min(errlen - 1, msg.size());
    std::memcpy(err, msg.data(), k);
    err[k] = '\0';
}

}  // namespace sship

namespace {

// The entry points of this file report every failed HIP call as SS_HIP_ERUNTIME, a failed allocation included ("The host
// boundary"): guarded() with that mapping.
template <typename F>
int guarded_rt(char* err, size_t errlen, const char* prefix, F&& body) { return guarded(err, errlen, prefix, body, SS_HIP_ERUNTIME); }

template <typename T>
Workspace<T>* ws_of(ss_hip_ctx* ctx) { return ctx->ws.as<Workspace<T>>(); }

// ---- re-layout: At[j][i] = src[i*rs + j*cs] for rows [r0, r0+R) --------------------
template <typename T>
__global__ __launch_bounds__(1024)
void k_relayout(const T* __restrict__ src, long long rs, long long cs, uint32_t R, uint32_t n,
                uint32_t r0, T* __restrict__ At, uint32_t ldm)
{
    __shared__ T tile[32][33];
    const uint32_t j0 = blockIdx.x * 32;
    const uint32_t tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (uint32_t i0 = blockIdx.y * 32; i0 < R; i0 += gridDim.y * 32) {   // uniform per block
        {
            const uint32_t i = i0 + ty, j = j0 + tx;
            tile[ty][tx] = (i < R && j < n) ? src[(long long)i * rs + (long long)j * cs] : T(0);
        }
        __syncthreads();
        {
            const uint32_t j = j0 + ty, i = i0 + tx;
            if (j < n && i < R) At[(size_t)j * ldm + r0 + i] = tile[tx][ty];
        }
        __syncthreads();
    }
}

template <typename T>
void upload_matrix(ss_hip_ctx* ctx, const T* A, ptrdiff_t rs, ptrdiff_t cs)
{
    const size_t m = ctx->m, n = ctx->n, s = sizeof(T);
    T* At = static_cast<T*>(ctx->At);
    const uint32_t ldm = ctx->ldm;
    if (on_device(A)) {
        // one generic strided transpose straight from the caller's device buffer
        const dim3 grid((unsigned)((n + 31) / 32), (unsigned)std::min<size_t>((m + 31) / 32, 32768));
        hipLaunchKernelGGL((k_relayout<T>), grid, dim3(1024), 0, ctx->stream, A, (long long)rs,
                           (long long)cs, (uint32_t)m, (uint32_t)n, 0u, At, ldm);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(ctx->stream));
        return;
    }

    if ((rs == 1 || m == 1) && (cs >= (ptrdiff_t)m || n == 1) && cs > 0) {
        // column-major host view: columns are already contiguous
        // (a single column has no meaningful column stride: any pitch >= the width will do)
        const size_t spitch = (n == 1) ? m * s : (size_t)cs * s;
        HIPCHK(hipMemcpy2D(At, (size_t)ldm * s, A, spitch, m * s, n, hipMemcpyHostToDevice));
        return;
    }

    // row panels through a staging buffer, transposed on the device
    const size_t panel_bytes = (size_t)256 << 20;
    size_t R = std::max<size_t>(1, std::min(m, panel_bytes / std::max<size_t>(1, n * s)));
    DeviceBuf stage_buf;
    stage_buf.alloc(R * n * s, "hipMalloc(&stage, R * n * s)");
    T* stage = stage_buf.get<T>();
    std::vector<T> gather;
    const bool rowmajor = (cs == 1 || n == 1) && (rs >= (ptrdiff_t)n || m == 1) && rs > 0;
    for (size_t r0 = 0; r0 < m; r0 += R) {
        const size_t rows = std::min(R, m - r0);
        if (rowmajor) {
            const size_t spitch = (m == 1) ? n * s : (size_t)rs * s;
            HIPCHK(hipMemcpy2D(stage, n * s, A + (ptrdiff_t)r0 * rs, spitch, n * s, rows, hipMemcpyHostToDevice));
        } else {
            // arbitrary (e.g. negative or doubly strided) host view: gather on the host
            gather.resize(rows * n);
            for (size_t i = 0; i < rows; ++i)
                for (size_t j = 0; j < n; ++j)
                    gather[i * n + j] = A[(ptrdiff_t)(r0 + i) * rs + (ptrdiff_t)j * cs];
            HIPCHK(hipMemcpy(stage, gather.data(), rows * n * s, hipMemcpyHostToDevice));
        }
        const dim3 grid((unsigned)((n + 31) / 32), (unsigned)std::min<size_t>((rows + 31) / 32, 32768));
        hipLaunchKernelGGL((k_relayout<T>), grid, dim3(1024), 0, ctx->stream, stage, (long long)n,
                           1LL, (uint32_t)rows, (uint32_t)n, (uint32_t)r0, At, ldm);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
}

// ---- compact output: one fixed-size record per signal, packed from the solver's own lists ----------
// Record layout (include/ss_hip.h): u32 K, u32 iter, f64 err, u32 idx[kmax], T val[kmax].
// The non-zero coefficients of x live on the columns of the slot's `touched` list (every column that was
// ever in the support: reference mode, where a leaving column may keep a rounding residue) or on its
// support list (zero_on_removal = 1: leaving columns carry exact zeros) — both sorted by column, so a
// stable compaction of the entries with x != 0 gives the record without scanning the n coefficients.

template <typename T>
__global__ __launch_bounds__(256)
void k_pack_records(const T* __restrict__ x, const uint32_t* __restrict__ gam2, const uint32_t* __restrict__ touched2,
                    const DevState* __restrict__ st, SlotDims L, int use_touched, uint32_t kmax,
                    unsigned char* __restrict__ rec, size_t rec_bytes)
{
    const size_t s = blockIdx.x;
    x += s * L.n_pad;
    st += s;
    const uint32_t cur = st->cur & 1u;
    const uint32_t* list = (use_touched ? touched2 : gam2) + s * 2 * (size_t)L.kcap + (size_t)cur * L.kcap;
    // (a solve that ended on an emptied support keeps the one column in its list: its x is handed back)
    uint32_t cnt = use_touched ? st->ntouched : st->K;
    if (cnt == 0u) cnt = 1u;
    if (cnt > L.kcap) cnt = L.kcap;
    // A slot that did not report (a form declined it: the one-workgroup kernels then leave K set and the lists unwritten) packs an
    // EMPTY record — whoever solves it again overwrites the record; its lists must not be walked (stale words as column indices)
    if (st->status != 0u) cnt = 0u;
    unsigned char* r = rec + s * rec_bytes;
    uint32_t* idx = reinterpret_cast<uint32_t*>(r + 16);
    T* val = reinterpret_cast<T*>(r + 16 + (size_t)kmax * 4);
    __shared__ uint32_t s_w[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t base = 0;
    for (uint32_t j0 = 0; j0 < cnt; j0 += 256u) {
        const uint32_t j = j0 + tid;
        uint32_t col = 0;
        T v = T(0);
        if (j < cnt) { col = list[j]; v = col < L.n_pad ? x[col] : T(0); }
        const bool nz = j < cnt && v != T(0);
        const uint64_t bal = __ballot(nz);
        __syncthreads();
        if (lane == 0) s_w[wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t w = 0; w < 4u; ++w) { if (w < wave) before += s_w[w]; total += s_w[w]; }
        const uint32_t pos = base + before + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
        if (nz && pos < kmax) { idx[pos] = col; val[pos] = v; }
        base += total;
    }
    for (uint32_t p = (base < kmax ? base : kmax) + tid; p < kmax; p += 256u) { idx[p] = 0u; val[p] = T(0); }
    for (size_t p = 16 + (size_t)kmax * (4 + sizeof(T)) + tid; p < rec_bytes; p += 256u) r[p] = 0;     // alignment padding
    if (tid == 0) {
        reinterpret_cast<uint32_t*>(r)[0] = base;
        reinterpret_cast<uint32_t*>(r)[1] = st->iter;
        *reinterpret_cast<double*>(r + 8) = st->c_inf;
    }
}

// ---- end of a solve in ONE launch: the device state to pinned (device-mapped) host memory and, when the caller's x
// ---- lives on the device, the n coefficients to it — instead of two or three copy commands with 10-20 us between them
template <typename T>
__global__ __launch_bounds__(256)
void k_epilogue(const uint32_t* __restrict__ st_words, uint32_t* __restrict__ hs_mapped, uint32_t st_nwords,
                const T* __restrict__ x_src, T* __restrict__ x_dst, long long incx, uint32_t n, uint32_t status_word, uint32_t flag_word)
{
    // status_word != 0xffffffff (the screened form of one signal): the verdict of its certificate — "a column was not certified"
    // (the word at flag_word, raised by the screening pass) makes a clean status kStatusSubsetFail — is applied to the copy the host
    // reads, instead of a launch of its own (k_sub_finish) before this one
    // (the caller's x receives the coefficients only of a path that was certified: an uncertified one is solved again by the engine
    // behind the form, and if THAT fails the caller must not be left holding uncertified numbers beside an error code)
    const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x, gsz = gridDim.x * blockDim.x;
    const bool withheld = status_word != 0xffffffffu && (st_words[status_word] != 0u || st_words[flag_word] != 0u);
    if (x_dst != nullptr && !withheld)
        for (uint32_t i = gtid; i < n; i += gsz) x_dst[(long long)i * incx] = x_src[i];
    if (blockIdx.x == 0)
        for (uint32_t i = threadIdx.x; i < st_nwords; i += blockDim.x) {
            uint32_t w = st_words[i];
            if (i == status_word && w == 0u && st_words[flag_word] != 0u) w = kStatusSubsetFail;
            __hip_atomic_store(&hs_mapped[i], w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
}

// everything but the trace buffer given back, every field as in a new workspace (the move assignment releases what `own` and `cache` held)
template <typename T>
void release_arrays(Workspace<T>* w)
{
    Workspace<T> fresh;
    fresh.trace_own = std::move(w->trace_own);
    fresh.trace = w->trace;
    fresh.trace_cap = w->trace_cap;
    *w = std::move(fresh);
}

// Makes sure the workspace holds `nslots` signals and an active set of `kcap` columns each.
// Everything is (re)allocated together; sizes only grow.
template <typename T>
void ensure_workspace(ss_hip_ctx* ctx, uint32_t nslots, uint32_t kcap)
{
    Workspace<T>* w = &part<Workspace<T>>(ctx->ws);
    if (nslots <= w->b_cap && kcap <= w->kcap) return;
    uint32_t want_k = std::max<uint32_t>(kcap, w->kcap);
    if (kcap > w->kcap)   // grow geometrically so slightly larger max_iter does not realloc
        want_k = std::max<uint32_t>(kcap, std::min<uint32_t>(kKcapLimit, std::max<uint32_t>(64, w->kcap * 2)));
    const uint32_t want_b = std::max<uint32_t>(nslots, w->b_cap);
    // one slot keeps the classic [2][ldm] / [2][n_pad] layout; batches are padded to whole
    // 128-row GEMM tiles
    const uint32_t b_pad = want_b == 1 ? 1u : (want_b + 127u) / 128u * 128u;
    release_arrays(w);
    const size_t ldm = ctx->ldm, np = ctx->n_pad, s = sizeof(T), B = want_b, K = want_k;
    SlotDims L{};
    L.n_pad = ctx->n_pad;
    L.ldm = ctx->ldm;
    L.m = (uint32_t)ctx->m;
    L.kcap = want_k;
    L.b_pad = b_pad;
    L.pmax_stride = kMaxSweepBlocks;
    L.pmin_stride = kMaxScanBlocks;
    HELD(w->own, hipMalloc, &w->y, B * ldm * s);
    HELD(w->own, hipMalloc, &w->rhs, 2 * (size_t)b_pad * ldm * s);
    HELD(w->own, hipMalloc, &w->cq, 2 * (size_t)b_pad * np * s);
    HELD(w->own, hipMalloc, &w->x, B * np * s);
    HELD(w->own, hipMalloc, &w->d, B * np * s);
    HELD(w->own, hipMalloc, &w->insup, B * np);
    HELD(w->own, hipMalloc, &w->pmax_val, B * L.pmax_stride * s);
    HELD(w->own, hipMalloc, &w->pmax_idx, B * L.pmax_stride * sizeof(uint32_t));
    HELD(w->own, hipMalloc, &w->pmin_val, B * L.pmin_stride * s);
    HELD(w->own, hipMalloc, &w->pmin_idx, B * L.pmin_stride * sizeof(uint32_t));
    HELD(w->own, hipMalloc, &w->gam, B * 2 * K * sizeof(uint32_t));
    HELD(w->own, hipMalloc, &w->touched, B * 2 * K * sizeof(uint32_t));
    HELD(w->own, hipMalloc, &w->inv[0], B * 2 * K * K * s);
    HELD(w->own, hipMalloc, &w->u1, B * K * s);
    HELD(w->own, hipMalloc, &w->u2, B * K * s);
    HELD(w->own, hipMalloc, &w->sgn, B * K * s);
    HELD(w->own, hipMalloc, &w->st, B * sizeof(DevState));
    HELD(w->own, hipMalloc, &w->ndone, 64);
    HELD(w->own, hipMalloc, &w->tile_skip, ((size_t)b_pad / 128 + 1) * sizeof(uint32_t));
    HIPCHK(hipMemsetAsync(w->tile_skip, 0, ((size_t)b_pad / 128 + 1) * sizeof(uint32_t), ctx->stream));
    w->inv[1] = w->inv[0] + K * K;
    w->c = w->cq;
    w->q = w->cq + (size_t)b_pad * np;
    w->b_cap = want_b;
    w->kcap = want_k;
    w->dims = L;
    HIPCHK(hipMemsetAsync(w->y, 0, B * ldm * s, ctx->stream));
    HIPCHK(hipMemsetAsync(w->rhs, 0, 2 * (size_t)b_pad * ldm * s, ctx->stream));
    HIPCHK(hipMemsetAsync(w->cq, 0, 2 * (size_t)b_pad * np * s, ctx->stream));
    HIPCHK(hipMemsetAsync(w->st, 0, B * sizeof(DevState), ctx->stream));
    HIPCHK(hipMemsetAsync(w->ndone, 0, 64, ctx->stream));
    // the support / touched lists start as "no column" (0xffffffff), not as whatever the allocation held: a reader that walks a list
    // nobody wrote (a slot a form declined) then meets an index every consumer bounds-checks — the same on every run, not a stale
    // word that happens to be a valid column in one process and an unmapped address in the next
    HIPCHK(hipMemsetAsync(w->gam, 0xff, B * 2 * K * sizeof(uint32_t), ctx->stream));
    HIPCHK(hipMemsetAsync(w->touched, 0xff, B * 2 * K * sizeof(uint32_t), ctx->stream));
}

}  // namespace

namespace sship {
int colshard_workspace(ss_hip_ctx* ctx, uint32_t kcap)
{
    try {
        if (ctx->is_f64) ensure_workspace<double>(ctx, 1, kcap);
        else ensure_workspace<float>(ctx, 1, kcap);
    } catch (const HipFail&) {
        (void)hipGetLastError();
        return SS_HIP_ENOMEM;
    } catch (const std::bad_alloc&) {
        return SS_HIP_ENOMEM;
    }
    return SS_HIP_OK;
}
}  // namespace sship

namespace {

template <typename T>
ss_hip_ctx* create_impl(const T* A, size_t m, size_t n, ptrdiff_t rs, ptrdiff_t cs, int device,
                        char* err, size_t errlen, int kind = 0)
{
    if (kind == 1 && m < n) {
        // irls-cpu.cpp / qr_decomposition.h:101 assert M >= N ("underdetermined systems not supported")
        set_err(err, errlen, "ss_hip_irls_create: IRLS needs a matrix with at least as many rows as columns");
        return nullptr;
    }
    if (!A || m == 0 || n == 0) {
        set_err(err, errlen, "ss_hip_homotopy_create: A must be a non-empty m x n matrix");
        return nullptr;
    }
    if (m > (size_t)1 << 28 || n > (size_t)1 << 30) {
        set_err(err, errlen, "ss_hip_homotopy_create: matrix dimensions too large");
        return nullptr;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        set_err(err, errlen, "ss_hip_homotopy_create: no HIP device available");
        return nullptr;
    }
    if (device < 0 || device >= ndev) {
        set_err(err, errlen, "ss_hip_homotopy_create: device index out of range");
        return nullptr;
    }
    ss_hip_ctx* ctx = new (std::nothrow) ss_hip_ctx();
    if (!ctx) {
        set_err(err, errlen, "ss_hip_homotopy_create: out of host memory");
        return nullptr;
    }
    try {
        HIPCHK(hipSetDevice(device));
        ctx->device = device;
        ctx->is_f64 = sizeof(T) == 8;
        ctx->m = m;
        ctx->n = n;
        ctx->ldm = (uint32_t)((m + kRowPad - 1) / kRowPad * kRowPad);
        ctx->n_pad = (uint32_t)((n + kColPad - 1) / kColPad * kColPad);
        hipDeviceProp_t prop;
        HIPCHK(hipGetDeviceProperties(&prop, device));
        ctx->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        HELD(ctx->own, hipStreamCreateWithFlags, &ctx->stream, hipStreamNonBlocking);
        const size_t bytes = (size_t)ctx->n_pad * ctx->ldm * sizeof(T);
        HELD(ctx->own, hipMalloc, &ctx->At, bytes);
        HIPCHK(hipMemsetAsync(ctx->At, 0, bytes, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        upload_matrix<T>(ctx, A, rs, cs);
        ctx->kind = kind;
        // (SS_HIP_SCREEN_SINGLE = 0 / 1 / 2: the initial value of option "screen_single" — the test suite pins the engines it
        // examines one by one with it; ss_hip_set_option overrides)
        if (const char* ev = std::getenv("SS_HIP_SCREEN_SINGLE")) ctx->screen_single = std::max(0, std::min(2, std::atoi(ev)));
        if (kind == 1) HIPCHK(irls_factor<T>(ctx));
        else ensure_workspace<T>(ctx, 1, 64);
        HELD(ctx->own, hipHostMalloc, &ctx->host_flags, 64 * sizeof(uint32_t), hipHostMallocMapped);
        std::memset(ctx->host_flags, 0, 64 * sizeof(uint32_t));
        HELD(ctx->own, hipHostMalloc, &ctx->hs_pinned, sizeof(DevState), hipHostMallocMapped);
        std::memset(ctx->hs_pinned, 0, sizeof(DevState));
        if (hipHostGetDevicePointer(&ctx->hs_mapped, ctx->hs_pinned, 0) != hipSuccess) { (void)hipGetLastError(); ctx->hs_mapped = nullptr; }
        HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void**>(&ctx->dev_flags), ctx->host_flags, 0));
        HELD(ctx->own, hipEventCreate, &ctx->ev_solve0);
        HELD(ctx->own, hipEventCreate, &ctx->ev_solve1);
        const uint64_t s = sizeof(T);
        ctx->stats.sweep_bytes = (uint64_t)m * n * s + 2 * (uint64_t)m * s + 2 * (uint64_t)n * s;
        ctx->stats.sweep1_bytes = (uint64_t)m * n * s + (uint64_t)m * s + (uint64_t)n * s;
        ctx->stats.sweep32_bytes = (uint64_t)m * n * s + 32 * (uint64_t)m * s + 32 * (uint64_t)n * s;
        ctx->stats.sweep32_timed_cols = n;
        ctx->stats.sweep64_bytes = (uint64_t)m * n * s + 64 * (uint64_t)m * s + 64 * (uint64_t)n * s;
        ctx->stats.sweep64_flops = 2ull * 64ull * (uint64_t)m * n;
    } catch (const HipFail& f) {
        set_err(err, errlen, hip_msg(f));
        ss_hip_homotopy_destroy(ctx);
        return nullptr;
    } catch (const std::bad_alloc&) {
        set_err(err, errlen, "ss_hip_homotopy_create: out of host memory");
        ss_hip_homotopy_destroy(ctx);
        return nullptr;
    }
    return ctx;
}

// ---- lookahead engine (fp32): Gram-column cache management and round launches -------------
bool ensure_full_gram(ss_hip_ctx* ctx);     // G = A^T A of the context (defined with the batched paths)
void gram_reserve_start(ss_hip_ctx* ctx, size_t B);

// the 32-RHS lookahead sweep of either precision, and the resident iteration kernel (fp32 only)
inline hipError_t launch_gemm32(const ss_hip_ctx* ctx, const uint32_t* rcols, const uint32_t* drows, float* D, uint32_t ldd, const DevState* st)
{ return launch_gemm32_tn_f32(ctx, rcols, drows, D, ldd, st); }
inline hipError_t launch_gemm32(const ss_hip_ctx* ctx, const uint32_t* rcols, const uint32_t* drows, double* D, uint32_t ldd, const DevState* st)
{ return launch_gemm32_tn_f64(ctx, rcols, drows, D, ldd, st); }
// (fp32 only — the speculative and the resident form are never chosen in double precision: an error there)
template <typename T>
hipError_t launch_persist(ss_hip_ctx* ctx, Workspace<T>& ws, T tol, uint32_t max_iter, uint32_t lds_cols, bool after_solo = false)
{
    if constexpr (sizeof(T) == 4) return launch_la_persist_f32(ctx, ws, tol, max_iter, lds_cols, after_solo);
    else return hipErrorInvalidConfiguration;
}
// speculative form: solo launch + verification + publication; seeding of the subset ranking
template <typename T>
hipError_t launch_solo_group(ss_hip_ctx* ctx, Workspace<T>& ws, T tol, uint32_t max_iter)
{
    if constexpr (sizeof(T) == 4) {
        const hipError_t e = launch_la_solo_f32(ctx, ws, tol, max_iter);
        return e != hipSuccess ? e : launch_la_verify_f32(ctx, ws);
    } else return hipErrorInvalidConfiguration;
}
template <typename T>
hipError_t launch_cand_init(ss_hip_ctx* ctx, Workspace<T>& ws)
{
    if constexpr (sizeof(T) == 4) return launch_la_cand_init_f32(ctx, ws);
    else return hipErrorInvalidConfiguration;
}
template <typename T>
hipError_t launch_top_cand(ss_hip_ctx* ctx, Workspace<T>& ws, uint32_t nsel = 32)
{
    if constexpr (sizeof(T) == 4) return launch_la_top_cand_f32(ctx, ws, nsel);
    else return hipErrorInvalidConfiguration;
}
// the first lookahead sweep of a fp32 solve may fetch 64 Gram columns in one (MFMA-bound) pass
inline hipError_t launch_gemm_first(const ss_hip_ctx* ctx, uint32_t nsel, const uint32_t* rcols, const uint32_t* drows, float* D, uint32_t ldd, const DevState* st)
{ return nsel > 32 ? launch_gemm64_tn_f32(ctx, rcols, drows, D, ldd, st) : launch_gemm32_tn_f32(ctx, rcols, drows, D, ldd, st); }
inline hipError_t launch_gemm_first(const ss_hip_ctx* ctx, uint32_t nsel, const uint32_t* rcols, const uint32_t* drows, double* D, uint32_t ldd, const DevState* st)
{ return nsel > 32 ? launch_gemm64_tn_f64(ctx, rcols, drows, D, ldd, st) : launch_gemm32_tn_f64(ctx, rcols, drows, D, ldd, st); }
// columns of a miss sweep: 32 in fp32 (HBM-bound); in double precision 64 (the pass is MFMA-bound either way), late ones 32
// (fetch = how many passes this solve has fetched after its first: in double precision the first two passes are wide;
// later misses come late on the path — at configs[4] the third pass serves the last ~8 of 128 iterations — and take 32)
inline uint32_t miss_cols(const ss_hip_ctx*, const Workspace<float>&, uint32_t = 0) { return 32u; }
inline uint32_t miss_cols(const ss_hip_ctx*, const Workspace<double>& ws, uint32_t fetch = 0)
{
    if (ws.gcap < 192) return 32u;
    return fetch >= 1 ? 32u : 64u;
}

// early form of the speculative engine (fp32): the first solo launch runs on the subset Gram matrix beside the passes over A
inline void early_prologue(ss_hip_ctx* ctx, Workspace<float>& ws, uint32_t nparts, float tol, uint32_t max_iter, uint32_t lds_cols,
                           EventPair pass1, EventPair pass2);
inline void early_prologue(ss_hip_ctx*, Workspace<double>&, uint32_t, double, uint32_t, uint32_t, EventPair, EventPair)
{ throw HipFail{ hipErrorInvalidConfiguration, "early_prologue<double>" }; }

template <typename T> struct Lookahead {
    static constexpr bool supported = true;

    static void ensure(ss_hip_ctx* ctx, Workspace<T>& ws, uint32_t kcap)
    {
        const uint32_t gpitch = (ctx->n_pad + 1023u) / 1024u * 1024u;
        // every sweep caches up to 32 columns; a solve needs at most one sweep per inserted column
        uint64_t want = 32ull * ((uint64_t)kcap + 2);
        // (the resident kernel addresses cache rows with 32-bit byte offsets: stay below 4 GiB)
        const uint64_t budget = std::min<uint64_t>((uint64_t)ctx->cache_mib << 20, (4095ull << 20));
        const uint64_t fit = std::max<uint64_t>(64, budget / ((uint64_t)gpitch * sizeof(T)));
        if (want > fit) want = fit;
        if (ws.gcache && ws.gcap >= want && ws.gpitch == gpitch) return;
        static_cast<LaCache<T>&>(ws) = LaCache<T>();      // (the old cache released, its fields as new)
        HELD(ws.cache, hipMalloc, &ws.gcache, (size_t)want * gpitch * sizeof(T));
        HELD(ws.cache, hipMalloc, &ws.slot_of, (size_t)ctx->n_pad * sizeof(int32_t));
        HELD(ws.cache, hipMalloc, &ws.c0, (size_t)ctx->n_pad * sizeof(T));
        HELD(ws.cache, hipMalloc, &ws.tcand, (size_t)ctx->n_pad * sizeof(T));
        HELD(ws.cache, hipMalloc, &ws.sw_list, 128 * sizeof(uint32_t));
        // (0xffffffff = "no column": k_subset_pick with a small subset writes only the entries it uses)
        HIPCHK(hipMemsetAsync(ws.sw_list, 0xff, 128 * sizeof(uint32_t), ctx->stream));
        if (sizeof(T) == 4) {
            // speculative form: slot -> column map, breakpoint log, verification partials, subset ranking
            ws.nvwg = (uint32_t)((ctx->n + kSoloWidth - 1) / kSoloWidth);
            HELD(ws.cache, hipMalloc, &ws.slot_col, (size_t)want * sizeof(uint32_t));
            HELD(ws.cache, hipMalloc, &ws.solo_log, ((size_t)kSoloHeaderWords + (size_t)kSoloLogCap * kSoloEntryWords) * sizeof(uint32_t));
            HELD(ws.cache, hipMalloc, &ws.solo_stage, (size_t)kSoloStageWords * sizeof(uint32_t));
            HELD(ws.cache, hipMalloc, &ws.sub_pos, (size_t)ctx->n_pad);
            HIPCHK(hipMemsetAsync(ws.sub_pos, 0, (size_t)ctx->n_pad, ctx->stream));
            HELD(ws.cache, hipMalloc, &ws.v_max, (size_t)kSoloLogCap * ws.nvwg * sizeof(uint32_t));
            HELD(ws.cache, hipMalloc, &ws.v_min, (size_t)kSoloLogCap * ws.nvwg * sizeof(uint64_t));
            HELD(ws.cache, hipMalloc, &ws.sw_list2, 128 * sizeof(uint32_t));
            HIPCHK(hipMemsetAsync(ws.sw_list2, 0xff, 128 * sizeof(uint32_t), ctx->stream));
            HELD(ws.cache, hipMalloc, &ws.sub_cols, 2 * (size_t)kSoloWidth * sizeof(uint32_t));     // columns, then the progress hints (float)
            HELD(ws.cache, hipMalloc, reinterpret_cast<void**>(&ws.subg), (size_t)kSoloWidth * kSoloWidth * sizeof(float));
            HELD(ws.cache, hipMalloc, &ws.cand_top, kCandPerBlock * (size_t)ws.nvwg * sizeof(uint64_t));
            HIPCHK(hipMemsetAsync(ws.cand_top, 0xff, kCandPerBlock * (size_t)ws.nvwg * sizeof(uint64_t), ctx->stream));
        }
        ws.gcap = (uint32_t)want;
        ws.gpitch = gpitch;
        // developer aid: SS_HIP_LA_DEBUG=<file> dumps the stage timestamps of k_la_iter after each solve
        if (!ws.la_dbg && std::getenv("SS_HIP_LA_DEBUG")) HELD(ws.own, hipMalloc, &ws.la_dbg, 2048 * 8 * sizeof(uint64_t));
        if (!ws.la_sync) HELD(ws.own, hipMalloc, &ws.la_sync, kLaSyncBytes);
        if (!ws.cq_alt) HELD(ws.own, hipMalloc, &ws.cq_alt, 2 * (size_t)ctx->n_pad * sizeof(T));
    }

    // the columns of a solve's first lookahead sweep (0: none — full-G mode, every column is "cached": no sweep, ever): the entering
    // column and the largest |c0| — 64 columns in one pass (fp32; MFMA-bound, ~0.45 ms at C2) instead of two 32-column passes and a
    // round trip through the host in between
    static uint32_t first_cols(const ss_hip_ctx* ctx, const Workspace<T>& ws)
    {
        if (ws.gram_is_full) return 0;
        if (sizeof(T) == 8) return miss_cols(ctx, ws);
        return (ctx->first_sweep_cols > 32 && ctx->sweep32_variant == 0 && ws.gcap >= 128) ? 64u : 32u;
    }

    // c0 = A^T y has been swept into ws.c0 (partials in pmax): first pick, first lookahead sweep (ev: events around it)
    static void init(ss_hip_ctx* ctx, Workspace<T>& ws, uint32_t nparts, T tol, bool solo = false, EventPair ev = {})
    {
        hipStream_t st = ctx->stream;
        const uint32_t nsel = first_cols(ctx, ws);
        const bool full = nsel == 0;
        // (the slot map, the hand-off area of the resident kernel and the dense vectors were cleared by
        // k_la_reset before the sweep; the first sign is read from c0 itself)
        if (ws.la_dbg) HIPCHK(hipMemsetAsync(ws.la_dbg, 0, 2048 * 8 * sizeof(uint64_t), st));
        HIPCHK(launch_la_init_pick<T>(ctx, ws, nparts, tol, full));
        if (solo) HIPCHK(launch_cand_init(ctx, ws));           // per-block tops of |c0|: ranking of the first sweep and subset
        if (!full) {
            if (solo && ctx->n > 32u * 512u) HIPCHK(launch_top_cand(ctx, ws, nsel));
            else HIPCHK(launch_la_top<T>(ctx, ws, 1, nsel));
            if (ev.a) HIPCHK(hipEventRecord(ev.a, ctx->stream));
            HIPCHK(launch_gemm_first(ctx, nsel, ws.sw_list, ws.sw_list + 64, ws.gcache, ws.gpitch, ws.st));
            if (ev.b) HIPCHK(hipEventRecord(ev.b, ctx->stream));
        }
        HIPCHK(launch_la_update<T>(ctx, ws, 0, tol));
        if (ctx->la_fused) return;      // k_la_iter forms c and q itself
        uint32_t np2 = 0;
        HIPCHK(launch_la_cq<T>(ctx, ws, &np2));
        ws.la_nparts = np2;
    }

    // fused form: one launch per iteration ...
    // lds_cols != 0: resident form holding up to that many support columns in LDS
    // solo: the speculative form (one workgroup + verification) while the device has not switched it off
    static void iterate(ss_hip_ctx* ctx, Workspace<T>& ws, T tol, uint32_t max_iter, uint32_t lds_cols, bool solo = false)
    {
        if (solo) HIPCHK(launch_solo_group(ctx, ws, tol, max_iter));
        else if (lds_cols != 0) HIPCHK(launch_persist(ctx, ws, tol, max_iter, lds_cols));
        else HIPCHK(launch_la_iter<T>(ctx, ws, tol, max_iter));
    }
    // ... and, when the device reports an entering column without cached Gram column, the sweep
    // that fetches it (plus 31 likely successors) and the inverse update that was waiting for it
    // from_cand: the speculative form is running — its verification has left the per-block candidate tops of
    // the scan that missed (wide dictionaries only: with few blocks the tops are too few to rank from)
    static void fetch(ss_hip_ctx* ctx, Workspace<T>& ws, T tol, EventPair ev = {}, bool from_cand = false, uint32_t fetch_index = 0)
    {
        const uint32_t nsel = miss_cols(ctx, ws, fetch_index);
        if (from_cand && ctx->n > 32u * 512u) HIPCHK(launch_top_cand(ctx, ws));
        else HIPCHK(launch_la_top<T>(ctx, ws, 0, nsel));
        if (ev.a) HIPCHK(hipEventRecord(ev.a, ctx->stream));
        HIPCHK(launch_gemm_first(ctx, nsel, ws.sw_list, ws.sw_list + 64, ws.gcache, ws.gpitch, ws.st));
        if (ev.b) HIPCHK(hipEventRecord(ev.b, ctx->stream));
        HIPCHK(launch_la_update<T>(ctx, ws, 1, tol));
    }
    // OMP: the next picks are the largest correlations; the pending update is k_gramupd in OMP mode
    static void fetch_omp(ss_hip_ctx* ctx, Workspace<T>& ws, T tol, EventPair ev = {})
    {
        const uint32_t nsel = miss_cols(ctx, ws);
        HIPCHK(launch_la_top<T>(ctx, ws, 2, nsel));
        if (ev.a) HIPCHK(hipEventRecord(ev.a, ctx->stream));
        HIPCHK(launch_gemm_first(ctx, nsel, ws.sw_list, ws.sw_list + 64, ws.gcache, ws.gpitch, ws.st));
        if (ev.b) HIPCHK(hipEventRecord(ev.b, ctx->stream));
        HIPCHK(launch_la_omp_update<T>(ctx, ws, tol));
    }

    // one homotopy iteration: scan + select, (sweep if the entering column is not cached),
    // inverse update + direction from the cache, Gram-form c and q
    static void round(ss_hip_ctx* ctx, Workspace<T>& ws, uint32_t rnd, T tol, uint32_t max_iter, EventPair ev = {})
    {
        HIPCHK(launch_la_scansel<T>(ctx, ws, rnd, ws.la_nparts, tol, max_iter));
        const uint32_t nsel = miss_cols(ctx, ws);
        HIPCHK(launch_la_top<T>(ctx, ws, 0, nsel));
        if (ev.a) HIPCHK(hipEventRecord(ev.a, ctx->stream));
        HIPCHK(launch_gemm_first(ctx, nsel, ws.sw_list, ws.sw_list + 64, ws.gcache, ws.gpitch, ws.st));
        if (ev.b) HIPCHK(hipEventRecord(ev.b, ctx->stream));
        HIPCHK(launch_la_update<T>(ctx, ws, rnd, tol));
        uint32_t np2 = 0;
        HIPCHK(launch_la_cq<T>(ctx, ws, &np2));
        ws.la_nparts = np2;
    }
};

// ---- early form (fp32, option early_solo): everything of a typical solve in ONE enqueue ---------------------------------
// After c0 = A^T y the columns that matter are ranked once (|c0| tops).  The best 256 become the subset of the
// first solo launch, whose Gram values all come from Gs = A_S^T A_S (subgram.hip: bit for bit the sweep's values,
// 8 MiB of A instead of two passes over it); the best 64 get cache slots and their full Gram columns are swept on a
// SECOND stream while the solo workgroup iterates (the barrier-free pass: 2048 single-wave workgroups that share
// the chip with it; a gate kernel holds them back until the solo workgroup is resident).  Afterwards, on the main
// stream again: slots + up to two passes for the columns the launch used beyond those 64, then the verification of
// every breakpoint over all n columns (from the swept rows, exactly as in the plain form), the commit, and the
// resident form for the last step of the path.  A solve that does not fit this mould (a pick outside the subset,
// a miss, a failed check) simply continues in the plain pump below.
inline void early_prologue(ss_hip_ctx* ctx, Workspace<float>& ws, uint32_t nparts, float tol, uint32_t max_iter, uint32_t lds_cols,
                           EventPair pass1, EventPair pass2)
{
    hipStream_t st = ctx->stream;
    if (!ctx->stream2) {
        // A stream of another priority class: HIP keeps a pool of hardware queues per class, so this one never
        // shares a queue with the main stream (two streams on ONE hardware queue execute in submission order, and
        // the gate kernel below would then sit in front of the very launch it waits for).
        int lo = 0, hi = 0;
        if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) { (void)hipGetLastError(); lo = hi = 0; }
        Holdings& own = ctx->own;
        if (own.stream(&ctx->stream2, hipStreamNonBlocking, hi) != hipSuccess) HELD(own, hipStreamCreateWithFlags, &ctx->stream2, hipStreamNonBlocking);
        HELD(own, hipEventCreateWithFlags, &ctx->ev_fork, hipEventDisableTiming);
        HELD(own, hipEventCreateWithFlags, &ctx->ev_join, hipEventDisableTiming);
        // a third stream (lowest priority class: again its own hardware queue) for the tiles dealt out by shader engine
        if (own.stream(&ctx->stream3, hipStreamNonBlocking, lo) == hipSuccess) {
            HELD(own, hipEventCreateWithFlags, &ctx->ev_gate, hipEventDisableTiming);
            HELD(own, hipEventCreateWithFlags, &ctx->ev_b0, hipEventDisableTiming);
            HELD(own, hipEventCreateWithFlags, &ctx->ev_join3, hipEventDisableTiming);
            HELD(own, hipMalloc, &ctx->se_count, 2 * (kSeCount + 2) * sizeof(uint32_t));
            if (own.stream(&ctx->stream4, hipStreamNonBlocking, lo) == hipSuccess) HELD(own, hipEventCreateWithFlags, &ctx->ev_join4, hipEventDisableTiming);
        }
    }
    // Dealing the passes out around the solo workgroup (option early_se).  The hardware distributes a grid statically:
    // every shader engine of every XCD gets the same number of workgroups, whatever its CUs hold (per-workgroup trace of
    // the real pass, tools/probe_pass_trace.py).  The solo workgroup owns one CU of one SE; 512 tiles put 16 on the 7
    // other CUs of that SE, two of them run a third tile, and a pass — bound by what ONE CU can load — ends at 0.49 ms
    // instead of 0.37.  So: the main launch takes 14 tiles per SE (two per CU on the solo SE, room for exactly two
    // workgroups per CU: LDS padding), a second launch on a third stream puts two more workgroups on every SE, which
    // pick their tile by where they run and leave at once on the solo workgroup's SE (k_gemm32_tn_f32<BYSE>), and the
    // two tiles that are left of 512 are formed by the VALU chain (k_cols_gram) on a fourth stream.  Every CU but one
    // then carries exactly two tiles.
    uint32_t main_tiles = 0, se_last = 0, tail_c0 = 0, tail_cols = 0, se_quota = 2u, range_last = 0;
    if (ctx->early_se && ctx->early_pass == 2 && ctx->stream3 && ctx->num_cus == 8 * (int)kSeCount &&
        ctx->n_pad % 128 == 0 && ctx->ldm % 256 == 0) {
        const uint32_t nt = (uint32_t)(ctx->n_pad / 128);
        if (nt > 14u * kSeCount && nt <= 16u * kSeCount) {
            main_tiles = 14u * kSeCount;                                        // 448
            se_last = std::min<uint32_t>(nt, main_tiles + 2u * (kSeCount - 1u)); // tiles [448, 510) by shader engine
            tail_c0 = se_last * 128u;
            tail_cols = (nt - se_last) * 128u;                                  // the last 256 columns at 8192 x 65536
        } else if (nt > 16u * kSeCount && ctx->early_se == 3) {
            // Wider dictionaries, opt-in (early_se = 3; measured no faster than one launch per pass: 2.43 against 2.21 ms per
            // solve at 98304 columns, 2.79 against 2.78 at 131072 — with three or more tiles per CU the launch evens itself
            // out as workgroups finish; the cliff round 2 saw beyond 65536 columns was the candidate ranking, solo.hip:
            // rank_offers): a pass is bound by what ONE CU can load, so its time is the largest number of
            // tiles any CU gets — u = nt / 255 per CU when the 255 CUs beside the solo workgroup share evenly: the main
            // launch takes 7 u tiles per shader engine (u per CU on the solo workgroup's SE, which has 7), the workgroups
            // dealt out by shader engine come back until their SE has had u more (u per CU there too), and the remainder
            // (< 255 tiles) runs as a partial round behind the main launch — or, when it is at most 16 tiles, on the VALU
            // chain beside the pass like the two left-over tiles at 65536 columns.
            const uint32_t per = 8u * kSeCount - 1u;                            // 255 CUs take tiles
            const uint32_t u = nt / per;
            main_tiles = 7u * kSeCount * u;
            se_quota = u;
            se_last = main_tiles + (kSeCount - 1u) * u;                          // = 255 u
            const uint32_t rest = nt - se_last;
            if (rest <= 16u) { tail_c0 = se_last * 128u; tail_cols = rest * 128u; }
            else range_last = nt;
        }
    }
    ctx->stats.sweep32_timed_cols = main_tiles ? (uint64_t)main_tiles * 128u : (uint64_t)ctx->n;   // (of THIS form's timed launch: kind 5 below)
    if (ws.la_dbg) HIPCHK(hipMemsetAsync(ws.la_dbg, 0, 2048 * 8 * sizeof(uint64_t), st));
    HIPCHK(launch_la_init_pick<float>(ctx, ws, nparts, tol, false));
    HIPCHK(launch_la_cand_init_f32(ctx, ws));
    HIPCHK(launch_subset_pick_f32(ctx, ws));                        // subset of 256, slots 0..63, the two sweep lists
    // Gs, and a_idx . a_idx seeded into the first pick's cache row for the first inverse update
    HIPCHK(launch_subset_gram_f32(ctx, ws.sub_cols, ws.subg, ws.st, ws.gcache, ws.slot_of, ws.gpitch));
    // (the counters of the dealing-out were zeroed by k_subset_pick)
    HIPCHK(hipEventRecord(ctx->ev_fork, st));
    // main stream: first inverse + direction (k_gramupd, round 0: reads only the seeded entry), then the solo launch
    HIPCHK(launch_la_update<float>(ctx, ws, 0, tol));
    HIPCHK(launch_la_solo_f32(ctx, ws, tol, max_iter));
    // second stream: the two 32-column passes, held back until the solo workgroup is resident.  (Enqueued AFTER the
    // solo launch: should the two streams ever share a hardware queue after all, the gate then follows the launch it
    // waits for and everything merely runs one after the other.)
    HIPCHK(hipStreamWaitEvent(ctx->stream2, ctx->ev_fork, 0));
    HIPCHK(launch_wait_started(ctx, ws, ctx->stream2));
    if (main_tiles) {
        // third stream: the tiles dealt out by shader engine.  Its workgroups must hold their CUs BEFORE the main launch
        // of the pass arrives (a workgroup that finds its SE full holds up every workgroup behind it in its grid; the
        // two that land on the solo workgroup's SE leave at once when they get there first): the main launch waits for
        // their arrival count
        HIPCHK(hipEventRecord(ctx->ev_gate, ctx->stream2));                     // (behind the gate: the solo workgroup is resident)
        HIPCHK(hipStreamWaitEvent(ctx->stream3, ctx->ev_gate, 0));
        HIPCHK(launch_gemm32se_on(ctx, ctx->stream3, ws.sw_list, ws.sw_list + 64, ws.gcache, ws.gpitch, main_tiles, se_last, ws.st,
                                  ctx->se_count, se_quota));
        HIPCHK(launch_wait_count(ctx->stream2, ctx->se_count + kSeCount, early_se_wgs(ctx), ws.st));
    }
    if (pass1.a) HIPCHK(hipEventRecord(pass1.a, ctx->stream2));
    HIPCHK(launch_gemm32w_on(ctx, ctx->stream2, ws.sw_list, ws.sw_list + 64, ws.gcache, ws.gpitch, main_tiles));
    if (pass1.b) HIPCHK(hipEventRecord(pass1.b, ctx->stream2));
    if (range_last) HIPCHK(launch_gemm32range_on(ctx, ctx->stream2, ws.sw_list, ws.sw_list + 64, ws.gcache, ws.gpitch, se_last, range_last));
    // the second pass's 32 columns are chosen now, half a millisecond into the solo launch: what has entered
    // its support without a Gram row so far, then the columns closest to entering (k_pick_pass_b)
    HIPCHK(launch_pick_pass_b_f32(ctx, ws, ctx->stream2));
    if (main_tiles) {
        HIPCHK(hipEventRecord(ctx->ev_b0, ctx->stream2));                       // (the second list exists, the first pass is complete)
        HIPCHK(hipStreamWaitEvent(ctx->stream3, ctx->ev_b0, 0));
        HIPCHK(launch_gemm32se_on(ctx, ctx->stream3, ws.sw_list + 32, ws.sw_list + 96, ws.gcache, ws.gpitch, main_tiles, se_last, ws.st,
                                  ctx->se_count + (kSeCount + 2), se_quota));
        HIPCHK(hipEventRecord(ctx->ev_join3, ctx->stream3));
        HIPCHK(launch_wait_count(ctx->stream2, ctx->se_count + (kSeCount + 2) + kSeCount, early_se_wgs(ctx), ws.st));
    }
    if (pass2.a) HIPCHK(hipEventRecord(pass2.a, ctx->stream2));
    HIPCHK(launch_gemm32w_on(ctx, ctx->stream2, ws.sw_list + 32, ws.sw_list + 96, ws.gcache, ws.gpitch, main_tiles));
    if (pass2.b) HIPCHK(hipEventRecord(pass2.b, ctx->stream2));
    if (range_last) HIPCHK(launch_gemm32range_on(ctx, ctx->stream2, ws.sw_list + 32, ws.sw_list + 96, ws.gcache, ws.gpitch, se_last, range_last));
    if (main_tiles) HIPCHK(hipStreamWaitEvent(ctx->stream2, ctx->ev_join3, 0));
    HIPCHK(hipEventRecord(ctx->ev_join, ctx->stream2));
    if (tail_cols) {
        // the last columns of both passes by the VALU chain (32 small workgroups each, ~70 us): on a fourth stream beside the
        // passes when there is one, else on this stream behind the solo launch
        hipStream_t ts = ctx->stream4 ? ctx->stream4 : st;
        if (ctx->stream4) HIPCHK(hipStreamWaitEvent(ts, ctx->ev_gate, 0));
        else HIPCHK(hipStreamWaitEvent(ts, ctx->ev_b0, 0));
        HIPCHK(launch_cols_gram_on(ctx, ts, tail_c0, tail_cols, ws.sw_list, ws.sw_list + 64, ws.gcache, ws.gpitch));
        if (ctx->stream4) HIPCHK(hipStreamWaitEvent(ts, ctx->ev_b0, 0));
        HIPCHK(launch_cols_gram_on(ctx, ts, tail_c0, tail_cols, ws.sw_list + 32, ws.sw_list + 96, ws.gcache, ws.gpitch));
        if (ctx->stream4) {
            HIPCHK(hipEventRecord(ctx->ev_join4, ts));
            HIPCHK(hipStreamWaitEvent(st, ctx->ev_join4, 0));
        }
    }
    // ... which the passes have to be complete for from here on
    HIPCHK(hipStreamWaitEvent(st, ctx->ev_join, 0));
    HIPCHK(launch_missing_cols_f32(ctx, ws));
    HIPCHK(launch_gemm32_tn_f32(ctx, ws.sw_list2, ws.sw_list2 + 64, ws.gcache, ws.gpitch, nullptr));
    HIPCHK(launch_gemm32_tn_f32(ctx, ws.sw_list2 + 32, ws.sw_list2 + 96, ws.gcache, ws.gpitch, nullptr));
    HIPCHK(launch_la_verify_f32(ctx, ws));                          // verification + publication
    if (lds_cols != 0) HIPCHK(launch_la_persist_f32(ctx, ws, tol, max_iter, lds_cols, true));
}

// copies a strided vector (host or device) into a contiguous device buffer
template <typename T>
void copy_in(ss_hip_ctx* ctx, T* dst_dev, const T* src, ptrdiff_t inc, size_t len)
{
    if (inc == 1) {
        HIPCHK(hipMemcpyAsync(dst_dev, src, len * sizeof(T), hipMemcpyDefault, ctx->stream));
    } else {
        HIPCHK(hipMemcpy2DAsync(dst_dev, sizeof(T), src, (size_t)inc * sizeof(T), sizeof(T), len,
                                hipMemcpyDefault, ctx->stream));
    }
}

template <typename T>
void copy_out(ss_hip_ctx* ctx, T* dst, ptrdiff_t inc, const T* src_dev, size_t len)
{
    if (inc == 1) {
        HIPCHK(hipMemcpyAsync(dst, src_dev, len * sizeof(T), hipMemcpyDefault, ctx->stream));
    } else {
        HIPCHK(hipMemcpy2DAsync(dst, (size_t)inc * sizeof(T), src_dev, sizeof(T), sizeof(T), len,
                                hipMemcpyDefault, ctx->stream));
    }
}

hipEvent_t prof_event(ss_hip_ctx* ctx, size_t i)
{
    while (ctx->prof_events.size() <= i) {
        hipEvent_t e;
        HELD(ctx->own, hipEventCreate, &e);
        ctx->prof_events.push_back(e);
    }
    return ctx->prof_events[i];
}

// Grow-only device buffer of `own`: `have` and `need` count units of `unit_bytes`.  A buffer that is too small is given back and taken
// anew (its contents are not kept); pointer and size are left null / 0 when the new allocation fails.  try_grow_device returns the
// allocation's error instead of throwing it (a failed release throws in both).
template <typename P, typename N>
hipError_t try_grow_device(Holdings& own, P*& ptr, N& have, size_t need, size_t unit_bytes)
{
    if (have >= need) return hipSuccess;
    HIPCHK(own.drop(ptr));
    have = 0;
    const hipError_t e = own.device(&ptr, need * unit_bytes);
    if (e == hipSuccess) have = (N)need;
    return e;
}
template <typename P, typename N>
void grow_device(Holdings& own, P*& ptr, N& have, size_t need, size_t unit_bytes, const char* what)
{
    held(try_grow_device(own, ptr, have, need, unit_bytes), what);
}

// The trace buffer for the extent of a solve or a chunk: room for `want` entries, or — want = 0 — hidden from the kernels, which
// then skip their stores.  The workspace gets its pointer back when the window goes out of scope.
template <typename T>
struct TraceWindow {
    Workspace<T>& ws;
    TraceEntry* keep;
    TraceWindow(Workspace<T>& w, uint32_t want) : ws(w)
    {
        grow_device(ws.trace_own, ws.trace, ws.trace_cap, want, sizeof(TraceEntry), "hipMalloc(trace)");
        keep = ws.trace;
        if (want == 0u) ws.trace = nullptr;
    }
    ~TraceWindow() { ws.trace = keep; }
    TraceWindow(const TraceWindow&) = delete;
    TraceWindow& operator=(const TraceWindow&) = delete;
};

// the traced path of a solve that took `iter` iterations into ctx->last_trace (entry 0 = the initial pick, entry t = the toggle of iteration t)
template <typename T>
void fetch_trace(ss_hip_ctx* ctx, Workspace<T>& ws, uint32_t iter)
{
    const size_t cnt = std::min<size_t>((size_t)iter + 1, ws.trace_cap);
    ctx->last_trace.resize(cnt);
    HIPCHK(hipMemcpy(ctx->last_trace.data(), ws.trace, cnt * sizeof(TraceEntry), hipMemcpyDeviceToHost));
}

// The lookahead wait of the round loops: round `round` is queued once the device has reached round - L (host_flags[0]) or the
// stream has drained.  false: the device raised `done` (host_flags[1]) — leave the loop.
inline bool wait_round(ss_hip_ctx* ctx, uint64_t round, uint32_t L, const char* what)
{
    if (round <= L) return true;
    volatile uint32_t* hf = ctx->host_flags;
    const uint32_t need = (uint32_t)(round - L);
    uint32_t spins = 0;
    while (hf[1] == 0 && hf[0] < need) {
        if ((++spins & 0x3ffu) == 0) {
            const hipError_t q = hipStreamQuery(ctx->stream);
            if (q == hipSuccess) break;               // queue drained
            if (q != hipErrorNotReady) throw HipFail{ q, what };
        }
        std::this_thread::yield();
    }
    return hf[1] == 0;
}

// compact output: pack the records of `nslots` finished slots into the context's staging buffer (device)
template <typename T>
unsigned char* pack_records(ss_hip_ctx* ctx, Workspace<T>& ws, uint32_t nslots, uint32_t kmax)
{
    const size_t rb = record_bytes(kmax, sizeof(T));
    grow_device(ctx->own, ctx->rec_stage, ctx->rec_stage_bytes, rb * nslots, 1, "hipMalloc(rec_stage)");
    hipLaunchKernelGGL((k_pack_records<T>), dim3(nslots), dim3(256), 0, ctx->stream, (const T*)ws.x, (const uint32_t*)ws.gam,
                       (const uint32_t*)ws.touched, (const DevState*)ws.st, ws.dims, ctx->zero_on_removal ? 0 : 1, kmax,
                       ctx->rec_stage, rb);
    HIPCHK(hipGetLastError());
    return ctx->rec_stage;
}

// The profiling events of one solve: pairs handed out in call order, each with what it brackets (account_profile books them).
// A solve that is not profiled gets null pairs, and nothing is recorded.
struct ProfSpans {
    ss_hip_ctx* ctx;
    bool on;
    ProfSpans(ss_hip_ctx* c, bool profiled) : ctx(c), on(profiled) { ctx->prof_spans.clear(); }
    EventPair span(ProfKind kind, uint32_t round = 0)
    {
        if (!on) return {};
        const size_t i = ctx->prof_spans.size();
        ctx->prof_spans.push_back({ kind, round });
        return { prof_event(ctx, 2 * i), prof_event(ctx, 2 * i + 1) };
    }
};
inline void record(hipEvent_t e, hipStream_t st) { if (e) HIPCHK(hipEventRecord(e, st)); }

// c0 = A^T y (residual_vector with x = 0, homotopy-cpu.cpp:215) into `out` — ws.c0 for the forms on the Gram cache, ws.c for the
// residual form —, the partial maxima in ws.pmax_* (*nparts of them); timed as the solve's first sweep
template <typename T>
void first_sweep(ss_hip_ctx* ctx, Workspace<T>& ws, T* out, ProfSpans& spans, uint32_t* nparts)
{
    const EventPair ev = spans.span(ProfKind::FirstSweep);
    record(ev.a, ctx->stream);
    HIPCHK(launch_sweep<T>(ctx, ws.rhs, (size_t)ws.dims.b_pad * ctx->ldm, 1, out, nullptr, ws.pmax_val, ws.pmax_idx, nparts, ws.st));
    record(ev.b, ctx->stream);
}

// one signal in the screened form (screen.hip): no G — the subset's own Gram matrix from A, then one pass over the fp16 copy of A
// (developer switch, read per solve: which hand-offs inside launches the form may use — 1 = the one-launch tail, 2 = the selection by
// many workgroups, 4 = k_la_reset's clears in the prologue of the fp8 ranking pass; unset = all, 0 = the launches before them)
inline void scr_handoff_mask(ScrHandoff* ho)
{
    if (const char* e = std::getenv("SS_HIP_SCR_HANDOFF")) ho->mask = (uint32_t)std::strtoul(e, nullptr, 0);
}

inline hipError_t scr_single(ss_hip_ctx* ctx, Workspace<float>& ws, float tol, uint32_t max_iter, bool first16, EventPair first, EventPair screen, EventPair path,
                             bool omp, bool rescue, ScrHandoff* ho)
{
    grow_device(ctx->own, ctx->sub_buf, ctx->sub_buf_bytes, sub_buffer_bytes(1), 1, "hipMalloc(sub_buf)");
    if (ctx->sub_dbg == nullptr && std::getenv("SS_HIP_SUB_STAMPS")) {
        HELD(ctx->own, hipMalloc, &ctx->sub_dbg, 16 * sizeof(unsigned long long));
        HIPCHK(hipMemsetAsync(ctx->sub_dbg, 0, 16 * sizeof(unsigned long long), ctx->stream));
    }
    // (with the state mirrored to mapped host memory the epilogue launch applies the certificate's verdict: no k_sub_finish)
    return launch_screen_form(ctx, ws, tol, max_iter, first16, ctx->hs_mapped == nullptr, first, screen, path, omp, rescue, ho);
}

// why a subset / screened solve was not reported: DevState::sub_reason's bits into the statistics
inline void count_reasons(ss_hip_ctx* ctx, uint32_t r, bool tie)
{
    ss_hip_stats& S = ctx->stats;
    if (r & kReasonRemoval) S.why_removal += 1;
    if (r & kReasonPositions) S.why_positions += 1;
    if (r & kReasonLog) S.why_breakpoints += 1;
    if (r & kReasonGuard) S.why_guard += 1;
    if (r & kReasonNoCand) S.why_no_candidate += 1;
    if (r & kReasonFirstState) S.why_first_state += 1;
    if (r & kReasonIrregular) S.why_irregular += 1;
    if (r & kReasonOverflow) S.why_overflow += 1;
    if (r & kReasonColumn) S.why_column += 1;
    if (tie || (r & kReasonTie)) S.why_tie += 1;
}

// ---- the host side of a solve in the launch-chain engines ---------------------------------------------------------------------
// The device decides termination (k_scansel / k_la_iter raise DevState::done and mirror it, with the round reached, into pinned host
// memory).  The host keeps at most `lookahead` launches queued beyond the device's position and stops enqueueing as soon as it
// sees `done`; launches already queued behind it are no-ops.
struct PumpState {
    bool solo = false;            // speculative launches still in use (the device may hand over to the resident form)
    bool solo_started = false;
    bool early = false;           // early form: a solo group (and the resident launch behind it) is queued already
    uint32_t early_lds_cols = 0;
    uint32_t ro_parts = 0;        // reference-order engine: partial maxima of its first sweep
    bool enqueued = false;        // the pump queued work behind a speculative epilogue
};

// Fused lookahead engine: every launch of k_la_iter performs the next iteration, or nothing while the device waits for a Gram
// column (host_flags[2] counts those waits).  Returns false if the loop made no progress (internal error).
template <typename T>
bool pump_fused(ss_hip_ctx* ctx, Workspace<T>& ws, T tol, uint32_t max_iter, bool la, bool la_omp, ProfSpans& spans, PumpState& ps)
{
    hipStream_t st = ctx->stream;
    const uint32_t L = (uint32_t)std::max(1, std::min(ctx->lookahead, 64));
    volatile uint32_t* hf = ctx->host_flags;
    // Fused lookahead engine: every launch of k_la_iter performs the next iteration, or
    // nothing while the device waits for a Gram column (hf[2] counts those waits).  The
    // host keeps L launches queued ahead and answers each wait with one fetch.
    uint64_t enq = ps.early ? (ps.early_lds_cols != 0 ? 2u : 1u) : 0u;   // (early form: a solo group and the resident launch behind it are queued)
    uint32_t handled = 0, timed_fetches = 0;
    // resident kernel: LDS tier (support columns it can hold); 0 = one launch per iteration
    uint32_t lds_cols = 0;
    const uint32_t kcap_ws = ws.dims.kcap;       // what the device checks K against (>= this solve's kcap)
    if (la && ctx->la_fused >= 2 && sizeof(T) == 4) {
        lds_cols = std::min<uint32_t>((kcap_ws + 15u) & ~15u, kLaLdsSmall);
        if (!la_persist_usable(ctx, lds_cols)) lds_cols = 0;
    }
    const uint64_t max_launch = 4 * ((uint64_t)max_iter + 2) + 64;
    bool stuck = false;
    for (;;) {
        uint32_t spins = 0;
        // (a solo group runs until the host has to act — fetch, hand-over, end — so one group in
        // flight is enough: every further one is three launches that find nothing to do; after
        // the hand-over, near the end of the path, two resident launches)
        const uint32_t depth = ps.solo ? 1u : (ps.solo_started ? std::min<uint32_t>(L, 2u) : L);
        while (hf[1] == 0 && hf[2] == handled && enq >= (uint64_t)hf[0] + depth) {
            if ((++spins & 0x3ffu) == 0) {
                const hipError_t qs = hipStreamQuery(st);
                if (qs == hipSuccess) break;
                if (qs != hipErrorNotReady) throw HipFail{ qs, "hipStreamQuery(solve loop)" };
            }
            std::this_thread::yield();
        }
        if (hf[1] != 0) break;
        ps.enqueued = true;
        if (hf[2] != handled) {
            const bool timed_la = spans.on && (timed_fetches++ % (uint32_t)std::max(1, ctx->profile_every) == 0);
            const EventPair ev = timed_la ? spans.span(ProfKind::Sweep32) : EventPair{};
            if (la_omp) Lookahead<T>::fetch_omp(ctx, ws, tol, ev);
            else Lookahead<T>::fetch(ctx, ws, tol, ev, ps.solo, handled);
            ++handled;
        }
        if (lds_cols != 0 && hf[3] > lds_cols) {
            // the support outgrew the tier: take the large one, or go on one launch per iteration
            const uint32_t big = std::min<uint32_t>((kcap_ws + 15u) & ~15u, kLaLdsLarge);
            lds_cols = (hf[3] <= big && big > lds_cols && la_persist_usable(ctx, big)) ? big : 0u;
        }
        if (enq >= max_launch) { stuck = true; break; }
        if (ps.solo && hf[4] != 0) ps.solo = false;   // the device handed over to the resident / launch-per-iteration form
        if (la_omp) HIPCHK(launch_la_omp<T>(ctx, ws, tol, max_iter));
        else Lookahead<T>::iterate(ctx, ws, tol, max_iter, lds_cols, ps.solo);
        ++enq;
        if (ps.solo && lds_cols != 0) {
            // the resident form queued right behind the speculative group: a no-op unless that group hands
            // over (the last step of a path), which then costs no trip through the host
            HIPCHK(launch_persist(ctx, ws, tol, max_iter, lds_cols, true));
            ++enq;
        }
    }
    if (stuck) {
        HIPCHK(hipStreamSynchronize(st));
        if (hf[1] == 0) return false;
    }
    return true;
}

// One launch chain per round (engine 0: the fused sweep + tail; the lookahead engine without in-kernel grid synchronisation; the
// reference-order engine; OMP in residual form).
template <typename T>
void pump_rounds(ss_hip_ctx* ctx, Workspace<T>& ws, T tol, uint32_t max_iter, bool la, bool ro, bool omp, ProfSpans& spans, const PumpState& ps)
{
    hipStream_t st = ctx->stream;
    const uint32_t L = (uint32_t)std::max(1, std::min(ctx->lookahead, 64));
    const uint64_t last_round = (uint64_t)max_iter + 1;
    const size_t rhs_stride = (size_t)ws.dims.b_pad * ctx->ldm;   // r-block -> p-block
    for (uint64_t round = 1; round <= last_round; ++round) {
        if (!wait_round(ctx, round, L, "hipStreamQuery(solve loop)")) break;
        if (la) {
            // the launch is a no-op unless a column without cached Gram column enters: time
            // every `profile_every`-th launch and keep the ones that did work (see below)
            const bool timed_la = spans.on && (round % (uint64_t)std::max(1, ctx->profile_every) == 0);
            Lookahead<T>::round(ctx, ws, (uint32_t)round, tol, max_iter, timed_la ? spans.span(ProfKind::Sweep32) : EventPair{});
            continue;
        }
        if (ro) {
            // homotopy-cpu.cpp:236-272 with ONE pass over A per iteration: r = y - A x and p = A d (the direction built
            // from the signs of c - gamma q), the fused sweep [c, q] = A^T [r, p], lambda + the while-test + the check of
            // those signs against the re-computed c (a mismatch rebuilds the direction; p and q are then formed again),
            // the scan + toggle + x update, the inverse update and the next direction
            HIPCHK(launch_ro_round<T>(ctx, ws, 1u, (uint32_t)round, ps.ro_parts, tol, max_iter));
            continue;
        }
        if (omp) {
            // orthogonal matching pursuit round: c = A^T r (one right-hand side), pick,
            // bordered inverse + least squares on the support, new residual
            uint32_t nbo = 0;
            HIPCHK(launch_sweep<T>(ctx, ws.rhs, rhs_stride, 1, ws.c, nullptr, ws.pmax_val, ws.pmax_idx, &nbo, ws.st));
            HIPCHK(launch_omp_tail<T>(ctx, ws, 1, (uint32_t)round, nbo, tol, max_iter));
            continue;
        }
        uint32_t nb = 0;
        // HIP events cost tens of microseconds of stream time each: time every
        // `profile_every`-th fused sweep only (option), still inside the solve
        const bool timed = spans.on && (round % (uint64_t)std::max(1, ctx->profile_every) == 0);
        const EventPair ev = timed ? spans.span(ProfKind::FusedSweep, (uint32_t)round) : EventPair{};
        record(ev.a, st);
        HIPCHK(launch_sweep<T>(ctx, ws.rhs, rhs_stride, 2, ws.c, ws.q, ws.pmax_val, ws.pmax_idx, &nb, ws.st));
        record(ev.b, st);
        HIPCHK(launch_iteration_tail<T>(ctx, ws, 1, (uint32_t)round, nb, tol, max_iter));
    }
}

// The HIP events of a profiled solve into the context's statistics (ctx->prof_spans says what each pair bracketed)
template <typename T>
void account_profile(ss_hip_ctx* ctx, uint32_t scr_launches, const DevState& hs)
{
    ss_hip_stats& S = ctx->stats;
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, ctx->ev_solve0, ctx->ev_solve1));
    S.solve_ms += ms;
    for (size_t i = 0; i < ctx->prof_spans.size(); ++i) {
        const ProfSpan sp = ctx->prof_spans[i];
        HIPCHK(hipEventElapsedTime(&ms, ctx->prof_events[2 * i], ctx->prof_events[2 * i + 1]));
        switch (sp.kind) {
        case ProfKind::FirstSweep:
            S.sweep1_launches += 1;
            S.sweep1_ms += ms;
            break;
        case ProfKind::Screen:
            // the screening pass: fp16 copy of A + the residual block (re-read from L2 by every workgroup: not counted) + norms
            S.screen_launches += scr_launches;
            S.screen_ms += ms;
            S.screen_bytes += (uint64_t)scr_launches * ((uint64_t)ctx->ldm * ctx->n_pad * 2ull + 96ull * ctx->ldm * 2ull + (uint64_t)ctx->n_pad * 4ull);
            break;
        case ProfKind::PathKernel:
            S.res_solve_launches += 1;
            S.res_solve_ms += ms;
            break;
        case ProfKind::FirstReduced:
            S.first16_launches += 1;
            S.first16_ms += ms;
            S.first16_bytes += (uint64_t)ctx->ldm * ctx->n_pad * (uint64_t)ctx->first_pass_elem_bytes + (uint64_t)ctx->ldm * sizeof(T) + (uint64_t)ctx->n_pad * 4ull;
            break;
        case ProfKind::Sweep64First:
            if (ms > 0.02f) {                          // (a launch of a solve that ended at the first pick is a no-op)
                S.sweep64_launches += 1;
                S.sweep64_ms += ms;
            }
            break;
        case ProfKind::Sweep32:
        case ProfKind::EarlyPass: {
            // lookahead sweep: a launch that found nothing to do returns in microseconds.  Bytes per EVENT: a
            // plain pass covers all n columns, the early form's main launch its share of them
            const uint64_t sz = sizeof(T);
            const uint64_t cols = sp.kind == ProfKind::EarlyPass ? S.sweep32_timed_cols : (uint64_t)ctx->n;
            const uint64_t bytes = (uint64_t)ctx->m * cols * sz + 32ull * ctx->m * sz + 32ull * cols * sz;
            if ((double)bytes / (ms * 1e-3) < 50e12) {   // < 50 TB/s: it streamed A
                S.sweep32_launches += 1;
                S.sweep32_ms += ms;
                S.sweep32_bytes_timed += bytes;
            }
            break;
        }
        case ProfKind::FusedSweep:
            if (sp.round <= hs.done_round) {           // only sweeps that did real work: rounds 1 .. done_round
                S.sweep_launches += 1;
                S.sweep_ms += ms;
            }
            break;
        }
    }
}

// developer aid (SS_HIP_SOLO_DEBUG = a path): the log and the verification partials of the last speculative launch
template <typename T>
void dump_solo_debug(Workspace<T>& ws, const DevState& hs, const char* path)
{
    // developer aid: the log and the verification partials of the last solo launch
    const size_t lw = (size_t)kSoloHeaderWords + (size_t)kSoloLogCap * kSoloEntryWords;
    std::vector<uint32_t> lg(lw), vm((size_t)kSoloLogCap * ws.nvwg);
    std::vector<uint64_t> vn((size_t)kSoloLogCap * ws.nvwg);
    HIPCHK(hipMemcpy(lg.data(), ws.solo_log, lw * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(vm.data(), ws.v_max, vm.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(vn.data(), ws.v_min, vn.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (FILE* fp = std::fopen(path, "wb")) {
        const uint32_t hdr[4] = { hs.solo_nlog, ws.nvwg, kSoloEntryWords, kSoloHeaderWords };
        std::fwrite(hdr, 4, 4, fp);
        std::fwrite(lg.data(), 4, lg.size(), fp);
        std::fwrite(vm.data(), 4, vm.size(), fp);
        std::fwrite(vn.data(), 8, vn.size(), fp);
        std::fclose(fp);
    }
}

// ---- which way a single-signal solve goes ---------------------------------------------------------------------------------
// A solve is ONE attempt in one form (solve_once); what the attempt reports decides whether another form takes the signal
// (the ladder in solve_once's verdict section).  A Route is everything a later attempt is told about the earlier ones.
struct Route {
    bool omp = false;              // orthogonal matching pursuit (ss_hip_omp_solve_*)
    bool force_residual = false;   // the Gram form's tolerance guard tripped: residual form (engine 0) for this signal
    bool no_solo = false;          // no speculative launches (callers that run many contexts side by side)
    bool force_ro = false;         // a step-length scan met an exact tie: the reference-order engine (reforder.hip) arbitrates
    bool no_sub = false;           // the subset / screened forms declined the signal: the default engine
    bool no_res = false;           // fp64: the resident tier declined it: the sub-dictionary tier
    bool plain = false;            // the early form asked for the plain speculative form (sticky for the rest of this solve)
    bool rescue = false;           // the screened form declined the signal for a column its ranking missed: once more, with the columns its log names
    uint32_t rescue_why = 0;       // ... the declined attempt's reason bits (kReason*)
    Route after() const { Route r; r.plain = plain; return r; }     // a fresh route that keeps what is sticky
};

// The forms an attempt can take (at most one of sub1 / scr1 / scr64 / scr64r; la / la_omp / ro say which engine stands behind)
struct Forms {
    bool y_direct = false;   // the lookahead engine reads the signal from the caller's device buffer (no copy command)
    bool ro = false;         // reference-order engine (option engine = 3, and the arbiter of tie stalls)
    bool la = false;         // lookahead (Gram-form) engine: the default
    bool la_omp = false;     // OMP in Gram form (k_la_omp)
    bool sub1 = false;       // G = A^T A at hand: the subset form of the batches for ONE signal (subbatch.hip)
    bool scr1 = false;       // fp32 screened form (screen.hip + resident.hip): the default on large dictionaries
    bool scr64 = false;      // fp64 screened form, sub-dictionary tier (2048 columns, a context of its own)
    bool scr64r = false;     // fp64 screened form, resident tier (256 columns, one workgroup)
};

// What a context's options, its size and the route so far allow.  (No side effects: the step-aside counters are applied by the
// caller, so that asking twice gives the same answer.)
template <typename T>
Forms choose_forms(ss_hip_ctx* ctx, const Route& route, const T* y, void* rec_out)
{
    Forms f;
    const bool omp = route.omp;
    f.y_direct = !omp && !route.force_ro && ctx->engine != 3 && Lookahead<T>::supported && ctx->engine >= 1 && !route.force_residual &&
                 on_device(y);
    f.ro = !omp && (route.force_ro || ctx->engine == 3);
    f.la = !omp && Lookahead<T>::supported && ctx->engine >= 1 && !route.force_residual && !f.ro;
    f.la_omp = omp && Lookahead<T>::supported && ctx->engine >= 1 && !route.force_residual && ctx->la_fused >= 1;
    // With G = A^T A at hand (a large batch has run on the context, or option gram_full_after) a single signal takes the
    // subset form of the batches (subbatch.hip): A^T y, one workgroup on 448 columns, the check over all columns — no
    // pass over A beyond A^T y.  What the form does not vouch for is solved again the usual way (no_sub).
    // (where the screened form below applies it is the faster of the two since its first pass reads the fp16 copy — 0.71 ms against
    // 1.0 at configs[1] — and takes the signal; option screen_single = 0 leaves it to this form)
    f.sub1 = f.la && sizeof(T) == 4 && !route.no_sub && ctx->batch_subset && ctx->gram_single && ctx->gram_full != nullptr && sub_form_usable(ctx);
    // Without G: the screened form (screen.hip) — the same subset solve on the subset's own Gram matrix (formed from A), every
    // state of its path then screened against all columns by ONE pass over a half-precision copy of A with a rigorous error
    // bound, instead of the default engine's two fp32 passes.  It stands in for the default speculative engine only
    // (la_fused = 3 with the early form: contexts whose options ask for another engine get that engine).
    // (OMP — ss::omp<float> — takes it too: the resident kernel's OMP statement on the same subset, the same certificate; not with a trace)
    f.scr1 = (f.la || (f.la_omp && ctx->screen_resident && !ctx->tracing)) && sizeof(T) == 4 && !route.no_sub && ctx->la_fused >= 3 && ctx->early_solo &&
             ctx->solo_subset == 256 && (!f.sub1 || screen_first16_usable(ctx)) && screen_form_usable(ctx);
    if (f.scr1) f.sub1 = false;
    // fp64: the same certificate around the fp64 engine — the path is solved by a context of its own on the 2048 columns with
    // the largest |c0| (passes and iterations on 1.6 % of the dictionary), its logged states are screened against all columns
    // (not with a trace or compact records asked for: the sub-context's lists are over ITS columns)
    // (OMP too: the sub-context runs k_la_omp, the certificate is the same — nothing outside the sub-dictionary reaches the pick's |c|)
    f.scr64 = (f.la || f.la_omp) && sizeof(T) == 8 && !route.no_sub && !ctx->tracing && rec_out == nullptr && ctx->la_fused >= 1 && screen64_usable(ctx);
    // ... and before that tier, the RESIDENT tier (resident.hip): the path on the 256 best-ranked columns in ONE workgroup with the
    // Gram values in registers — no sub-context, no host round trip, everything queued in one go; its lists are over the
    // dictionary's own columns, so a trace and compact records work too.  What it does not report goes to the tier above.
    f.scr64r = (f.la || f.la_omp) && sizeof(T) == 8 && !route.no_sub && !route.no_res && ctx->screen_resident && ctx->la_fused >= 1 &&
               !(omp && ctx->tracing) && screen64_usable(ctx) && screen64_resident_usable(ctx);
    return f;
}

// ---- what an attempt reported: the ladder ---------------------------------------------------------------------------------------
// Reads the device state of a finished attempt and decides: report it (*report), fail (the returned status), or hand the signal to
// another form (*again, *next).  Rungs, in the order they are tried:
//   exact tie in a step-length scan            -> reference-order engine (the arbiter; option tie_rerun)
//   fp64 resident tier declined                -> sub-dictionary tier                      (no_res)
//   fp32 screened form declined, a missed column -> the same form once more with it        (rescue)
//   screened form (fp32 / fp64 tier 2) declined -> default engine                           (no_sub)
//   subset form on G declined                  -> default engine                           (no_sub)
//   early form used too many unfetched columns -> plain speculative form                   (plain)
//   Gram-form tolerance guard                  -> residual form                            (force_residual)
//   a resident grid's wait expired             -> launch per iteration, then no in-kernel grid synchronisation (context options)
// Every rung also keeps the statistics (ss_hip_stats) and the step-aside counters of its form.
// the form did not report the signal: it declined or failed it, or its subset's view met a tie
inline bool handed_back(const DevState& hs, bool scr_tie) { return hs.status == kStatusSubsetDecline || hs.status == kStatusSubsetFail || scr_tie; }
// the reasons a rescue can answer (the path ran out of positions / states, or an outside column beat a state) and nothing else wrong
inline bool rescuable_reasons(uint32_t rs)
{
    return (rs & (kReasonPositions | kReasonLog | kReasonColumn)) != 0u &&
           (rs & (kReasonRemoval | kReasonIrregular | kReasonTie | kReasonGuard | kReasonNoCand | kReasonFirstState | kReasonOverflow)) == 0u;
}

template <typename T>
int attempt_verdict(ss_hip_ctx* ctx, const Route& route, const Forms& f, const DevState& hs, Route* next, bool* again, bool* report,
                    char* err, size_t errlen)
{
    const bool omp = route.omp, force_residual = route.force_residual, no_solo = route.no_solo;
    const bool ro = f.ro, la = f.la, la_omp = f.la_omp, sub1 = f.sub1, scr1 = f.scr1, scr64 = f.scr64, scr64r = f.scr64r;
    auto retry = [&](const Route& r) { *next = r; *again = true; return SS_HIP_OK; };

    if (!hs.done) {
        set_err(err, errlen, "solve: internal error, device loop did not terminate");
        return SS_HIP_ERUNTIME;
    }
    // (a tie met by the screened form's subset solve is a tie of the SUBSET's view — on a subset that cannot be certified it may not
    // exist over all columns: such a signal goes to the default engine below, which meets the tie itself if it is real)
    const bool scr_tie = (scr1 || scr64r) && ctx->tie_rerun && !ctx->tie_guard && (hs.tie_stall != 0 || hs.status == kStatusTieRerun);
    if (!ro && !omp && !scr_tie && ctx->tie_rerun && !ctx->tie_guard && (hs.tie_stall != 0 || hs.status == kStatusTieRerun)) {
        // a step-length scan met an exact tie (DevState::tie_stall): whether the strict t > 0 of the reference then
        // derails the path is decided by rounding — the reference-order engine is the arbiter
        ctx->stats.tie_reruns += 1;
        Route r = route.after(); r.no_solo = no_solo; r.force_ro = true;
        return retry(r);
    }
    const bool back = handed_back(hs, scr_tie);
    // (a context whose signals the form hands back more often than not stops trying for a while)
    if (sub1 || scr1 || scr64) ctx->sub_aside.note(back);
    if (scr64r) {
        ctx->res_aside.note(back);
        if (back) {
            const uint32_t rs = hs.sub_reason;
            if (!route.rescue) count_reasons(ctx, rs, scr_tie);
            if (std::getenv("SS_HIP_SUB_DEBUG"))
                std::fprintf(stderr, "[screened form, fp64 resident tier%s] status %u reason 0x%x after %u iterations, %u states logged, K = %u, lambda %g\n",
                             route.rescue ? ", rescue" : "", hs.status, hs.sub_reason, hs.iter, hs.solo_nlog, hs.K, hs.c_inf);
            // (the rescue, as in fp32: a column the ranking left out of the 256 — the tier once more with the columns its log names)
            const bool rescuable = !omp && !route.rescue && !scr_tie && ctx->screen_rescue && !ctx->tracing && screen_first16_usable(ctx) &&
                                   rescuable_reasons(rs);
            if (rescuable) { Route r = route; r.rescue = true; r.rescue_why = rs; return retry(r); }
            // the resident tier does not report this signal: the sub-dictionary tier (2048 columns) takes it next
            ctx->stats.screen_tier2 += 1;
            Route r = route; r.rescue = false; r.no_res = true;
            return retry(r);
        }
        if (hs.status == 0 && route.rescue) ctx->stats.screen_rescued += 1;
        if (hs.status == 0) { ctx->stats.screen_signals += 1; ctx->stats.screen_resident += 1; }
    }
    if ((scr1 || scr64) && back) {
        const uint32_t rs = hs.sub_reason;
        if (!route.rescue) count_reasons(ctx, rs, scr_tie);            // (why the FIRST attempt declined)
        if (std::getenv("SS_HIP_SUB_DEBUG")) {
            std::fprintf(stderr, "[screened form%s] status %u reason 0x%x after %u iterations, %u states logged, K = %u, lambda %g, lambda0 %g\n",
                         route.rescue ? ", rescue" : "", hs.status, hs.sub_reason, hs.iter, hs.solo_nlog, hs.K, hs.c_inf, (double)hs.lambda0);
            if (scr1) screen_debug_recheck(ctx);
        }
        // The rescue (fp32 Homotopy, option screen_rescue): the path ran out of positions / states, or an outside column beat a state, and
        // nothing else was wrong with it — typically a planted column the ranking left out of the subset.  The next attempt scans this
        // attempt's log for such columns (screen.hip: launch_screen_rescue_scan) and repeats the form with them; once.
        const bool rescuable = scr1 && !omp && !route.rescue && !scr_tie && ctx->screen_rescue && ctx->screen_resident && !ctx->tracing &&
                               screen_first16_usable(ctx) && rescuable_reasons(rs);
        if (rescuable) { Route r = route; r.rescue = true; r.rescue_why = rs; return retry(r); }
        ctx->stats.screen_redone += 1;
        Route r = route; r.rescue = false; r.no_sub = true;
        return retry(r);
    }
    if (scr1 && hs.status == 0 && route.rescue) ctx->stats.screen_rescued += 1;
    if ((scr1 || scr64) && hs.status == 0) ctx->stats.screen_signals += 1;
    if (scr1 && hs.status == 0 && ctx->screen_resident && res_solve_usable<float>()) ctx->stats.screen_resident += 1;
    if ((scr1 || scr64r) && hs.status == 0 && (hs.sub_reason & kReasonRechecked)) ctx->stats.screen_recheck += 1;
    if ((scr1 || scr64r) && hs.status == 0 && (hs.sub_reason & kReasonRechecked) && std::getenv("SS_HIP_SUB_DEBUG"))
        std::fprintf(stderr, "[screened form] certified by the exact re-check%s (reason 0x%x)\n",
                     (hs.sub_reason & kReasonRepaired) ? ", last step repaired" : "", hs.sub_reason);
    if (scr1 && ctx->sub_dbg != nullptr) {
        unsigned long long tp[9];
        HIPCHK(hipMemcpy(tp, ctx->sub_dbg, sizeof(tp), hipMemcpyDeviceToHost));
        const double r = tp[8] ? (double)tp[8] : 1.0;
        std::fprintf(stderr, "[k_sub_solve, cycles per round over %llu rounds] chain %.0f  max|c| %.0f  log+scan %.0f  arg-min %.0f  hand-shake+x %.0f  u1/u2 %.0f  "
                             "inverse+signs %.0f  direction %.0f\n", tp[8], tp[0] / r, tp[1] / r, tp[2] / r, tp[3] / r, tp[4] / r, tp[5] / r, tp[6] / r, tp[7] / r);
    }
    if (sub1 && back) {
        ctx->stats.subset_redone += 1;
        count_reasons(ctx, hs.sub_reason, false);
        Route r = route; r.no_sub = true;
        return retry(r);
    }
    if (sub1 && hs.status == 0) ctx->stats.subset_signals += 1;
    if (la && hs.status == kStatusRetryPlain) {
        // the early form's first launch used too many columns beyond the prefetched ones: plain form for this solve
        // (solve_impl switches option early_solo off until this solve has returned)
        Route r = route.after(); r.omp = omp; r.force_residual = force_residual; r.no_solo = no_solo; r.plain = true;
        return retry(r);
    }
    if ((la || la_omp) && hs.status == kStatusRetryResidual) {
        // tolerance too tight for Gram-form correlations (see k_la_init_pick): residual form
        ctx->stats.gram_fallbacks += 1;
        Route r = route.after(); r.omp = omp; r.force_residual = true; r.no_solo = no_solo;
        return retry(r);
    }
    if (la && hs.status == SS_HIP_ERUNTIME && ctx->la_fused >= 2 && (ctx->persist_workers[0] != 0 || ctx->persist_workers[1] != 0)) {
        // the resident kernel gave up on a wait (its grid was not fully resident): this context
        // goes on with one launch per iteration
        ctx->persist_workers[0] = 0;
        ctx->persist_workers[1] = 0;
        ctx->stats.persist_fallbacks += 1;
        Route r = route.after(); r.omp = omp; r.force_residual = force_residual; r.no_solo = no_solo;
        return retry(r);
    }
    if ((la || la_omp) && hs.status == SS_HIP_ERUNTIME && ctx->la_fused >= 1) {
        // k_la_iter's grid barrier expired as well (the GPU is shared with another resident grid):
        // from here on this context uses the form without in-kernel grid synchronisation
        ctx->la_fused = 0;
        ctx->stats.persist_fallbacks += 1;
        Route r = route.after(); r.omp = omp; r.force_residual = force_residual; r.no_solo = no_solo;
        return retry(r);
    }
    if (hs.status != 0) {
        set_err(err, errlen, hs.status == SS_HIP_ECAPACITY
                                 ? "solve: active set outgrew the workspace capacity (4096 columns)"
                                 : "solve: internal error, a device-side wait expired");
        return (int)hs.status;
    }
    *report = true;
    return SS_HIP_OK;
}

template <typename T>
int solve_impl(ss_hip_ctx* ctx, const T* y, ptrdiff_t incy, T tol, uint32_t max_iter, T* x,
               ptrdiff_t incx, uint32_t* iter_out, double* err_out, char* err, size_t errlen,
               Route route = Route(), void* rec_out = nullptr, uint32_t kmax = 0);

// The preconditions the reference asserts on a solve's arguments (homotopy-cpu.cpp:193-199, irls-cpu.cpp:78), in the order every
// entry point reports them: max_iterations, then the tolerance (with_tol: IRLS takes any), then the increments.  `prefix` names
// the entry point in the message.
template <typename T>
int check_solve_args(const char* prefix, uint32_t max_iter, T tol, bool with_tol, ptrdiff_t incy, ptrdiff_t incx, char* err, size_t errlen)
{
    const char* what = nullptr;
    if (max_iter == 0) what = ": max_iterations must be > 0";
    else if (with_tol && !(tol >= std::numeric_limits<T>::epsilon() && tol < T(1))) what = ": tolerance must satisfy eps <= tolerance < 1";
    else if (incy <= 0 || incx <= 0) what = ": vector increments must be positive";
    if (!what) return SS_HIP_OK;
    set_err(err, errlen, std::string(prefix) + what);
    return SS_HIP_EINVAL;
}

// The prologue of a rescue (route.rescue: the screened form — fp32 — or its resident tier — fp64 — declined the signal for a column its
// ranking missed): the scan of the declined attempt's log for such columns — its state, logs and c~0 are still in place, nothing has been
// reset yet.  true: the form runs once more with them.  false: there is nothing to rescue with, *next is the route that hands the signal
// on (fp64: to the sub-dictionary tier, fp32: to the default engine).  scan = false: the form cannot run, nothing is scanned.
template <typename T>
bool rescue_prologue(ss_hip_ctx* ctx, Workspace<T>& ws, T tol, const Route& route, bool scan, Route* next)
{
    constexpr bool tier64 = sizeof(T) == 8;
    uint32_t found = 0;
    // (a decline by the exact re-check alone left the list of the columns that failed it: no scan)
    const bool from_recheck = (route.rescue_why & kReasonRechecked) != 0u && (route.rescue_why & (kReasonPositions | kReasonLog)) == 0u;
    if (scan) {
        if constexpr (tier64) HIPCHK(launch_screen64_rescue_scan(ctx, ws, tol, from_recheck, &found));
        else HIPCHK(launch_screen_rescue_scan(ctx, ws, tol, from_recheck, &found));
    }
    if (std::getenv("SS_HIP_SUB_DEBUG"))
        std::fprintf(stderr, "[screened form%s, rescue] the scan lists %u columns the ranking missed\n", tier64 ? ", fp64 resident tier" : "", found);
    if (scan && found >= 1u && found <= screen_rescue_cap()) {
        ctx->stats.screen_rescue_tried += 1;
        return true;
    }
    *next = route;
    next->rescue = false;
    if (tier64) { ctx->stats.screen_tier2 += 1; next->no_res = true; }
    else { ctx->stats.screen_redone += 1; next->no_sub = true; }
    return false;
}

// One attempt.  Returns the status of the solve, or — with *again set — the route of the next attempt in *next.
template <typename T>
int solve_once(ss_hip_ctx* ctx, const T* y, ptrdiff_t incy, T tol, uint32_t max_iter, T* x,
               ptrdiff_t incx, uint32_t* iter_out, double* err_out, char* err, size_t errlen,
               const Route& route, void* rec_out, uint32_t kmax, Route* next, bool* again)
{
    const bool omp = route.omp, no_solo = route.no_solo;
    auto retry = [&](const Route& r) { *next = r; *again = true; return SS_HIP_OK; };
    return guarded_rt(err, errlen, "solve", [&]() -> int {
        HIPCHK(hipSetDevice(ctx->device));
        const size_t m = ctx->m, n = ctx->n;
        const uint32_t kcap = (uint32_t)std::min<uint64_t>(
            std::min<uint64_t>(n, (uint64_t)max_iter + 1), kKcapLimit);
        ensure_workspace<T>(ctx, 1, kcap);
        Workspace<T>& ws = *ws_of<T>(ctx);
        hipStream_t st = ctx->stream;
        const uint32_t want_trace = ctx->tracing ? (uint32_t)std::min<uint64_t>((uint64_t)max_iter + 2, 1u << 20) : 0u;
        TraceWindow<T> trace_window(ws, want_trace);
        // (OMP does not write entry 0 — it has no initial pick —: a traced solve starts from zeros, not from whatever an earlier
        // allocation left in the buffer, so that a context's trace does not depend on its history)
        if (ctx->tracing) HIPCHK(hipMemsetAsync(ws.trace, 0, (size_t)want_trace * sizeof(TraceEntry), st));
        // (option profile_solve_every = k: with profiling on, only every k-th solve carries the HIP events — each costs
        // stream time, ~0.07 ms per solve in all at 8192 x 65536)
        const bool prof = ctx->profiling != 0 && (ctx->profile_solve_every <= 1 || (ctx->prof_solve_tick++ % (uint64_t)ctx->profile_solve_every) == 0);
        ProfSpans spans(ctx, prof);

        ctx->host_flags[0] = 0;     // the stream is idle here: the previous solve synchronised
        ctx->host_flags[1] = 0;
        ctx->host_flags[2] = 0;
        ctx->host_flags[3] = 0;
        ctx->host_flags[4] = 0;
        if (prof) HIPCHK(hipEventRecord(ctx->ev_solve0, st));
        // ---- prepare: the forms of this attempt, the signal, the state ----
        Forms f = choose_forms<T>(ctx, route, y, rec_out);
        // (lookahead engine with the signal on the device: k_la_reset reads it from the caller's buffer — no copy command)
        if (!f.y_direct) copy_in<T>(ctx, ws.y, y, incy, m);
        const T* const y_dev = f.y_direct ? y : (const T*)nullptr;
        if (!f.la) {
            HIPCHK(hipMemsetAsync(ws.x, 0, (size_t)ctx->n_pad * sizeof(T), st));
            HIPCHK(hipMemsetAsync(ws.d, 0, (size_t)ctx->n_pad * sizeof(T), st));
            HIPCHK(hipMemsetAsync(ws.insup, 0, (size_t)ctx->n_pad, st));
            HIPCHK(hipMemsetAsync(ws.st, 0, sizeof(DevState), st));
            HIPCHK(hipMemsetAsync(ws.ndone, 0, sizeof(uint32_t), st));
            HIPCHK(hipMemcpyAsync(ws.rhs, ws.y, (size_t)ctx->ldm * sizeof(T), hipMemcpyDeviceToDevice, st));
        }
        // (a context whose signals a form hands back more often than not steps that form aside for a while: attempt_verdict keeps the windows)
        if ((f.sub1 || f.scr1 || f.scr64 || f.scr64r) && ctx->sub_aside.take()) { f.sub1 = false; f.scr1 = false; f.scr64 = false; f.scr64r = false; }
        if (f.scr64r && ctx->res_aside.take()) f.scr64r = false;
        if (route.rescue && !f.scr1 && !f.scr64r) ctx->stats.screen_redone += 1;      // (the form has stepped aside meanwhile: the signal is the default engine's after all)
        if (f.scr64r) f.scr64 = false;
        uint32_t scr_launches = 1;
        PumpState ps;
        // end of a solve: the device state to pinned memory, x (and the compact record) to the caller
        bool spec_epilogue = false;
        const bool x_on_device = x != nullptr && on_device(x);
        // (the screened fp32 form's last launch may do k_epilogue's work: scr_single hears where x goes and says whether it did)
        ScrHandoff scr_ho;
        auto enqueue_epilogue = [&]() {
            if (ctx->hs_mapped != nullptr && scr_ho.tail_fused) {
                if (x && !x_on_device) copy_out<T>(ctx, x, incx, ws.x, n);
            } else if (ctx->hs_mapped != nullptr) {
                // one launch: state -> pinned memory, x -> the caller's device buffer (a host x still takes a copy command)
                const uint32_t grid = x_on_device ? std::min<uint32_t>(((uint32_t)n + 1023u) / 1024u, 256u) : 1u;
                hipLaunchKernelGGL((k_epilogue<T>), dim3(std::max(1u, grid)), dim3(256), 0, st, reinterpret_cast<const uint32_t*>(ws.st),
                                   static_cast<uint32_t*>(ctx->hs_mapped), (uint32_t)(sizeof(DevState) / 4), (const T*)ws.x,
                                   x_on_device ? x : (T*)nullptr, (long long)incx, (uint32_t)n,
                                   (f.scr1 || f.scr64r) ? (uint32_t)(offsetof(DevState, status) / 4) : 0xffffffffu, (uint32_t)(offsetof(DevState, need_sweep) / 4));
                HIPCHK(hipGetLastError());
                if (x && !x_on_device) copy_out<T>(ctx, x, incx, ws.x, n);
            } else {
                HIPCHK(hipMemcpyAsync(ctx->hs_pinned, ws.st, sizeof(DevState), hipMemcpyDeviceToHost, st));
                if (x) copy_out<T>(ctx, x, incx, ws.x, n);
            }
            if (rec_out) {
                // compact output (a record that is superseded by a retry below is simply overwritten)
                const unsigned char* stage = pack_records<T>(ctx, ws, 1, kmax);
                HIPCHK(hipMemcpyAsync(rec_out, stage, record_bytes(kmax, sizeof(T)), hipMemcpyDefault, st));
            }
            if (prof) HIPCHK(hipEventRecord(ctx->ev_solve1, st));
        };
        // full-G mode (fp32): G = A^T A of the context as the cache.  G exists once a large batch has run
        // on the context, or — opt-in, option gram_full_after > 0 — is made here after that many single-signal
        // solves (17 GiB and a few tenths of a second at C2 against ~0.6 ms saved per solve from then on).
        struct FullGramView {
            Workspace<T>& w; bool on = false;
            ~FullGramView() { if (on) { w.gcache = w.gcache_own; w.gpitch = w.gpitch_own; w.slot_of = w.slot_of_own; w.gram_is_full = false; } }
        } full_view{ ws };
        auto enter_full_gram = [&]() {
            if (sizeof(T) != 4 || ctx->engine < 1 || ws.gram_is_full || !ctx->gram_single) return;     // (a retry runs inside the outer view)
            if (!ctx->gram_full && ctx->gram_full_after > 0 && ctx->single_solves + 1 >= (uint64_t)ctx->gram_full_after)
                (void)ensure_full_gram(ctx);
            if (!ctx->gram_full) return;
            if (!ws.slot_identity) {
                std::vector<int32_t> iota(ctx->n_pad);
                for (uint32_t i = 0; i < ctx->n_pad; ++i) iota[i] = (int32_t)i;
                HELD(ws.own, hipMalloc, &ws.slot_identity, (size_t)ctx->n_pad * sizeof(int32_t));
                HIPCHK(hipMemcpy(ws.slot_identity, iota.data(), (size_t)ctx->n_pad * sizeof(int32_t), hipMemcpyHostToDevice));
            }
            ws.gcache_own = ws.gcache; ws.gpitch_own = ws.gpitch; ws.slot_of_own = ws.slot_of;
            ws.gcache = reinterpret_cast<T*>(ctx->gram_full);
            ws.gpitch = ctx->gram_pitch;
            ws.slot_of = ws.slot_identity;
            ws.gram_is_full = true;
            full_view.on = true;
        };
        // ---- the first pass and the form's own launches ----
        uint32_t nb1 = 0;
        if (f.scr64r || f.sub1 || f.scr1) {
            // the screened forms that queue everything in one go (fp64: the resident tier; fp32: the screened form, or the subset form on G)
            Lookahead<T>::ensure(ctx, ws, kcap);
            const bool screened = f.scr64r || f.scr1;
            if (route.rescue && !rescue_prologue<T>(ctx, ws, tol, route, screened, next)) { *again = true; return SS_HIP_OK; }
            const bool rescue = route.rescue;
            // (the screened form's first pass — A^T y over all columns — reads the reduced-precision copy too: screen.hip, k_scr_first)
            const bool first16 = screened && screen_first16_usable(ctx);
            // x, d, flags, DevState, r = y (OMP: done above): by k_la_reset — or, where the fp8 ranking pass is the first launch of the
            // attempt (fp32 form, first attempt; decided here, before anything is queued), by that pass's workgroups in their prologue
            bool reset_folded = false;
            if constexpr (sizeof(T) == 4) {
                scr_handoff_mask(&scr_ho);
                if (f.scr1 && !f.sub1 && !omp && !rescue && first16 && (scr_ho.mask & 4u) && screen_first8_folds(ctx)) {
                    scr_ho.reset = la_reset_args<float>(ctx, ws, false, y_dev, incy);
                    reset_folded = true;
                }
            }
            if (!omp && !reset_folded) HIPCHK(launch_la_reset<T>(ctx, ws, false, y_dev, incy));
            if (!first16) first_sweep<T>(ctx, ws, ws.c0, spans, &nb1);
            if (f.sub1) {
                if constexpr (sizeof(T) == 4) {
                    // G = A^T A is at hand: the subset form (subbatch.hip) on c0 in ws.c0
                    grow_device(ctx->own, ctx->sub_buf, ctx->sub_buf_bytes, sub_buffer_bytes(1), 1, "hipMalloc(sub_buf)");
                    HIPCHK(launch_sub_form(ctx, ws, 1, ws.c0, tol, max_iter));
                }
            } else {
                const EventPair first = (first16 && !rescue) ? spans.span(ProfKind::FirstReduced) : EventPair{};
                const EventPair screen = spans.span(ProfKind::Screen), path = spans.span(ProfKind::PathKernel);
                if constexpr (sizeof(T) == 8) HIPCHK(launch_screen64_resident(ctx, ws, tol, max_iter, first16, omp, first, screen, path, rescue));
                else {
                    if (x_on_device) { scr_ho.x_dst = reinterpret_cast<float*>(x); scr_ho.incx = (long long)incx; }
                    HIPCHK(scr_single(ctx, ws, tol, max_iter, first16, first, screen, path, omp, rescue, &scr_ho));
                }
            }
        } else if (f.scr64) {
            if constexpr (sizeof(T) == 8) {
                Lookahead<T>::ensure(ctx, ws, kcap);
                if (!omp) HIPCHK(launch_la_reset<T>(ctx, ws, false, y_dev, incy));     // x, d, flags, DevState, r = y (OMP: done above)
                // (the first pass — A^T y over all columns, which here only ranks them — over the reduced-precision copy: k_scr_first)
                const bool first16 = screen_first16_usable(ctx);
                if (first16) {
                    HIPCHK(screen64_gather(ctx, nullptr, ws.rhs, spans.span(ProfKind::FirstReduced)));
                } else {
                    first_sweep<T>(ctx, ws, ws.c0, spans, &nb1);
                    HIPCHK(screen64_gather(ctx, ws.c0, ws.rhs));
                }
                HIPCHK(hipStreamSynchronize(st));
                ss_hip_ctx* sub = screen64_sub(ctx);
                sub->strict_sign = ctx->strict_sign; sub->zero_on_removal = ctx->zero_on_removal; sub->tie_guard = ctx->tie_guard;
                sub->tie_rerun = ctx->tie_rerun; sub->engine = ctx->engine; sub->lookahead = ctx->lookahead;
                sub->pass_tile128 = 1;                   // (128-column tiles: the sub-dictionary has 16 of them)
                const uint64_t ties0 = sub->stats.tie_reruns, gf0 = sub->stats.gram_fallbacks, pf0 = sub->stats.persist_fallbacks;
                uint32_t it_s = 0;
                double e_s = 0.0;
                Route rs; rs.omp = omp; rs.no_sub = true;
                const int rc_s = solve_impl<T>(sub, ws.rhs, 1, tol, max_iter, screen64_xsub(ctx), 1, &it_s, &e_s, err, errlen, rs, nullptr, 0);
                HIPCHK(hipSetDevice(ctx->device));
                const DevState hsub = *static_cast<const DevState*>(sub->hs_pinned);
                const bool clean = rc_s == SS_HIP_OK && sub->stats.tie_reruns == ties0 && sub->stats.gram_fallbacks == gf0 &&
                                   sub->stats.persist_fallbacks == pf0 && it_s >= 1u && it_s <= 192u;
                if (!clean) {
                    // the sub-context's solve left its common path (a tie re-run, a residual-form retry, too many states): the usual engine
                    if (std::getenv("SS_HIP_SUB_DEBUG"))
                        std::fprintf(stderr, "[screened form, fp64] handed back: sub-context status %u iter %u K %u ties %llu gram fallbacks %llu persist fallbacks %llu (%s)\n",
                                     hsub.status, hsub.iter, hsub.K, (unsigned long long)sub->stats.tie_reruns, (unsigned long long)sub->stats.gram_fallbacks,
                                     (unsigned long long)sub->stats.persist_fallbacks, err ? err : "");
                    ctx->stats.screen_redone += 1;
                    Route r = route; r.no_sub = true;
                    return retry(r);
                }
                HIPCHK(screen64_certify(ctx, ws, ws.rhs, it_s, tol, e_s, hsub.K, spans.span(ProfKind::Screen), omp, first16));
                scr_launches = (it_s + 95u) / 96u;
            }
        } else if (f.la_omp) {
            Lookahead<T>::ensure(ctx, ws, kcap);
            enter_full_gram();
            first_sweep<T>(ctx, ws, ws.c0, spans, &nb1);
            if (!ws.gram_is_full) HIPCHK(hipMemsetAsync(ws.slot_of, 0xff, (size_t)ctx->n_pad * sizeof(int32_t), st));   // nothing cached yet
        } else if (f.la) {
            Lookahead<T>::ensure(ctx, ws, kcap);
            enter_full_gram();
            HIPCHK(launch_la_reset<T>(ctx, ws, !ws.gram_is_full, y_dev, incy));     // x, d, flags, slot map, exchange area, DevState, r = y
            first_sweep<T>(ctx, ws, ws.c0, spans, &nb1);
            // Speculative form (fp32): the default
            // (la_fused = 3).  It also runs where the resident kernel cannot (dictionaries too wide for one
            // launch to own every column).
            const bool solo_wanted = ctx->la_fused >= 3;
            // (not with the full Gram matrix as the cache: there every entering column's row slice is a gather of
            // 256 scattered entries of a 256-KiB row in the iteration's chain — 1.81 ms per C2 solve against 1.55 ms)
            ps.solo = solo_wanted && !no_solo && ctx->solo_off_solves == 0 && sizeof(T) == 4 &&
                      (!ws.gram_is_full || ctx->solo_full_gram) && la_solo_usable(ctx);
            if (solo_wanted && !ps.solo && ctx->solo_off_solves > 0 && !no_solo) ctx->solo_off_solves -= 1;
            ps.solo_started = ps.solo;
            ps.early = ps.solo && ctx->early_solo && sizeof(T) == 4 && !ws.gram_is_full && ctx->n > 32u * 512u && ws.gcap >= 160 &&
                       ctx->sweep32_variant == 0 && ws.subg != nullptr && !ws.la_dbg;
            if (ps.early) {
                // resident tier of the launch queued behind the solo group (the last step of the path)
                uint32_t lc = std::min<uint32_t>((ws.dims.kcap + 15u) & ~15u, kLaLdsSmall);
                if (ctx->la_fused < 2 || !la_persist_usable(ctx, lc)) lc = 0;
                ps.early_lds_cols = lc;
                // (the main launch of each early-form pass covers its share of the columns: both passes of the solve are timed)
                const EventPair pass1 = spans.span(ProfKind::EarlyPass), pass2 = spans.span(ProfKind::EarlyPass);
                early_prologue(ctx, ws, nb1, tol, max_iter, lc, pass1, pass2);
                // The typical solve is complete with what is queued now: its epilogue (state, x, record) goes right
                // behind instead of after a trip through the host (host notices `done`, three enqueues: ~70 us).
                // Should the pump below have to queue more work, the epilogue is simply issued again at the end.
                enqueue_epilogue();
                spec_epilogue = true;
            } else {
                // (a span only where a sweep is launched: none with the full Gram matrix as the cache)
                const uint32_t fc = Lookahead<T>::first_cols(ctx, ws);
                Lookahead<T>::init(ctx, ws, nb1, tol, ps.solo, fc == 0 ? EventPair{} : spans.span(fc > 32 ? ProfKind::Sweep64First : ProfKind::Sweep32));
            }
        } else if (f.ro) {
            // c = A^T y in reference order, first pick with the column norm as a chain dot product
            HIPCHK(launch_ro_sweep<T>(ctx, ws.rhs, 0, ws.c, 0, ws.dims.n_pad, 1, 1u, ws.pmax_val, ws.pmax_idx, ws.dims.pmax_stride, &ps.ro_parts, ws.st, false));
            HIPCHK(launch_ro_init<T>(ctx, ws, 1u, ps.ro_parts, tol));
        } else if (!omp) {
            first_sweep<T>(ctx, ws, ws.c, spans, &nb1);
            HIPCHK(launch_init<T>(ctx, ws, 1, nb1, tol));
            HIPCHK(launch_rp<T>(ctx, ws, 1));
        }

        // ---- pump: the rounds the host has to queue ----
        if (f.sub1 || f.scr1 || f.scr64 || f.scr64r) {
            // (everything is queued: selection, the solve, the check)
        } else if ((f.la && ctx->la_fused) || f.la_omp) {
            if (!pump_fused<T>(ctx, ws, tol, max_iter, f.la, f.la_omp, spans, ps)) {
                set_err(err, errlen, "solve: internal error, lookahead loop made no progress");
                return SS_HIP_ERUNTIME;
            }
        } else {
            pump_rounds<T>(ctx, ws, tol, max_iter, f.la, f.ro, omp, spans, ps);
        }

        // ---- epilogue and verdict ----
        if (!(spec_epilogue && !ps.enqueued)) enqueue_epilogue();
        HIPCHK(hipStreamSynchronize(st));
        const DevState hs = *static_cast<const DevState*>(ctx->hs_pinned);
        {
            bool report = false;
            const int vrc = attempt_verdict<T>(ctx, route, f, hs, next, again, &report, err, errlen);
            if (!report) return vrc;
        }
        // ---- account: the caller's outputs, the statistics ----
        if (iter_out) *iter_out = hs.iter;
        if (err_out) *err_out = hs.c_inf;
        if (f.la && ws.la_dbg && !f.scr64) {                 // (fp64 screened form: the stamps are the sub-context's, dumped by its solve)
            if (const char* path = std::getenv("SS_HIP_LA_DEBUG")) {
                std::vector<uint64_t> tsb(2048 * 8);
                HIPCHK(hipMemcpy(tsb.data(), ws.la_dbg, tsb.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
                if (FILE* fp = std::fopen(path, "wb")) { std::fwrite(tsb.data(), sizeof(uint64_t), tsb.size(), fp); std::fclose(fp); }
            }
        }
        ctx->last_trace.clear();
        if (ctx->tracing && ws.trace) fetch_trace(ctx, ws, hs.iter);

        ctx->stats.solves += 1;
        ctx->single_solves += 1;
        if (ps.solo_started) {
            // Speculative launches that failed their check cost a replay and the rest of the solve in the
            // resident form; contexts whose problems do that on most solves stop speculating for a while.
            ctx->stats.solo_solves += 1;
            ctx->stats.solo_retries += hs.solo_fails;
            // (private counters: the decision must not depend on whether the caller reset the statistics)
            ctx->solo_seen += 1;
            ctx->solo_failed += hs.solo_fails;
            if (ctx->solo_seen >= 8 && 2 * ctx->solo_failed > ctx->solo_seen) ctx->solo_off_solves = 64;
            const char* path = hs.solo_fails ? std::getenv("SS_HIP_SOLO_DEBUG") : nullptr;
            if (path != nullptr) dump_solo_debug<T>(ws, hs, path);
        }
        ctx->stats.iterations += hs.iter;
        if (f.la || f.la_omp) ctx->stats.lookahead_sweeps += hs.nsweeps;
        if (f.ro) ctx->stats.ro_resweeps += hs.nsweeps;
        if (prof) account_profile<T>(ctx, scr_launches, hs);
        return SS_HIP_OK;
    });
}

// The solve: validate once, then attempts until one of them reports (at most one per rung of the ladder: every retry sets a
// flag of the route or changes the context so that the same rung cannot be taken twice).
template <typename T>
int solve_impl(ss_hip_ctx* ctx, const T* y, ptrdiff_t incy, T tol, uint32_t max_iter, T* x,
               ptrdiff_t incx, uint32_t* iter_out, double* err_out, char* err, size_t errlen,
               Route route, void* rec_out, uint32_t kmax)
{
    if (!ctx) { set_err(err, errlen, "solve: null context"); return SS_HIP_EINVAL; }
    if (ctx->kind != 0) { set_err(err, errlen, "solve: this context was created for IRLS"); return SS_HIP_EINVAL; }
    if (ctx->is_f64 != (sizeof(T) == 8)) {
        set_err(err, errlen, "solve: element type of the call does not match the context");
        return SS_HIP_ETYPE;
    }
    if (!y || (!x && !rec_out)) { set_err(err, errlen, "solve: y and x must not be null"); return SS_HIP_EINVAL; }
    if (const int rc = check_solve_args<T>("solve", max_iter, tol, true, incy, incx, err, errlen)) return rc;
    // (a retry in the plain speculative form runs — with everything it may fall back to in turn — with option early_solo off)
    struct EarlyKeep { ss_hip_ctx* c; int keep; bool on = false; ~EarlyKeep() { if (on) c->early_solo = keep; } } early_keep{ ctx, ctx->early_solo };
    for (int attempt = 0; attempt < 16; ++attempt) {
        Route next;
        bool again = false;
        if (route.plain && !early_keep.on) { early_keep.on = true; ctx->early_solo = 0; }
        const int rc = solve_once<T>(ctx, y, incy, tol, max_iter, x, incx, iter_out, err_out, err, errlen, route, rec_out, kmax, &next, &again);
        if (!again) return rc;
        route = next;
    }
    set_err(err, errlen, "solve: internal error, the forms kept handing the signal on");
    return SS_HIP_ERUNTIME;
}

// ---- batched solve: B signals share the sensing matrix and advance in lock-step ---------
// Per round the 2*B correlation GEMVs are two MFMA GEMMs ([c] = R·Atᵀ, [q] = P·Atᵀ, gemm.hip);
// the active-set tail runs for all signals at once (grid.y = slot).  A signal that has
// terminated turns its kernels into no-ops; the solve ends when every slot is done.

// Reserves the memory of G = A^T A ahead of time, on a helper thread (ss_hip_ctx::gram_reserve_thread): started by the first batch
// of >= 4 signals a context receives, where G would fit the budget and is at most an eighth of the device's memory.
void gram_reserve_start(ss_hip_ctx* ctx, size_t B)
{
    if (!ctx->gram_reserve || ctx->gram_full || ctx->gram_reserve_thread || B < 4 || ctx->engine < 1 || ctx->batch_gram_min <= 0) return;
    const size_t np = ctx->n_pad;
    const size_t bytes = np * ((np + 1023) / 1024 * 1024) * sizeof(float);
    if (ctx->gram_full_gib <= 0 || bytes > ((size_t)ctx->gram_full_gib << 30)) return;
    size_t free_b = 0, total_b = 0;
    if (hipSetDevice(ctx->device) != hipSuccess || hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return; }
    if (bytes > total_b / 8 || bytes + ((size_t)16 << 30) > free_b) return;
    const int device = ctx->device;
    float** slot = &ctx->gram_reserved;
    // (the thread's own, unowned until the join: gram_reserve_join hands it to the context's owner)
    try {
        ctx->gram_reserve_thread.reset(new std::thread([device, bytes, slot]() {
            float* p = nullptr;
            if (hipSetDevice(device) != hipSuccess || hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); p = nullptr; }
            *slot = p;
        }));
    } catch (...) {
        ctx->gram_reserve_thread.reset();       // no thread, or no memory for one: no reservation
    }
}

// The join of that thread (none: nothing happens): what it obtained now belongs to the context's owner.
void gram_reserve_join(ss_hip_ctx* ctx)
{
    if (!ctx->gram_reserve_thread) return;
    ctx->gram_reserve_thread->join();
    ctx->gram_reserve_thread.reset();
    ctx->own.adopt_device(ctx->gram_reserved);
}

// The full Gram matrix G = A^T A for the batched Gram form: one GEMM of 2 m n^2 flops on the MFMA units (0.55 s at C2), kept in
// the context for later batches.  false if it does not fit the budget.
bool ensure_full_gram(ss_hip_ctx* ctx)
{
    if (ctx->gram_full) return true;
    const size_t np = ctx->n_pad;
    const uint32_t pitch = (uint32_t)((np + 1023) / 1024 * 1024);
    const size_t bytes = np * (size_t)pitch * sizeof(float);
    if (ctx->gram_full_gib <= 0 || bytes > ((size_t)ctx->gram_full_gib << 30)) return false;
    float* G = nullptr;
    const auto t_alloc = std::chrono::steady_clock::now();
    // (reserved ahead on a helper thread: what is left of that allocation is all this batch waits for)
    gram_reserve_join(ctx);
    G = ctx->gram_reserved;
    ctx->gram_reserved = nullptr;
    if (G == nullptr) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || bytes + ((size_t)8 << 30) > free_b) {
            (void)hipGetLastError();
            return false;
        }
        if (ctx->own.device(&G, bytes) != hipSuccess) return false;
    }
    ctx->stats.gram_alloc_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_alloc).count();
    Holdings timing;         // (the two events of this build alone)
    hipEvent_t g0 = nullptr, g1 = nullptr;
    if (timing.event(&g0) != hipSuccess || timing.event(&g1) != hipSuccess) g0 = g1 = nullptr;
    if (g0) (void)hipEventRecord(g0, ctx->stream);
    const hipError_t e = ctx->gram_symmetric
        ? launch_gemm_sym_f32(ctx, G, pitch)
        : launch_gemm_tn_f32(ctx, static_cast<const float*>(ctx->At), (uint32_t)np, ctx->ldm, G, pitch, nullptr, false);
    if (g1) (void)hipEventRecord(g1, ctx->stream);
    if (e != hipSuccess) { (void)ctx->own.drop(G); throw HipFail{ e, "launch_gemm_tn_f32(full Gram)" }; }
    if (g0 && g1 && hipEventSynchronize(g1) == hipSuccess) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, g0, g1) == hipSuccess) ctx->stats.gram_build_ms += ms;
    }
    (void)hipGetLastError();
    ctx->gram_full = G;
    ctx->gram_pitch = pitch;
    ctx->stats.gram_full_builds += 1;
    return true;
}

// Column form of mid-size batches: makes sure the context holds the Gram-column cache ((max_iter + 2) * per rows of
// n_pad fp32, rounded up to 1024 columns), the row tables and the pass lists for chunks of `per` signals.  Returns
// false — nothing thrown, the sticky error cleared — when that does not fit the budget (option gram_full_gib) or the
// free HBM, or an allocation fails: the dispatcher then runs the batch another way.  Sizes only grow; the buffers are
// released with the context.
bool ensure_bcol(ss_hip_ctx* ctx, size_t per, uint32_t max_iter)
{
    const size_t np = ctx->n_pad;
    const size_t pitchc = (np + 1023) / 1024 * 1024;
    const size_t rows_needed = ((size_t)max_iter + 2) * per;
    Holdings& own = ctx->own;
    if (ctx->bcol_cache_rows < rows_needed) {
        const size_t bytes = rows_needed * pitchc * sizeof(float);
        const size_t held = ctx->bcol_cache_rows * pitchc * sizeof(float);
        if (ctx->gram_full_gib <= 0 || bytes > ((size_t)ctx->gram_full_gib << 30)) return false;
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return false; }
        if (bytes + ((size_t)4 << 30) > free_b + held) return false;          // keep 4 GiB for everything else
        (void)own.drop(ctx->bcol_cache);
        ctx->bcol_cache_rows = 0;
        if (own.device(&ctx->bcol_cache, bytes) != hipSuccess) return false;
        ctx->bcol_cache_rows = rows_needed;
    }
    if (ctx->bcol_slot_rows < per) {
        (void)own.drop(ctx->bcol_slot);
        ctx->bcol_slot_rows = 0;
        if (own.device(&ctx->bcol_slot, per * np * sizeof(int32_t)) != hipSuccess) return false;
        ctx->bcol_slot_rows = per;
    }
    if (!ctx->bcol_lists && own.device(&ctx->bcol_lists, 2 * 1024 * sizeof(uint32_t)) != hipSuccess) return false;
    return true;
}

// ---- what the batch drivers share --------------------------------------------------------------------------------------------
// What a batch entry point received.  Signal g is y(g); its outputs are x(g) (null without X), rec(g) (null without compact
// records) and report(g, ...).
template <typename T>
struct BatchCall {
    const T* Y;
    size_t B;
    ptrdiff_t y_stride, incy;
    T tol;
    uint32_t max_iter;
    T* X;
    ptrdiff_t x_stride, incx;
    uint32_t* iter_out;
    double* err_out;
    char* err;
    size_t errlen;
    void* rec_out;
    uint32_t kmax;

    const T* y(size_t g) const { return Y + (ptrdiff_t)g * y_stride; }
    T* x(size_t g) const { return X ? X + (ptrdiff_t)g * x_stride : nullptr; }
    unsigned char* rec(size_t g) const { return rec_out ? static_cast<unsigned char*>(rec_out) + g * record_bytes(kmax, sizeof(T)) : nullptr; }
    void report(size_t g, uint32_t iter, double e) const
    {
        if (iter_out) iter_out[g] = iter;
        if (err_out) err_out[g] = e;
    }
};

// The argument checks of a Homotopy / OMP batch entry, in the order they are reported: null context, a context made for IRLS, the
// element type (SS_HIP_ETYPE; every other one is SS_HIP_EINVAL), null Y or no output, kmax and the alignment of the records; then,
// for a batch that has signals (B = 0 is SS_HIP_OK and nothing to do), max_iterations, the tolerance and the increments.
// (The _compact entry points report null records before any of these.)
template <typename T>
int check_batch_call(const ss_hip_ctx* ctx, const BatchCall<T>& c)
{
    if (!ctx) { set_err(c.err, c.errlen, "solve_batch: null context"); return SS_HIP_EINVAL; }
    if (ctx->kind != 0) { set_err(c.err, c.errlen, "solve_batch: this context was created for IRLS"); return SS_HIP_EINVAL; }
    if (ctx->is_f64 != (sizeof(T) == 8)) { set_err(c.err, c.errlen, "solve_batch: element type mismatch"); return SS_HIP_ETYPE; }
    if (!c.Y || (!c.X && !c.rec_out)) { set_err(c.err, c.errlen, "solve_batch: Y and the output must not be null"); return SS_HIP_EINVAL; }
    if (c.rec_out && (c.kmax == 0 || c.kmax > kKcapLimit || (reinterpret_cast<uintptr_t>(c.rec_out) & 7u))) {
        set_err(c.err, c.errlen, "solve_batch_compact: kmax must be 1..4096 and records 8-byte aligned");
        return SS_HIP_EINVAL;
    }
    if (c.B == 0) return SS_HIP_OK;
    return check_solve_args<T>("solve_batch", c.max_iter, c.tol, true, c.incy, c.incx, c.err, c.errlen);
}

// Signal g of a batch alone, through solve_impl with this route; its outputs go to index g.  (solve_impl sets `err` itself.)
template <typename T>
int solve_alone(ss_hip_ctx* ctx, const BatchCall<T>& c, size_t g, const Route& route)
{
    uint32_t it = 0;
    double e = 0.0;
    const int rc = solve_impl<T>(ctx, c.y(g), c.incy, c.tol, c.max_iter, c.x(g), c.incx, &it, &e, c.err, c.errlen, route, c.rec(g), c.kmax);
    if (rc == SS_HIP_OK) c.report(g, it, e);
    return rc;
}

// Signals b0 .. b0 + Bc - 1 into the rows of ws.y: one 2-D copy when their elements are contiguous, else row by row
template <typename T>
void upload_chunk(ss_hip_ctx* ctx, Workspace<T>& ws, const BatchCall<T>& c, size_t b0, uint32_t Bc)
{
    const size_t m = ctx->m, ldm = ctx->ldm;
    if (c.incy == 1) {
        HIPCHK(hipMemcpy2DAsync(ws.y, ldm * sizeof(T), c.y(b0), (size_t)c.y_stride * sizeof(T), m * sizeof(T), Bc, hipMemcpyDefault, ctx->stream));
    } else {
        for (uint32_t b = 0; b < Bc; ++b) copy_in<T>(ctx, ws.y + (size_t)b * ldm, c.y(b0 + b), c.incy, m);
    }
}

// ... and the rows of ws.x to the caller's X (which must not be null), the same way
template <typename T>
void download_chunk(ss_hip_ctx* ctx, Workspace<T>& ws, const BatchCall<T>& c, size_t b0, uint32_t Bc)
{
    const size_t n = ctx->n, np = ctx->n_pad;
    if (c.incx == 1) {
        HIPCHK(hipMemcpy2DAsync(c.x(b0), (size_t)c.x_stride * sizeof(T), ws.x, np * sizeof(T), n * sizeof(T), Bc, hipMemcpyDefault, ctx->stream));
    } else {
        for (uint32_t b = 0; b < Bc; ++b) copy_out<T>(ctx, c.x(b0 + b), c.incx, ws.x + (size_t)b * np, n);
    }
}

// The start of a chunk of Bc signals (already in ws.y) in the fp32 forms that take c0 from the batch GEMM: the slots' state
// cleared, Rblk = y, c_b = A^T y_b for every signal (residual_vector with x = 0, homotopy-cpu.cpp:215), the first picks.
// Returns the number of partials of the absmax pass.  time_c0: the events ev_c0a / ev_c0b around the GEMM.
inline uint32_t begin_gemm_chunk(ss_hip_ctx* ctx, Workspace<float>& ws, uint32_t Bc, float tol, bool time_c0)
{
    using T = float;
    hipStream_t st = ctx->stream;
    const size_t ldm = ctx->ldm, np = ctx->n_pad, bp = ws.dims.b_pad;
    const uint32_t rows = (Bc + 127u) / 128u * 128u;          // GEMM rows of the block
    HIPCHK(hipMemsetAsync(ws.x, 0, (size_t)Bc * np * sizeof(T), st));
    HIPCHK(hipMemsetAsync(ws.d, 0, (size_t)Bc * np * sizeof(T), st));
    HIPCHK(hipMemsetAsync(ws.insup, 0, (size_t)Bc * np, st));
    HIPCHK(hipMemsetAsync(ws.st, 0, (size_t)Bc * sizeof(DevState), st));
    HIPCHK(hipMemsetAsync(ws.ndone, 0, sizeof(uint32_t), st));
    HIPCHK(hipMemsetAsync(ws.rhs, 0, 2 * bp * ldm * sizeof(T), st));
    HIPCHK(hipMemcpyAsync(ws.rhs, ws.y, (size_t)Bc * ldm * sizeof(T), hipMemcpyDeviceToDevice, st));
    uint32_t nparts = 0;
    if (time_c0 && !ctx->ev_c0a) { HELD(ctx->own, hipEventCreate, &ctx->ev_c0a); HELD(ctx->own, hipEventCreate, &ctx->ev_c0b); }
    if (time_c0) HIPCHK(hipEventRecord(ctx->ev_c0a, st));
    HIPCHK(launch_gemm_tn_f32(ctx, ws.rhs, rows, (uint32_t)ldm, ws.c, (uint32_t)np, nullptr));
    if (time_c0) HIPCHK(hipEventRecord(ctx->ev_c0b, st));
    HIPCHK(launch_absmax<T>(ctx, ws, Bc, &nparts));
    HIPCHK(launch_init<T>(ctx, ws, Bc, nparts, tol));
    return nparts;
}

// What a slot of a lock-step chunk reported: it must have terminated, with a clean status
inline int check_slot_status(const DevState& hs, char* err, size_t errlen)
{
    if (!hs.done) { set_err(err, errlen, "solve_batch: internal error, a signal did not terminate"); return SS_HIP_ERUNTIME; }
    if (hs.status != 0) {
        set_err(err, errlen, hs.status == SS_HIP_ECAPACITY ? "solve_batch: active set outgrew the workspace capacity"
                                                           : "solve_batch: internal error, a device-side wait expired");
        return (int)hs.status;
    }
    return SS_HIP_OK;
}

// Several signals in the reference-order engine at once (reforder.hip): up to ro_slots_max() of them share every pass
// over A — the sweep carries [r, p] of each — and run in lock-step like the batched forms; each signal's words are
// exactly those of a solve on its own (the slots share nothing but the dictionary tile in LDS).  Used for a batch's tie
// re-runs and for batches in engine 3.  sig: the `count` signals' indices into the call (nullptr: 0 .. count-1).
template <typename T>
int solve_batch_ro(ss_hip_ctx* ctx, const BatchCall<T>& c, const size_t* sig, size_t count)
{
    const T tol = c.tol;
    const uint32_t max_iter = c.max_iter;
    return guarded_rt(c.err, c.errlen, "solve_batch", [&]() -> int {
        HIPCHK(hipSetDevice(ctx->device));
        const size_t m = ctx->m, n = ctx->n, ldm = ctx->ldm, np = ctx->n_pad;
        const uint32_t kcap = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(n, (uint64_t)max_iter + 1), kKcapLimit);
        const size_t per = std::max<uint32_t>(1u, std::min<uint32_t>(ro_slots_max(ctx, sizeof(T) == 8), (uint32_t)std::max(1, ctx->ro_slots)));
        hipStream_t st = ctx->stream;
        std::vector<DevState> hs;
        for (size_t j0 = 0; j0 < count; j0 += per) {
            const uint32_t R = (uint32_t)std::min(per, count - j0);
            const uint32_t Rg = R <= 2 ? R : (R <= 4 ? 4u : 8u);  // the sweep carries 1, 2, 4 or 8 slots: the workspace holds that many
            auto gidx = [&](uint32_t b) { return sig ? sig[j0 + b] : j0 + b; };
            ensure_workspace<T>(ctx, Rg, kcap);
            Workspace<T>& ws = *ws_of<T>(ctx);
            const uint32_t want_trace = (ctx->tracing && gidx(0) == 0) ? (uint32_t)std::min<uint64_t>((uint64_t)max_iter + 2, 1u << 20) : 0u;
            TraceWindow<T> trace_window(ws, want_trace);

            ctx->host_flags[0] = 0;
            ctx->host_flags[1] = 0;
            HIPCHK(hipMemsetAsync(ws.y, 0, (size_t)Rg * ldm * sizeof(T), st));
            for (uint32_t b = 0; b < R; ++b) copy_in<T>(ctx, ws.y + (size_t)b * ldm, c.y(gidx(b)), c.incy, m);
            HIPCHK(hipMemsetAsync(ws.x, 0, (size_t)R * np * sizeof(T), st));
            HIPCHK(hipMemsetAsync(ws.d, 0, (size_t)R * np * sizeof(T), st));
            HIPCHK(hipMemsetAsync(ws.insup, 0, (size_t)R * np, st));
            HIPCHK(hipMemsetAsync(ws.st, 0, (size_t)Rg * sizeof(DevState), st));
            // (a slot of the group that carries no signal is "done" from the start: DevState::done is its first word)
            for (uint32_t b = R; b < Rg; ++b) HIPCHK(hipMemsetAsync(&ws.st[b], 0x01, sizeof(uint32_t), st));
            HIPCHK(hipMemsetAsync(ws.ndone, 0, sizeof(uint32_t), st));
            // (the sweep reads whole slot groups of 1, 2, 4, 8 right-hand sides: the slots beyond R carry zeros)
            const size_t bp = ws.dims.b_pad;
            HIPCHK(hipMemsetAsync(ws.rhs, 0, 2 * bp * ldm * sizeof(T), st));

            // c = A^T y of every slot in one pass (the slots' y rows are the right-hand sides), first picks
            uint32_t nparts = 0;
            HIPCHK(launch_ro_sweep<T>(ctx, ws.y, 0, ws.c, 0, ws.dims.n_pad, 1, R, ws.pmax_val, ws.pmax_idx, ws.dims.pmax_stride, &nparts,
                                      ws.st, false));
            HIPCHK(launch_ro_init<T>(ctx, ws, R, nparts, tol));
            const uint32_t L = (uint32_t)std::max(1, std::min(ctx->lookahead, 64));
            const uint64_t last_round = (uint64_t)max_iter + 1;
            for (uint64_t round = 1; round <= last_round; ++round) {
                if (!wait_round(ctx, round, L, "hipStreamQuery(reference-order batch loop)")) break;
                HIPCHK(launch_ro_round<T>(ctx, ws, R, (uint32_t)round, nparts, tol, max_iter));
            }
            hs.resize(R);
            HIPCHK(hipMemcpyAsync(hs.data(), ws.st, (size_t)R * sizeof(DevState), hipMemcpyDeviceToHost, st));
            if (c.rec_out) {
                const size_t rb = record_bytes(c.kmax, sizeof(T));
                const unsigned char* stage = pack_records<T>(ctx, ws, R, c.kmax);
                for (uint32_t b = 0; b < R; ++b) HIPCHK(hipMemcpyAsync(c.rec(gidx(b)), stage + (size_t)b * rb, rb, hipMemcpyDefault, st));
            }
            if (c.X)
                for (uint32_t b = 0; b < R; ++b) copy_out<T>(ctx, c.x(gidx(b)), c.incx, ws.x + (size_t)b * np, n);
            HIPCHK(hipStreamSynchronize(st));
            if (want_trace != 0u && ws.trace) fetch_trace(ctx, ws, hs[0].iter);
            for (uint32_t b = 0; b < R; ++b) {
                if (const int rc = check_slot_status(hs[b], c.err, c.errlen)) return rc;
                c.report(gidx(b), hs[b].iter, hs[b].c_inf);
                ctx->stats.iterations += hs[b].iter;
                ctx->stats.ro_resweeps += hs[b].nsweeps;
            }
            ctx->stats.solves += R;
        }
        return SS_HIP_OK;
    });
}

// form: 0 = two GEMMs per round (residual form), 1 = Gram form on the full G = A^T A — the correlations of every signal come from
// rows of G (c = c0 - sum_j x_j G[j], q = sum_j d_j G[j]) instead of two GEMMs per round —, 2 = column form: Gram form on a cache
// of the entering columns' Gram columns, formed round by round (mid-size batches, no G), 3 = screened form (screen.hip): c0 by the
// batch GEMM, one workgroup per signal on its subset's own Gram matrix, one screening launch per chunk
int solve_batch_gemm_f32(ss_hip_ctx* ctx, const BatchCall<float>& c, int form = 0, bool no_subset = false)
{
    using T = float;
    const bool gram = form != 0, cols_form = form == 2;
    const size_t B = c.B;
    const T tol = c.tol;
    const uint32_t max_iter = c.max_iter;
    return guarded_rt(c.err, c.errlen, "solve_batch", [&]() -> int {
        HIPCHK(hipSetDevice(ctx->device));
        const size_t m = ctx->m, n = ctx->n, ldm = ctx->ldm, np = ctx->n_pad;
        const uint32_t kcap = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(n, (uint64_t)max_iter + 1), kKcapLimit);
        // (column form: chunks of at most 448 signals = 7 full passes per round, fewer if the cache budget says so)
        const bool scr_form = form == 3;
        const size_t chunk = scr_form ? (size_t)screen_batch_cap()
                                      : cols_form ? (size_t)std::max(1, ctx->bcol_chunk) : (size_t)std::max(4, ctx->batch_chunk);
        hipStream_t st = ctx->stream;
        std::vector<DevState> hs;
        std::vector<size_t> all_ties;                        // signals whose scan met a tie stall, over all chunks
        std::vector<size_t> redo;                            // subset form: signals it declined or whose check failed
        for (size_t b0 = 0; b0 < B; b0 += chunk) {
            const uint32_t Bc = (uint32_t)std::min(chunk, B - b0);
            ensure_workspace<T>(ctx, Bc, kcap);
            Workspace<T>& ws = *ws_of<T>(ctx);
            // option "trace": the path of the batch's FIRST signal (slot 0 of the first chunk) is recorded like a single solve's
            const uint32_t want_trace = (ctx->tracing && b0 == 0) ? (uint32_t)std::min<uint64_t>((uint64_t)max_iter + 2, 1u << 20) : 0u;
            TraceWindow<T> trace_window(ws, want_trace);
            const uint32_t rows = (Bc + 127u) / 128u * 128u;          // GEMM rows of each block
            const size_t bp = ws.dims.b_pad;
            T* const Rblk = ws.rhs;
            T* const Pblk = ws.rhs + bp * ldm;

            ctx->host_flags[0] = 0;
            ctx->host_flags[1] = 0;
            upload_chunk<T>(ctx, ws, c, b0, Bc);
            uint32_t nparts = begin_gemm_chunk(ctx, ws, Bc, tol, ctx->profiling != 0);
            bool gram_chunk = gram;
            if (gram_chunk && ctx->engine == 1) {
                // the tolerance guard of engine 1, for every signal of the chunk at once
                ctx->host_flags[4] = 0;
                HIPCHK(launch_gram_guard_batched<T>(ctx, ws, Bc, tol));
                HIPCHK(hipStreamSynchronize(st));
                if (ctx->host_flags[4] != 0) { gram_chunk = false; ctx->stats.gram_fallbacks += 1; }
            }
            if (gram_chunk) {
                // keep c0 = A^T y of every signal: the Gram-form rounds subtract from it
                grow_device(ctx->own, ctx->c0_batch, ctx->c0_batch_rows, bp, np * sizeof(T), "hipMalloc(c0_batch)");
                HIPCHK(hipMemcpyAsync(ctx->c0_batch, ws.c, (size_t)Bc * np * sizeof(T), hipMemcpyDeviceToDevice, st));
            } else {
                HIPCHK(launch_rp<T>(ctx, ws, Bc));
            }
            BatchCols bc;
            const bool cols_chunk = gram_chunk && cols_form;
            if (cols_chunk) {
                // one cache row per slot and round (round 0 = the first pick), a row table per slot, the pass lists:
                // sized by the dispatcher (ensure_bcol), which sends the batch another way when they do not fit
                const size_t rows_needed = ((size_t)max_iter + 2) * Bc;
                const size_t pitchc = (np + 1023) / 1024 * 1024;          // (k_la_cq reads whole 1024-column chunks of a row)
                if (ctx->bcol_cache_rows < rows_needed || ctx->bcol_slot_rows < Bc || !ctx->bcol_lists)
                    throw HipFail{ hipErrorOutOfMemory, "column form: cache not sized for this chunk" };
                bc.pitch = (uint32_t)pitchc;
                HIPCHK(hipMemsetAsync(ctx->bcol_slot, 0xff, (size_t)Bc * np * sizeof(int32_t), st));
                bc.cache = ctx->bcol_cache;
                bc.bslot = ctx->bcol_slot;
                bc.rcols = ctx->bcol_lists;
                bc.drows = ctx->bcol_lists + 1024;
                bc.cap = (Bc + 63u) / 64u * 64u;
                bc.row_base = 0;
                HIPCHK(launch_batch_cols(ctx, ws.st, Bc, 0, true, bc.bslot, bc.rcols, bc.drows, bc.cap));
                HIPCHK(launch_batch_passes(ctx, &bc, Bc));
                ctx->stats.batch_col_rounds += 1;
            }
            const T* const Gsrc = cols_chunk ? bc.cache : ctx->gram_full;
            const uint32_t Gpitch = cols_chunk ? bc.pitch : ctx->gram_pitch;

            // Subset form (subbatch.hip): with G at hand every signal is solved by one workgroup on the 448 columns with the
            // largest |c0| and then checked against all columns — 16.8 MB of G per signal instead of 545
            bool sub_chunk = gram_chunk && form == 1 && !no_subset && ctx->batch_subset && ctx->gram_full != nullptr && sub_form_usable(ctx);
            if (sub_chunk && ctx->sub_off_chunks > 0) { ctx->sub_off_chunks -= 1; sub_chunk = false; }     // (it handed back too much lately)
            const bool scr_chunk = gram_chunk && scr_form && !no_subset;
            // (a chunk whose tolerance is too tight for Gram-form correlations runs the residual-form rounds below, as in every form)
            if ((sub_chunk || scr_chunk) && try_grow_device(ctx->own, ctx->sub_buf, ctx->sub_buf_bytes, sub_buffer_bytes(Bc), 1) != hipSuccess) {
                // (the subset form steps aside for this chunk; the screened form has no other way to go)
                (void)hipGetLastError();
                sub_chunk = false;
                if (scr_chunk) throw HipFail{ hipErrorOutOfMemory, "screened batch form: log buffers" };
            }
            const uint32_t L = (uint32_t)std::max(1, std::min(ctx->lookahead, 64));
            const uint64_t last_round = (uint64_t)max_iter + 1;
            uint64_t rounds_run = 0;
            size_t ncq = 0;                                  // timed k_la_cq launches of this chunk (profiling on)
            if (sub_chunk) {
                const bool timed = ctx->profiling != 0;
                EventPair ev;
                hipEvent_t verified = nullptr;
                if (timed) { ev = { prof_event(ctx, 0), prof_event(ctx, 1) }; verified = prof_event(ctx, 2); if (!ctx->ev_sub_sel) HELD(ctx->own, hipEventCreate, &ctx->ev_sub_sel); }
                HIPCHK(launch_sub_form(ctx, ws, Bc, ctx->c0_batch, tol, max_iter, ev, verified));
                if (timed) {
                    HIPCHK(hipEventSynchronize(verified));
                    float ms = 0.f;
                    HIPCHK(hipEventElapsedTime(&ms, ev.a, ev.b)); ctx->stats.sub_solve_ms += ms;
                    if (std::getenv("SS_HIP_SUB_DEBUG")) { float ms2 = 0.f; HIPCHK(hipEventElapsedTime(&ms2, ev.a, ctx->ev_sub_sel)); std::fprintf(stderr, "[subset form] select %.3f ms, solve %.3f ms\n", ms2, ms - ms2); }
                    HIPCHK(hipEventElapsedTime(&ms, ev.b, verified)); ctx->stats.sub_verify_ms += ms;
                    HIPCHK(hipEventElapsedTime(&ms, ctx->ev_c0a, ctx->ev_c0b));
                    ctx->stats.c0_gemm_ms += ms;
                    ctx->stats.c0_gemm_flops += 2.0 * (double)rows * (double)ldm * (double)np;
                }
            }
            if (scr_chunk) HIPCHK(launch_screen_batch(ctx, ws, Bc, ctx->c0_batch, tol, max_iter));
            for (uint64_t round = 1; round <= last_round && !sub_chunk && !scr_chunk; ++round) {
                if (!wait_round(ctx, round, L, "hipStreamQuery(batch loop)")) break;
                if (gram_chunk) {
                    const bool timed_cq = ctx->profiling != 0 && ncq < 4096;
                    if (timed_cq) HIPCHK(hipEventRecord(prof_event(ctx, 2 * ncq), st));
                    // (fused form: the scan and the pick of this round happen inside the Gram-form pass, k_la_cqs)
                    const bool fused = cqs_usable(ctx, ws.dims.pmin_stride);
                    HIPCHK(launch_cq_gram_batched<T>(ctx, ws, Bc, Gsrc, Gpitch, ctx->c0_batch, &nparts, cols_chunk ? bc.bslot : nullptr,
                                                     fused ? (uint32_t)round : 0u, tol, max_iter));
                    if (timed_cq) { HIPCHK(hipEventRecord(prof_event(ctx, 2 * ncq + 1), st)); ++ncq; }
                    bc.row_base = (uint32_t)(round * Bc);
                    HIPCHK(launch_tail_gram_batched<T>(ctx, ws, Bc, (uint32_t)round, nparts, tol, max_iter,
                                                       Gsrc, Gpitch, cols_chunk ? &bc : nullptr, fused));
                    if (cols_chunk) ctx->stats.batch_col_rounds += 1;
                } else {
                    HIPCHK(launch_tile_list(ctx, ws.st, Bc, rows, ws.tile_skip));
                    HIPCHK(launch_gemm_tn_f32(ctx, Rblk, rows, (uint32_t)ldm, ws.c, (uint32_t)np, ws.tile_skip));
                    HIPCHK(launch_gemm_tn_f32(ctx, Pblk, rows, (uint32_t)ldm, ws.q, (uint32_t)np, ws.tile_skip));
                    HIPCHK(launch_absmax<T>(ctx, ws, Bc, &nparts));
                    HIPCHK(launch_iteration_tail<T>(ctx, ws, Bc, (uint32_t)round, nparts, tol, max_iter));
                }
                ++rounds_run;
            }
            hs.resize(Bc);
            HIPCHK(hipMemcpyAsync(hs.data(), ws.st, (size_t)Bc * sizeof(DevState), hipMemcpyDeviceToHost, st));
            if (c.rec_out) {
                const unsigned char* stage = pack_records<T>(ctx, ws, Bc, c.kmax);
                HIPCHK(hipMemcpyAsync(c.rec(b0), stage, record_bytes(c.kmax, sizeof(T)) * Bc, hipMemcpyDefault, st));
            }
            if (c.X) download_chunk<T>(ctx, ws, c, b0, Bc);
            HIPCHK(hipStreamSynchronize(st));
            if (want_trace != 0u && ws.trace) fetch_trace(ctx, ws, hs[0].iter);
            // The fused scan's meeting of a signal's workgroups is a bounded wait (k_la_cqs): should it ever expire — the
            // workgroups of a signal not resident together — the slot carries SS_HIP_ERUNTIME; this context then goes on with
            // the two-kernel form and the chunk is solved again (nothing of it has been reported yet)
            if (gram && ctx->batch_fused_scan) {
                bool expired = false;
                for (uint32_t b = 0; b < Bc; ++b) expired = expired || hs[b].status == SS_HIP_ERUNTIME;
                if (expired) {
                    ctx->batch_fused_scan = 0;
                    ctx->stats.persist_fallbacks += 1;
                    b0 -= chunk;                                 // (the loop adds it back: unsigned arithmetic)
                    continue;
                }
            }
            std::vector<uint32_t> ties;                      // slots whose scan met a tie stall (DevState::tie_stall)
            uint32_t n_redo_chunk = 0;
            for (uint32_t b = 0; b < Bc; ++b) {
                // (a slot that did not terminate is neither handed on nor a tie: check_slot_status reports it)
                if (hs[b].done && (hs[b].status == kStatusSubsetDecline || hs[b].status == kStatusSubsetFail)) {
                    if (std::getenv("SS_HIP_SUB_DEBUG"))
                        std::fprintf(stderr, "[subset form] signal %zu: status %u after %u iterations, %u breakpoints logged, K = %u, lambda %g\n",
                                     b0 + b, hs[b].status, hs[b].iter, hs[b].solo_nlog, hs[b].K, hs[b].c_inf);
                    redo.push_back(b0 + b);                  // (nothing of it is reported: solved again in the lock-step form below)
                    ++n_redo_chunk;
                    count_reasons(ctx, hs[b].sub_reason, false);     // (why, as the single solves and the OMP / fp64 batches count it)
                    continue;
                }
                if (hs[b].done && ctx->tie_rerun && !ctx->tie_guard && (hs[b].status == kStatusTieRerun || (hs[b].status == 0 && hs[b].tie_stall != 0))) {
                    ties.push_back(b);
                    continue;
                }
                if (const int rc = check_slot_status(hs[b], c.err, c.errlen)) return rc;
                c.report(b0 + b, hs[b].iter, hs[b].c_inf);
                ctx->stats.iterations += hs[b].iter;
            }
            ctx->stats.solves += Bc - (uint32_t)ties.size() - n_redo_chunk;
            if (sub_chunk) {
                ctx->stats.subset_signals += Bc - n_redo_chunk;
                ctx->stats.subset_redone += n_redo_chunk;
                if (Bc >= 16 && 3u * n_redo_chunk > Bc) ctx->sub_off_chunks = 8;
            }
            if (scr_chunk) {
                ctx->stats.screen_signals += Bc - n_redo_chunk - (uint32_t)ties.size();
                ctx->stats.screen_redone += n_redo_chunk;
                // (a context whose signals the form mostly hands back — dense supports — goes the other way for the next 8 batches)
                if (Bc >= 8 && 3u * n_redo_chunk > Bc) ctx->sub_off_chunks = 8;
            }
            ctx->stats.batch_rounds += rounds_run;
            if (ncq != 0) {
                // rounds enqueued behind the end of the batch are no-ops (microseconds): only launches that
                // belong to a round some signal was still running in are counted, with their bytes
                uint32_t live_rounds = 0;
                for (uint32_t b = 0; b < Bc; ++b) live_rounds = std::max(live_rounds, std::min<uint32_t>(hs[b].iter + 1u, max_iter));
                for (size_t i = 0; i < ncq && i < live_rounds; ++i) {
                    float ms = 0.f;
                    HIPCHK(hipEventElapsedTime(&ms, ctx->prof_events[2 * i], ctx->prof_events[2 * i + 1]));
                    ctx->stats.cq_ms += ms;
                    ctx->stats.cq_launches += 1;
                }
                // a signal with `it` iterations is live in rounds 1 .. it + 1 (the last one finds the end); in
                // round r its list holds r columns (one per iteration; removals make this an upper bound)
                uint64_t rows = 0;
                for (uint32_t b = 0; b < Bc; ++b) {
                    const uint64_t r = std::min<uint64_t>(std::min<uint32_t>(hs[b].iter + 1u, max_iter), ncq);
                    rows += r * (r + 1) / 2 + 3 * r;
                }
                ctx->stats.cq_bytes += rows * (uint64_t)n * sizeof(T);
            }
            // Tie stalls: which implementation's rounding derails on an exact tie is luck (homotopy-cpu.cpp:143-153), so
            // these signals are solved again in the reference-order engine — after the last chunk, all of them together
            // (up to 4 share every pass over A: solve_batch_ro).  (A handful per 4096 signals at 8192 x 65536.)
            for (uint32_t b : ties) all_ties.push_back(b0 + b);
        }
        if (scr_form) {
            // screened batch form: what it hands back is solved by the default single-signal engine, one by one
            Route r; r.no_sub = true;                      // (the batch's screened form has declined it: the default engine)
            for (size_t g : redo)
                if (const int rc = solve_alone(ctx, c, g, r)) return rc;
            redo.clear();
        }
        if (!redo.empty()) {
            // the signals the subset form did not vouch for, gathered and solved in the lock-step Gram form (their own ties
            // are arbitrated inside that call), results scattered back
            const size_t nr = redo.size(), rb = record_bytes(c.kmax, sizeof(T));
            T* Yg = nullptr; T* Xg = nullptr; unsigned char* Rg = nullptr;
            Holdings tmp;        // (of this redo alone)
            HELD(tmp, hipMalloc, &Yg, nr * m * sizeof(T));
            if (c.X) HELD(tmp, hipMalloc, &Xg, nr * n * sizeof(T));
            if (c.rec_out) HELD(tmp, hipMalloc, &Rg, nr * rb);
            for (size_t r = 0; r < nr; ++r) copy_in<T>(ctx, Yg + r * m, c.y(redo[r]), c.incy, m);
            HIPCHK(hipStreamSynchronize(st));
            std::vector<uint32_t> it_r(nr, 0u);
            std::vector<double> er_r(nr, 0.0);
            const BatchCall<T> gathered{ Yg, nr, (ptrdiff_t)m, 1, tol, max_iter, Xg, (ptrdiff_t)n, 1, it_r.data(), er_r.data(), c.err, c.errlen, Rg, c.kmax };
            const int rc = solve_batch_gemm_f32(ctx, gathered, form, true);
            if (rc != SS_HIP_OK) return rc;
            for (size_t r = 0; r < nr; ++r) {
                const size_t g = redo[r];
                if (c.X) copy_out<T>(ctx, c.x(g), c.incx, Xg + r * n, n);
                if (c.rec_out) HIPCHK(hipMemcpyAsync(c.rec(g), Rg + r * rb, rb, hipMemcpyDefault, st));
                c.report(g, it_r[r], er_r[r]);
            }
            HIPCHK(hipStreamSynchronize(st));
        }
        if (!all_ties.empty()) {
            ctx->stats.tie_reruns += all_ties.size();
            const int rc = solve_batch_ro<T>(ctx, c, all_ties.data(), all_ties.size());
            if (rc != SS_HIP_OK) return rc;
        }
        return SS_HIP_OK;
    });
}

template <typename T>
int solve_batch_seq(ss_hip_ctx* ctx, const BatchCall<T>& c)
{
    for (size_t b = 0; b < c.B; ++b)
        if (const int rc = solve_alone(ctx, c, b, Route())) return rc;
    return SS_HIP_OK;
}

int solve_batch_dispatch(ss_hip_ctx* ctx, const BatchCall<float>& c)
{
    const size_t B = c.B;
    // reference-order engine: in lock-step, up to 4 signals per pass over A
    if (ctx->engine == 3) return solve_batch_ro<float>(ctx, c, nullptr, B);
    // lock-step MFMA path once enough signals share the matrix (batch_min option, default 192) — or, with G = A^T A already
    // in HBM, from four signals on: the subset form then runs every signal on a workgroup of its own (subbatch.hip)
    const bool have_g = ctx->gram_full != nullptr && ctx->batch_subset && ctx->engine >= 1 && ctx->batch_gram_min > 0;
    gram_reserve_start(ctx, B);
    // (from four: the batch GEMM that forms c0 works on 128 rows at a time — 1.1 ms at 8192 x 65536, three single sweeps)
    const bool lockstep = B >= (size_t)std::max(2, ctx->batch_min) || (have_g && B >= 4);
    int form = 0;
    // Gram form when G = A^T A is at hand, or the batch is large enough to pay for making it
    // (2 m n^2 flops once, against 4 m n flops per signal and round); same tolerance guard as engine 1
    // (where the screened batch form applies, G = A^T A — 0.28 s at 8192 x 65536 — pays later: a one-off batch breaks even at
    // ~1700 signals (5 300 signals/s against 31 000 + the build), a context that keeps receiving batches after ~3000 in all)
    const bool scr_batches = !ctx->gram_full && ctx->batch_screen && ctx->engine >= 1 && ctx->la_fused >= 3 && ctx->early_solo &&
                             ctx->solo_subset == 256 && !ctx->tracing && ctx->sub_off_chunks == 0 && screen_form_usable(ctx);
    const size_t gram_min = scr_batches ? std::max<size_t>((size_t)ctx->batch_gram_min, 1536) : (size_t)ctx->batch_gram_min;
    const bool gram_pays = B >= gram_min || (scr_batches && ctx->batch_signals_seen + B >= 3072 && B >= (size_t)ctx->batch_gram_min);
    ctx->batch_signals_seen += B;
    if (lockstep && ctx->engine >= 1 && ctx->batch_gram_min > 0 && (ctx->gram_full || gram_pays)) {
        const int rc = guarded_rt(c.err, c.errlen, "solve_batch", [&]() -> int {
            HIPCHK(hipSetDevice(ctx->device));
            if (ensure_full_gram(ctx)) form = 1;
            return SS_HIP_OK;
        });
        if (rc != SS_HIP_OK) return rc;
    }
    // screened form for the batches in between (4 .. batch_gram_min - 1 signals, no G; option batch_screen): c0 of a chunk by the
    // batch GEMM, every signal solved by one workgroup on its subset's own Gram matrix, one screening launch per chunk of 64
    if (form == 0 && !ctx->gram_full && ctx->batch_screen && ctx->engine >= 1 && B >= 4 && ctx->la_fused >= 3 && ctx->early_solo &&
        ctx->solo_subset == 256 && !ctx->tracing && screen_form_usable(ctx)) {
        if (ctx->sub_off_chunks > 0) ctx->sub_off_chunks -= 1;      // (it handed back too much lately)
        else form = 3;
    }
    // column form for the batches in between (batch_cols_min signals or more, no G): in lock-step, one pass
    // over A per round and 64 signals forms the Gram columns of the entering columns (half the flops of the two GEMMs
    // of form 0, and one pass serves 64 signals where a single solve spends three on one).  The cache holds one row
    // per slot and round; a budget (option gram_full_gib) it does not fit sends the batch the old way.
    if (form == 0 && !ctx->gram_full && ctx->engine >= 1 && ctx->batch_cols_min > 0 && B >= (size_t)std::max(2, ctx->batch_cols_min) &&
        ctx->n_pad % 256 == 0) {
        // signals per chunk: at most 448 (7 full passes per round), at most what the cache budget AND the free HBM hold
        // (the cache is (max_iter + 2) rows per signal: a large max_iter with many signals does not fit — such a batch
        // goes the old way instead of failing), whole passes
        const double row_bytes = ((double)c.max_iter + 2.0) * (double)((ctx->n_pad + 1023) / 1024 * 1024) * 4.0;
        double budget = (double)ctx->gram_full_gib * 1073741824.0;
        size_t free_b = 0, total_b = 0;
        if (hipSetDevice(ctx->device) == hipSuccess && hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            const double held = (double)ctx->bcol_cache_rows * (double)((ctx->n_pad + 1023) / 1024 * 1024) * 4.0;
            budget = std::min(budget, std::max(0.0, (double)free_b + held - 4.0 * 1073741824.0));
        } else (void)hipGetLastError();
        const double fit = budget / row_bytes;
        size_t per = (size_t)std::min<double>(448.0, std::max(0.0, fit));
        if (per >= B) per = B; else per = per / 64 * 64;
        if ((per >= 64 || (per == B && per > 0)) && ensure_bcol(ctx, per, c.max_iter)) { form = 2; ctx->bcol_chunk = (int)std::max<size_t>(per, 1); }
    }
    if (lockstep || form == 2 || form == 3) return solve_batch_gemm_f32(ctx, c, form);
    return solve_batch_seq<float>(ctx, c);
}

// fp64 batch, resident tier, in chunks of screen64_batch_cap() signals
// (omp: OMP batches — ss_hip_omp_solve_batch_f64 — the same tier with k_res_solve<double, OMP> and OMP's certificate)
int solve_batch_res64(ss_hip_ctx* ctx, const BatchCall<double>& c, bool omp = false)
{
    const size_t B = c.B, rb = record_bytes(c.kmax, sizeof(double));
    const uint32_t cap = screen64_batch_cap();
    std::vector<size_t> redo;
    const int rc = guarded_rt(c.err, c.errlen, "solve_batch", [&]() -> int {
        HIPCHK(hipSetDevice(ctx->device));
        const size_t m = ctx->m, n = ctx->n;
        const uint32_t kcap = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(n, (uint64_t)c.max_iter + 1), kKcapLimit);
        std::vector<DevState> hst(cap);
        for (size_t b0 = 0; b0 < B; b0 += cap) {
            const uint32_t nb = (uint32_t)std::min<size_t>(cap, B - b0);
            ensure_workspace<double>(ctx, cap, kcap);
            Workspace<double>& ws = *ws_of<double>(ctx);
            hipStream_t st = ctx->stream;
            HIPCHK(hipMemsetAsync(ws.y, 0, (size_t)cap * ctx->ldm * sizeof(double), st));
            for (uint32_t b = 0; b < nb; ++b) copy_in<double>(ctx, ws.y + (size_t)b * ctx->ldm, c.y(b0 + b), c.incy, m);
            HIPCHK(hipMemsetAsync(ws.x, 0, (size_t)nb * ctx->n_pad * sizeof(double), st));
            HIPCHK(hipMemsetAsync(ws.st, 0, (size_t)nb * sizeof(DevState), st));
            HIPCHK(launch_screen64_batch(ctx, ws, nb, c.tol, c.max_iter, omp));
            const unsigned char* stage = c.rec_out ? pack_records<double>(ctx, ws, nb, c.kmax) : nullptr;
            HIPCHK(hipMemcpyAsync(hst.data(), ws.st, (size_t)nb * sizeof(DevState), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            for (uint32_t b = 0; b < nb; ++b) {
                const DevState& hs = hst[b];
                const bool good = hs.done && hs.status == 0 && hs.tie_stall == 0;
                if (!good) {
                    redo.push_back(b0 + b);
                    ctx->stats.screen_tier2 += 1;
                    if (omp) ctx->stats.omp_batch_redone += 1;
                    count_reasons(ctx, hs.sub_reason, hs.tie_stall != 0 || hs.status == kStatusTieRerun);
                    continue;
                }
                if (c.X) copy_out<double>(ctx, c.x(b0 + b), c.incx, ws.x + (size_t)b * ctx->n_pad, n);
                if (c.rec_out) HIPCHK(hipMemcpyAsync(c.rec(b0 + b), stage + (size_t)b * rb, rb, hipMemcpyDefault, st));
                c.report(b0 + b, hs.iter, hs.c_inf);
                ctx->stats.solves += 1;
                ctx->stats.iterations += hs.iter;
                ctx->stats.screen_signals += 1;
                ctx->stats.screen_resident += 1;
                if (omp) ctx->stats.omp_batch_signals += 1;
            }
            HIPCHK(hipStreamSynchronize(st));
        }
        return SS_HIP_OK;
    });
    if (rc != SS_HIP_OK) return rc;
    // what the chunks did not report: alone, through the sub-dictionary tier and the engine behind it
    Route r; r.no_res = true; r.omp = omp;             // (the batch's resident tier has declined it: the tiers behind)
    for (size_t g : redo)
        if (const int rc1 = solve_alone(ctx, c, g, r)) return rc1;
    return SS_HIP_OK;
}

int solve_batch_dispatch(ss_hip_ctx* ctx, const BatchCall<double>& c)
{
    // reference-order engine: in lock-step, up to 4 signals per pass over A
    if (ctx->engine == 3) return solve_batch_ro<double>(ctx, c, nullptr, c.B);
    // fp64 batches of four signals or more on dictionaries the fp64 screened form takes: the resident tier with the signals of a chunk
    // side by side (screen.hip: launch_screen64_batch) — one pass over the fp16 copy ranks every signal's columns, the paths run in as
    // many workgroups at once, every signal's states are certified by a screening pass of its own; what a slot's certificate does not
    // cover is solved again alone, through the remaining tiers
    if (c.B >= 4 && !ctx->tracing && ctx->engine >= 1 && ctx->la_fused >= 1 && ctx->screen_resident && ctx->sub_aside.off == 0 && ctx->res_aside.off == 0) {
        bool usable = false;
        try { HIPCHK(hipSetDevice(ctx->device)); usable = screen64_batch_usable(ctx); } catch (const HipFail&) { usable = false; }
        if (usable) return solve_batch_res64(ctx, c);
    }
    // otherwise one signal at a time
    return solve_batch_seq<double>(ctx, c);
}

template <typename T>
int solve_batch_impl(ss_hip_ctx* ctx, const T* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, T tol,
                     uint32_t max_iter, T* X, ptrdiff_t x_stride, ptrdiff_t incx, uint32_t* iter_out,
                     double* err_out, char* err, size_t errlen, void* rec_out = nullptr, uint32_t kmax = 0)
{
    const BatchCall<T> c{ Y, B, y_stride, incy, tol, max_iter, X, x_stride, incx, iter_out, err_out, err, errlen, rec_out, kmax };
    const int rc = check_batch_call(ctx, c);
    if (rc != SS_HIP_OK || B == 0) return rc;
    return solve_batch_dispatch(ctx, c);
}

// ---- OMP batches (ss_hip_omp_solve_batch_*) --------------------------------------------------------------------------------
// Signal b's result is what ss_hip_omp_solve_* returns for it alone (the same picks, support and iteration count; coefficients to
// rounding).  A slot a chunk does not certify is solved again alone by the single-signal ladder, and nothing of it is written
// before: its result is that ladder's bit for bit.
// sig: the `count` signals' indices into the call (nullptr: 0 .. count-1)
template <typename T>
int solve_omp_seq(ss_hip_ctx* ctx, const BatchCall<T>& c, const size_t* sig, size_t count)
{
    Route r; r.omp = true;
    for (size_t i = 0; i < count; ++i)
        if (const int rc = solve_alone(ctx, c, sig ? sig[i] : i, r)) return rc;
    return SS_HIP_OK;
}

// fp32 chunks: c0 of every slot by the batch GEMM, then the Gram form (gram: ompbatch.hip, 256 slots per chunk) or the screened form in
// OMP mode (screen.hip: launch_screen_batch, 64 slots per chunk)
int solve_omp_batch_f32(ss_hip_ctx* ctx, const BatchCall<float>& c, bool gram)
{
    using T = float;
    const size_t B = c.B, rb = record_bytes(c.kmax, sizeof(T));
    const T tol = c.tol;
    const uint32_t max_iter = c.max_iter;
    std::vector<size_t> redo;
    const int rc = guarded_rt(c.err, c.errlen, "solve_batch", [&]() -> int {
        HIPCHK(hipSetDevice(ctx->device));
        const size_t n = ctx->n, ldm = ctx->ldm, np = ctx->n_pad;
        const uint32_t kcap = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(n, (uint64_t)max_iter + 1), kKcapLimit);
        const size_t chunk = gram ? (size_t)omp_gram_cap() : (size_t)screen_batch_cap();
        hipStream_t st = ctx->stream;
        std::vector<DevState> hs;
        for (size_t b0 = 0; b0 < B; b0 += chunk) {
            const uint32_t Bc = (uint32_t)std::min(chunk, B - b0);
            ensure_workspace<T>(ctx, Bc, kcap);
            Workspace<T>& ws = *ws_of<T>(ctx);
            TraceWindow<T> no_trace(ws, 0u);                     // (no trace in these forms)
            HIPCHK(hipMemsetAsync(ws.y, 0, (size_t)Bc * ldm * sizeof(T), st));
            upload_chunk<T>(ctx, ws, c, b0, Bc);
            (void)begin_gemm_chunk(ctx, ws, Bc, tol, false);
            grow_device(ctx->own, ctx->c0_batch, ctx->c0_batch_rows, ws.dims.b_pad, np * sizeof(T), "hipMalloc(c0_batch)");
            HIPCHK(hipMemcpyAsync(ctx->c0_batch, ws.c, (size_t)Bc * np * sizeof(T), hipMemcpyDeviceToDevice, st));
            grow_device(ctx->own, ctx->sub_buf, ctx->sub_buf_bytes, sub_buffer_bytes(Bc), 1, "hipMalloc(sub_buf)");
            if (gram) HIPCHK(launch_omp_gram_batch(ctx, ws, Bc, ctx->c0_batch, tol, max_iter));
            else HIPCHK(launch_screen_batch(ctx, ws, Bc, ctx->c0_batch, tol, max_iter, true));
            hs.resize(Bc);
            HIPCHK(hipMemcpyAsync(hs.data(), ws.st, (size_t)Bc * sizeof(DevState), hipMemcpyDeviceToHost, st));
            const unsigned char* stage = c.rec_out ? pack_records<T>(ctx, ws, Bc, c.kmax) : nullptr;
            HIPCHK(hipStreamSynchronize(st));
            uint32_t certified = 0;
            for (uint32_t b = 0; b < Bc; ++b) certified += (hs[b].done && hs[b].status == 0 && hs[b].tie_stall == 0) ? 1u : 0u;
            // (every slot certified, unit increments: the chunk's rows of X in one copy)
            const bool whole = c.X != nullptr && c.incx == 1 && certified == Bc;
            if (whole) download_chunk<T>(ctx, ws, c, b0, Bc);
            for (uint32_t b = 0; b < Bc; ++b) {
                const bool good = hs[b].done && hs[b].status == 0 && hs[b].tie_stall == 0;
                if (!good) {
                    redo.push_back(b0 + b);                      // (nothing of it is written: solved again alone)
                    count_reasons(ctx, hs[b].sub_reason, hs[b].tie_stall != 0 || hs[b].status == kStatusTieRerun);
                    continue;
                }
                if (c.X && !whole) copy_out<T>(ctx, c.x(b0 + b), c.incx, ws.x + (size_t)b * np, n);
                if (c.rec_out) HIPCHK(hipMemcpyAsync(c.rec(b0 + b), stage + (size_t)b * rb, rb, hipMemcpyDefault, st));
                c.report(b0 + b, hs[b].iter, hs[b].c_inf);
                ctx->stats.solves += 1;
                ctx->stats.iterations += hs[b].iter;
            }
            HIPCHK(hipStreamSynchronize(st));
            ctx->stats.omp_batch_signals += certified;
            ctx->stats.omp_batch_redone += Bc - certified;
            if (gram) {
                ctx->stats.omp_gram_signals += certified;
            } else {
                ctx->stats.screen_signals += certified;
                ctx->stats.screen_resident += certified;
                ctx->stats.screen_redone += Bc - certified;
            }
        }
        return SS_HIP_OK;
    });
    if (rc != SS_HIP_OK) return rc;
    return solve_omp_seq<T>(ctx, c, redo.data(), redo.size());
}

// The forms an OMP batch takes, in this order: (a) fp32 from 4 signals with G = A^T A at hand, or a batch large enough to form it (the
// Homotopy batch's rule: max(batch_gram_min, 1536) where the screened form applies): the Gram form, chunks of 256; (b) fp32 from 4 signals
// on dictionaries the screened form takes ("batch_screen"): chunks of 64 in that form; (c) fp64 from 4 signals: the resident tier's batch;
// (d) everything else one signal at a time through the single-signal ladder.
int omp_batch_dispatch(ss_hip_ctx* ctx, const BatchCall<float>& c)
{
    if (c.B >= 4 && !ctx->tracing && ctx->engine >= 1 && ctx->engine != 3 && ctx->screen_resident) {
        int form = 0;       // 1: (a) the Gram form, 2: (b) the screened form
        const int rc = guarded_rt(c.err, c.errlen, "solve_batch", [&]() -> int {
            HIPCHK(hipSetDevice(ctx->device));
            if (ctx->batch_gram_min > 0 && res_solve_usable<float>()) {
                const bool scr_batches = !ctx->gram_full && ctx->batch_screen && screen_form_usable(ctx);
                const size_t gram_min = scr_batches ? std::max<size_t>((size_t)ctx->batch_gram_min, 1536) : (size_t)ctx->batch_gram_min;
                if ((ctx->gram_full || c.B >= gram_min) && ensure_full_gram(ctx) && omp_gram_usable(ctx)) { form = 1; return SS_HIP_OK; }
            }
            if (ctx->batch_screen && ctx->la_fused >= 3 && ctx->early_solo && ctx->solo_subset == 256 && res_solve_usable<float>() && screen_form_usable(ctx))
                form = 2;
            return SS_HIP_OK;
        });
        if (rc != SS_HIP_OK) return rc;
        if (form != 0) return solve_omp_batch_f32(ctx, c, form == 1);
    }
    return solve_omp_seq<float>(ctx, c, nullptr, c.B);
}

int omp_batch_dispatch(ss_hip_ctx* ctx, const BatchCall<double>& c)
{
    if (c.B >= 4 && !ctx->tracing && ctx->engine >= 1 && ctx->engine != 3 && ctx->la_fused >= 1 && ctx->screen_resident && ctx->sub_aside.off == 0 &&
        ctx->res_aside.off == 0) {
        bool usable = false;
        try { HIPCHK(hipSetDevice(ctx->device)); usable = screen64_batch_usable(ctx); } catch (const HipFail&) { usable = false; }
        if (usable) return solve_batch_res64(ctx, c, true);
    }
    return solve_omp_seq<double>(ctx, c, nullptr, c.B);
}

template <typename T>
int omp_batch_impl(ss_hip_ctx* ctx, const T* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, T tol, uint32_t max_iter, T* X, ptrdiff_t x_stride,
                   ptrdiff_t incx, uint32_t* iter_out, double* err_out, char* err, size_t errlen, void* rec_out = nullptr, uint32_t kmax = 0)
{
    const BatchCall<T> c{ Y, B, y_stride, incy, tol, max_iter, X, x_stride, incx, iter_out, err_out, err, errlen, rec_out, kmax };
    const int rc = check_batch_call(ctx, c);
    if (rc != SS_HIP_OK || B == 0) return rc;
    return omp_batch_dispatch(ctx, c);
}

// The timed loop of the measurement hooks, on the context's stream: ev_solve0, `repeats` launches, ev_solve1, the entry point's
// copy-out, ONE synchronisation; *ms_out = the time of one launch.  (`launch` and `copy_out` check their own HIP calls.)
template <typename Launch, typename CopyOut>
void timed_repeats(ss_hip_ctx* ctx, int repeats, float* ms_out, Launch&& launch, CopyOut&& copy_out)
{
    HIPCHK(hipEventRecord(ctx->ev_solve0, ctx->stream));
    for (int i = 0; i < repeats; ++i) launch();
    HIPCHK(hipEventRecord(ctx->ev_solve1, ctx->stream));
    copy_out();
    HIPCHK(hipStreamSynchronize(ctx->stream));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, ctx->ev_solve0, ctx->ev_solve1));
    if (ms_out) *ms_out = ms / (float)repeats;
}

template <typename T>
int gemv_t_impl(ss_hip_ctx* ctx, const T* r, T* c, int repeats, float* ms_out, char* err, size_t errlen)
{
    if (ctx && ctx->kind != 0) { set_err(err, errlen, "this entry point needs a Homotopy context (an IRLS context holds the factorised matrix)"); return SS_HIP_EINVAL; }
    if (!ctx || !r || !c) { set_err(err, errlen, "gemv_t: null argument"); return SS_HIP_EINVAL; }
    if (ctx->is_f64 != (sizeof(T) == 8)) { set_err(err, errlen, "gemv_t: type mismatch"); return SS_HIP_ETYPE; }
    if (repeats < 1) repeats = 1;
    return guarded_rt(err, errlen, "gemv_t", [&]() -> int {
        HIPCHK(hipSetDevice(ctx->device));
        Workspace<T>& ws = *ws_of<T>(ctx);
        hipStream_t st = ctx->stream;
        copy_in<T>(ctx, ws.rhs, r, 1, ctx->m);
        if (ctx->ldm > ctx->m)
            HIPCHK(hipMemsetAsync(ws.rhs + ctx->m, 0, (ctx->ldm - ctx->m) * sizeof(T), st));
        uint32_t nb = 0;
        timed_repeats(ctx, repeats, ms_out, [&] {
            // (option engine = 3: the reference-order sweep, reforder.hip)
            if (ctx->engine == 3) HIPCHK(launch_ro_sweep<T>(ctx, ws.rhs, 0, ws.c, 0, ws.dims.n_pad, 1, 1u, ws.pmax_val, ws.pmax_idx, ws.dims.pmax_stride, &nb, nullptr, false));
            else HIPCHK(launch_sweep<T>(ctx, ws.rhs, 0, 1, ws.c, nullptr, ws.pmax_val, ws.pmax_idx, &nb, nullptr));
        }, [&] { copy_out<T>(ctx, c, 1, ws.c, ctx->n); });
        return SS_HIP_OK;
    });
}

// C[b][:] = A^T R[b][:] for B right-hand sides through the MFMA GEMM (fp32 contexts)
int gemm_t_impl(ss_hip_ctx* ctx, const float* R, size_t B, ptrdiff_t ldR, float* C, ptrdiff_t ldC,
                int repeats, float* ms_out, char* err, size_t errlen)
{
    if (ctx && ctx->kind != 0) { set_err(err, errlen, "this entry point needs a Homotopy context (an IRLS context holds the factorised matrix)"); return SS_HIP_EINVAL; }
    if (!ctx || !R || !C || B == 0) { set_err(err, errlen, "gemm_t: null/empty argument"); return SS_HIP_EINVAL; }
    if (ctx->is_f64) { set_err(err, errlen, "gemm_t: fp32 contexts only"); return SS_HIP_ETYPE; }
    if (repeats < 1) repeats = 1;
    DeviceBuf Dd_buf, Rd_buf;      // (scratch of the call: freed after its synchronisation, Rd first)
    return guarded_rt(err, errlen, "gemm_t", [&]() -> int {
        HIPCHK(hipSetDevice(ctx->device));
        const size_t Bp = (B + 127) / 128 * 128;
        const size_t ldm = ctx->ldm, np = ctx->n_pad;
        Rd_buf.alloc(Bp * ldm * sizeof(float), "hipMalloc(&Rd, Bp * ldm * sizeof(float))");
        Dd_buf.alloc(Bp * np * sizeof(float), "hipMalloc(&Dd, Bp * np * sizeof(float))");
        float *Rd = Rd_buf.get<float>(), *Dd = Dd_buf.get<float>();
        HIPCHK(hipMemsetAsync(Rd, 0, Bp * ldm * sizeof(float), ctx->stream));
        HIPCHK(hipMemcpy2DAsync(Rd, ldm * sizeof(float), R, (size_t)ldR * sizeof(float),
                                ctx->m * sizeof(float), B, hipMemcpyDefault, ctx->stream));
        timed_repeats(ctx, repeats, ms_out, [&] { HIPCHK(launch_gemm_tn_f32(ctx, Rd, (uint32_t)Bp, (uint32_t)ldm, Dd, (uint32_t)np, nullptr)); }, [&] {
            HIPCHK(hipMemcpy2DAsync(C, (size_t)ldC * sizeof(float), Dd, np * sizeof(float),
                                    ctx->n * sizeof(float), B, hipMemcpyDefault, ctx->stream));
        });
        return SS_HIP_OK;
    });
}

// The private pass fields of a context (the tiling and the row split of the fp64 passes: gemm.hip) as a measurement call found them,
// put back when the call leaves — by a return or by a thrown HipFail
struct PassTierGuard {
    ss_hip_ctx* ctx;
    int ksplit, tile128;
    void* part;
    explicit PassTierGuard(ss_hip_ctx* c) : ctx(c), ksplit(c->pass_ksplit), tile128(c->pass_tile128), part(c->pass_part) {}
    PassTierGuard(const PassTierGuard&) = delete;
    PassTierGuard& operator=(const PassTierGuard&) = delete;
    ~PassTierGuard() { ctx->pass_ksplit = ksplit; ctx->pass_tile128 = tile128; ctx->pass_part = part; }
};

// G[s][:] = A^T a_{cols[s]} for up to `max_cols` (32 or 64) columns in one pass: S <= 32 the 32-column pass, more the 64-column
// pass (launch_gemm_first's choice).  tier 0: the context's configuration; fp64 only: 1 = the 128-column tiling of the 32-column
// pass, k >= 2 = the rows split k ways (what the sub-context of the fp64 screened form runs: gemm.hip)
template <typename T>
int gram_cols_impl(ss_hip_ctx* ctx, const uint32_t* cols, size_t S, int tier, T* G, ptrdiff_t ldG, int repeats,
                   float* ms_out, char* err, size_t errlen, size_t max_cols)
{
    if (ctx && ctx->kind != 0) { set_err(err, errlen, "this entry point needs a Homotopy context (an IRLS context holds the factorised matrix)"); return SS_HIP_EINVAL; }
    if (!ctx || !cols || !G || S == 0 || S > max_cols) {
        set_err(err, errlen, max_cols > 32 ? "gram_cols_wide: need 1..64 columns" : "gram_cols: need 1..32 columns");
        return SS_HIP_EINVAL;
    }
    if (ctx->is_f64 != (sizeof(T) == 8)) { set_err(err, errlen, "gram_cols: element type of the call does not match the context"); return SS_HIP_ETYPE; }
    for (size_t s = 0; s < S; ++s)
        if (cols[s] >= ctx->n) { set_err(err, errlen, "gram_cols: column index out of range"); return SS_HIP_EINVAL; }
    if (tier < 0 || (tier != 0 && sizeof(T) != 8)) { set_err(err, errlen, "gram_cols_wide: tier must be 0 (fp64 contexts: 0, 1, or the number of row chunks)"); return SS_HIP_EINVAL; }
    if (tier >= 2 && (ctx->ldm / 16u < (uint32_t)tier || ctx->ldm % (16u * (uint32_t)tier) != 0u)) {
        set_err(err, errlen, "gram_cols_wide: the padded row count " + std::to_string(ctx->ldm) + " does not split into " + std::to_string(tier) +
                             " chunks of whole 16-row steps");
        return SS_HIP_EINVAL;
    }
    if (repeats < 1) repeats = 1;
    DeviceBuf Dd_buf, dlist_buf, part_buf;
    PassTierGuard restore(ctx);
    return guarded_rt(err, errlen, "gram_cols", [&]() -> int {
        HIPCHK(hipSetDevice(ctx->device));
        uint32_t h[128];
        for (int s = 0; s < 64; ++s) {
            h[s] = (size_t)s < S ? cols[s] : 0xffffffffu;
            h[64 + s] = (size_t)s < S ? (uint32_t)s : 0xffffffffu;
        }
        const size_t np = ctx->n_pad;
        const size_t rows = S > 32 ? 64 : 32;
        dlist_buf.alloc(sizeof(h), "hipMalloc(&dlist, sizeof(h))");
        Dd_buf.alloc(rows * np * sizeof(T), "hipMalloc(&Dd, rows * np * sizeof(T))");
        if (tier >= 2) {
            part_buf.alloc((size_t)tier * 64 * np * sizeof(double), "hipMalloc(&part, tier * 64 * np * sizeof(double))");
            ctx->pass_part = part_buf.get<void>();
            ctx->pass_ksplit = tier;
        } else if (tier == 1) {
            ctx->pass_ksplit = 0;
            ctx->pass_tile128 = 1;
        }
        uint32_t* dlist = dlist_buf.get<uint32_t>();
        T* Dd = Dd_buf.get<T>();
        HIPCHK(hipMemcpyAsync(dlist, h, sizeof(h), hipMemcpyHostToDevice, ctx->stream));
        timed_repeats(ctx, repeats, ms_out, [&] { HIPCHK(launch_gemm_first(ctx, (uint32_t)S, dlist, dlist + 64, Dd, (uint32_t)np, nullptr)); }, [&] {
            HIPCHK(hipMemcpy2DAsync(G, (size_t)ldG * sizeof(T), Dd, np * sizeof(T), ctx->n * sizeof(T), S,
                                    hipMemcpyDefault, ctx->stream));
        });
        return SS_HIP_OK;
    });
}

// rows of the context's G = A^T A (formed here if the context has not formed it yet), columns [0, n)
int gram_full_rows_impl(ss_hip_ctx* ctx, const uint32_t* rows, size_t count, float* out, ptrdiff_t ldout, char* err, size_t errlen)
{
    if (ctx && ctx->kind != 0) { set_err(err, errlen, "this entry point needs a Homotopy context (an IRLS context holds the factorised matrix)"); return SS_HIP_EINVAL; }
    if (!ctx || !rows || !out || count == 0) { set_err(err, errlen, "gram_full_rows: null/empty argument"); return SS_HIP_EINVAL; }
    if (ctx->is_f64) { set_err(err, errlen, "gram_full_rows: fp32 contexts only"); return SS_HIP_ETYPE; }
    if (ldout < 0 || (size_t)ldout < ctx->n) { set_err(err, errlen, "gram_full_rows: ldout must be at least n"); return SS_HIP_EINVAL; }
    for (size_t i = 0; i < count; ++i)
        if (rows[i] >= ctx->n) { set_err(err, errlen, "gram_full_rows: row index out of range"); return SS_HIP_EINVAL; }
    return guarded_rt(err, errlen, "gram_full_rows", [&]() -> int {
        HIPCHK(hipSetDevice(ctx->device));
        if (!ensure_full_gram(ctx)) {
            set_err(err, errlen, "gram_full_rows: G = A^T A (" + std::to_string(((size_t)ctx->n_pad * ctx->n_pad * sizeof(float)) >> 20) +
                                 " MiB) does not fit the budget (option gram_full_gib) or the free device memory");
            return SS_HIP_ENOMEM;
        }
        for (size_t i = 0; i < count; ++i)
            HIPCHK(hipMemcpyAsync(out + (ptrdiff_t)i * ldout, ctx->gram_full + (size_t)rows[i] * ctx->gram_pitch, ctx->n * sizeof(float),
                                  hipMemcpyDefault, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        return SS_HIP_OK;
    });
}

int subset_gram_impl(ss_hip_ctx* ctx, const uint32_t* cols, float* Gs, int repeats, float* ms_out, char* err, size_t errlen)
{
    if (ctx && ctx->kind != 0) { set_err(err, errlen, "this entry point needs a Homotopy context (an IRLS context holds the factorised matrix)"); return SS_HIP_EINVAL; }
    if (!ctx || !cols || !Gs) { set_err(err, errlen, "subset_gram: null argument"); return SS_HIP_EINVAL; }
    if (ctx->is_f64) { set_err(err, errlen, "subset_gram: fp32 contexts only"); return SS_HIP_ETYPE; }
    if (repeats < 1) repeats = 1;
    DeviceBuf dG_buf, dcols_buf;
    return guarded_rt(err, errlen, "subset_gram", [&]() -> int {
        HIPCHK(hipSetDevice(ctx->device));
        dcols_buf.alloc(kSoloWidth * sizeof(uint32_t), "hipMalloc(&dcols, kSoloWidth * sizeof(uint32_t))");
        dG_buf.alloc((size_t)kSoloWidth * kSoloWidth * sizeof(float), "hipMalloc(&dG, (size_t)kSoloWidth * kSoloWidth * sizeof(float))");
        uint32_t* dcols = dcols_buf.get<uint32_t>();
        float* dG = dG_buf.get<float>();
        HIPCHK(hipMemcpyAsync(dcols, cols, kSoloWidth * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        timed_repeats(ctx, repeats, ms_out, [&] { HIPCHK(launch_subset_gram_f32(ctx, dcols, dG, nullptr, nullptr, nullptr, 0)); },
                      [&] { HIPCHK(hipMemcpyAsync(Gs, dG, (size_t)kSoloWidth * kSoloWidth * sizeof(float), hipMemcpyDefault, ctx->stream)); });
        return SS_HIP_OK;
    });
}

template <typename T>
int reconstruct_impl(ss_hip_ctx* ctx, const T* x, T* y, char* err, size_t errlen)
{
    if (ctx && ctx->kind != 0) { set_err(err, errlen, "this entry point needs a Homotopy context (an IRLS context holds the factorised matrix)"); return SS_HIP_EINVAL; }
    if (!ctx || !x || !y) { set_err(err, errlen, "reconstruct: null argument"); return SS_HIP_EINVAL; }
    if (ctx->is_f64 != (sizeof(T) == 8)) { set_err(err, errlen, "reconstruct: type mismatch"); return SS_HIP_ETYPE; }
    return guarded_rt(err, errlen, "reconstruct", [&]() -> int {
        HIPCHK(hipSetDevice(ctx->device));
        Workspace<T>& ws = *ws_of<T>(ctx);
        copy_in<T>(ctx, ws.q, x, 1, ctx->n);
        HIPCHK(launch_gemv_n<T>(ctx, ws.q, ws.rhs));
        copy_out<T>(ctx, y, 1, ws.rhs, ctx->m);
        HIPCHK(hipStreamSynchronize(ctx->stream));
        // rhs padding must stay zero for the sweeps: rows >= m were not written
        return SS_HIP_OK;
    });
}


// ---- IRLS (irls.hip): y up, one launch, x and the report down ---------------------------------
template <typename T>
int irls_solve_impl(ss_hip_ctx* ctx, const T* y, ptrdiff_t incy, T tol, uint32_t max_iter, T* x, ptrdiff_t incx,
                    uint32_t* iter_out, double* err_out, int* spd_failure, char* err, size_t errlen)
{
    if (!ctx) { set_err(err, errlen, "irls_solve: null context"); return SS_HIP_EINVAL; }
    if (ctx->kind != 1) { set_err(err, errlen, "irls_solve: this context was not created for IRLS"); return SS_HIP_EINVAL; }
    if (ctx->is_f64 != (sizeof(T) == 8)) {
        set_err(err, errlen, "irls_solve: element type of the call does not match the context");
        return SS_HIP_ETYPE;
    }
    if (!y || !x) { set_err(err, errlen, "irls_solve: y and x must not be null"); return SS_HIP_EINVAL; }
    if (const int rc = check_solve_args<T>("irls_solve", max_iter, tol, false, incy, incx, err, errlen)) return rc;
    return guarded_rt(err, errlen, "irls_solve", [&]() -> int {
        HIPCHK(hipSetDevice(ctx->device));
        copy_in<T>(ctx, irls_y_buffer<T>(ctx), y, incy, ctx->m);
        IrlsResult res{};
        HIPCHK(irls_solve<T>(ctx, tol, max_iter, &res));
        copy_out<T>(ctx, x, incx, irls_x_buffer<T>(ctx), ctx->n);
        HIPCHK(hipStreamSynchronize(ctx->stream));
        if (iter_out) *iter_out = res.iter;
        if (err_out) *err_out = res.solution_error;
        if (spd_failure) *spd_failure = (int)res.spd_failure;
        ctx->stats.solves += 1;
        ctx->stats.iterations += res.iter;
        return SS_HIP_OK;
    });
}

// ---- IRLS batches (irlsbatch.hip): chunks of slots, each signal's words those of irls_solve_impl for it alone ----------
template <typename T>
int irls_batch_impl(ss_hip_ctx* ctx, const T* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, T tol, uint32_t max_iter,
                    T* X, ptrdiff_t x_stride, ptrdiff_t incx, uint32_t* iter_out, double* err_out, int* spd_failure,
                    char* err, size_t errlen)
{
    // (the single solve's checks, in its order)
    if (!ctx) { set_err(err, errlen, "irls_solve_batch: null context"); return SS_HIP_EINVAL; }
    if (ctx->kind != 1) { set_err(err, errlen, "irls_solve_batch: this context was not created for IRLS"); return SS_HIP_EINVAL; }
    if (ctx->is_f64 != (sizeof(T) == 8)) {
        set_err(err, errlen, "irls_solve_batch: element type of the call does not match the context");
        return SS_HIP_ETYPE;
    }
    if (!Y || !X) { set_err(err, errlen, "irls_solve_batch: Y and X must not be null"); return SS_HIP_EINVAL; }
    if (const int rc = check_solve_args<T>("irls_solve_batch", max_iter, tol, false, incy, incx, err, errlen)) return rc;
    if (B == 0) return SS_HIP_OK;
    return guarded_rt(err, errlen, "irls_solve_batch", [&]() -> int {
        HIPCHK(hipSetDevice(ctx->device));
        uint32_t chunk = 0;
        HIPCHK(irls_batch_reserve<T>(ctx, B, &chunk));
        const T *Qt, *R, *G0;
        irls_factors<T>(ctx, &Qt, &R, &G0);
        std::vector<IrlsResult> res(chunk);
        for (size_t b0 = 0; b0 < B; b0 += chunk) {
            const uint32_t nb = (uint32_t)std::min<size_t>(chunk, B - b0);
            for (uint32_t b = 0; b < nb; ++b)
                copy_in<T>(ctx, irls_batch_y<T>(ctx, b), Y + (ptrdiff_t)(b0 + b) * y_stride, incy, ctx->m);
            uint64_t rounds = 0;
            HIPCHK(irls_batch_run<T>(ctx, Qt, R, G0, nb, tol, max_iter, res.data(), &rounds));
            for (uint32_t b = 0; b < nb; ++b)
                copy_out<T>(ctx, X + (ptrdiff_t)(b0 + b) * x_stride, incx, irls_batch_x<T>(ctx, b), ctx->n);
            HIPCHK(hipStreamSynchronize(ctx->stream));
            for (uint32_t b = 0; b < nb; ++b) {
                if (iter_out) iter_out[b0 + b] = res[b].iter;
                if (err_out) err_out[b0 + b] = res[b].solution_error;
                if (spd_failure) spd_failure[b0 + b] = (int)res[b].spd_failure;
                ctx->stats.iterations += res[b].iter;
            }
            ctx->stats.solves += nb;
            ctx->stats.irls_batch_signals += nb;
            ctx->stats.irls_batch_rounds += rounds;
        }
        return SS_HIP_OK;
    });
}

}  // namespace

// ---- C-ABI ----------------------------------------------------------------------------

extern "C" {

int ss_hip_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

const char* ss_hip_version(void) { return "0.1.0"; }

ss_hip_ctx* ss_hip_homotopy_create_f32(const float* A, size_t m, size_t n, ptrdiff_t stride_row,
                                       ptrdiff_t stride_col, int device, char* err, size_t errlen)
{
    return create_impl<float>(A, m, n, stride_row, stride_col, device, err, errlen);
}

ss_hip_ctx* ss_hip_homotopy_create_f64(const double* A, size_t m, size_t n, ptrdiff_t stride_row,
                                       ptrdiff_t stride_col, int device, char* err, size_t errlen)
{
    return create_impl<double>(A, m, n, stride_row, stride_col, device, err, errlen);
}

ss_hip_ctx* ss_hip_irls_create_f32(const float* A, size_t m, size_t n, ptrdiff_t stride_row, ptrdiff_t stride_col,
                                   int device, char* err, size_t errlen)
{
    return create_impl<float>(A, m, n, stride_row, stride_col, device, err, errlen, 1);
}

ss_hip_ctx* ss_hip_irls_create_f64(const double* A, size_t m, size_t n, ptrdiff_t stride_row, ptrdiff_t stride_col,
                                   int device, char* err, size_t errlen)
{
    return create_impl<double>(A, m, n, stride_row, stride_col, device, err, errlen, 1);
}

int ss_hip_irls_solve_f32(ss_hip_ctx* ctx, const float* y, ptrdiff_t incy, float tol, uint32_t max_iter, float* x,
                          ptrdiff_t incx, uint32_t* iter_out, double* err_out, int* spd_failure, char* err, size_t errlen)
{
    return irls_solve_impl<float>(ctx, y, incy, tol, max_iter, x, incx, iter_out, err_out, spd_failure, err, errlen);
}

int ss_hip_irls_solve_f64(ss_hip_ctx* ctx, const double* y, ptrdiff_t incy, double tol, uint32_t max_iter, double* x,
                          ptrdiff_t incx, uint32_t* iter_out, double* err_out, int* spd_failure, char* err, size_t errlen)
{
    return irls_solve_impl<double>(ctx, y, incy, tol, max_iter, x, incx, iter_out, err_out, spd_failure, err, errlen);
}

int ss_hip_irls_solve_batch_f32(ss_hip_ctx* ctx, const float* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, float tol,
                                uint32_t max_iter, float* X, ptrdiff_t x_stride, ptrdiff_t incx, uint32_t* iter_out,
                                double* err_out, int* spd_failure_out, char* err, size_t errlen)
{
    return irls_batch_impl<float>(ctx, Y, B, y_stride, incy, tol, max_iter, X, x_stride, incx, iter_out, err_out, spd_failure_out,
                                  err, errlen);
}

int ss_hip_irls_solve_batch_f64(ss_hip_ctx* ctx, const double* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, double tol,
                                uint32_t max_iter, double* X, ptrdiff_t x_stride, ptrdiff_t incx, uint32_t* iter_out,
                                double* err_out, int* spd_failure_out, char* err, size_t errlen)
{
    return irls_batch_impl<double>(ctx, Y, B, y_stride, incy, tol, max_iter, X, x_stride, incx, iter_out, err_out, spd_failure_out,
                                   err, errlen);
}

void ss_hip_irls_destroy(ss_hip_ctx* ctx) { ss_hip_homotopy_destroy(ctx); }

void ss_hip_homotopy_destroy(ss_hip_ctx* ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream4) (void)hipStreamSynchronize(ctx->stream4);
    if (ctx->stream3) (void)hipStreamSynchronize(ctx->stream3);
    if (ctx->stream2) (void)hipStreamSynchronize(ctx->stream2);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    gram_reserve_join(ctx);
    delete ctx;       // the parts, then the context's own memory, events and streams (ss_hip_internal.h: the order of ss_hip_ctx's members)
}

int ss_hip_homotopy_solve_f32(ss_hip_ctx* ctx, const float* y, ptrdiff_t incy, float tol,
                              uint32_t max_iter, float* x, ptrdiff_t incx, uint32_t* iter_out,
                              double* err_out, char* err, size_t errlen)
{
    return solve_impl<float>(ctx, y, incy, tol, max_iter, x, incx, iter_out, err_out, err, errlen);
}

int ss_hip_homotopy_solve_f64(ss_hip_ctx* ctx, const double* y, ptrdiff_t incy, double tol,
                              uint32_t max_iter, double* x, ptrdiff_t incx, uint32_t* iter_out,
                              double* err_out, char* err, size_t errlen)
{
    return solve_impl<double>(ctx, y, incy, tol, max_iter, x, incx, iter_out, err_out, err, errlen);
}

int ss_hip_omp_solve_f32(ss_hip_ctx* ctx, const float* y, ptrdiff_t incy, float tol, uint32_t max_iter,
                         float* x, ptrdiff_t incx, uint32_t* iter_out, double* err_out, char* err, size_t errlen)
{
    Route r; r.omp = true;
    return solve_impl<float>(ctx, y, incy, tol, max_iter, x, incx, iter_out, err_out, err, errlen, r);
}

int ss_hip_omp_solve_f64(ss_hip_ctx* ctx, const double* y, ptrdiff_t incy, double tol, uint32_t max_iter,
                         double* x, ptrdiff_t incx, uint32_t* iter_out, double* err_out, char* err, size_t errlen)
{
    Route r; r.omp = true;
    return solve_impl<double>(ctx, y, incy, tol, max_iter, x, incx, iter_out, err_out, err, errlen, r);
}

int ss_hip_homotopy_solve_batch_f32(ss_hip_ctx* ctx, const float* Y, size_t B, ptrdiff_t y_stride,
                                    ptrdiff_t incy, float tol, uint32_t max_iter, float* X,
                                    ptrdiff_t x_stride, ptrdiff_t incx, uint32_t* iter_out,
                                    double* err_out, char* err, size_t errlen)
{
    return solve_batch_impl<float>(ctx, Y, B, y_stride, incy, tol, max_iter, X, x_stride, incx,
                                   iter_out, err_out, err, errlen);
}

int ss_hip_homotopy_solve_batch_f64(ss_hip_ctx* ctx, const double* Y, size_t B, ptrdiff_t y_stride,
                                    ptrdiff_t incy, double tol, uint32_t max_iter, double* X,
                                    ptrdiff_t x_stride, ptrdiff_t incx, uint32_t* iter_out,
                                    double* err_out, char* err, size_t errlen)
{
    return solve_batch_impl<double>(ctx, Y, B, y_stride, incy, tol, max_iter, X, x_stride, incx,
                                    iter_out, err_out, err, errlen);
}

int ss_hip_omp_solve_batch_f32(ss_hip_ctx* ctx, const float* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, float tol, uint32_t max_iter,
                               float* X, ptrdiff_t x_stride, ptrdiff_t incx, uint32_t* iter_out, double* err_out, char* err, size_t errlen)
{
    return omp_batch_impl<float>(ctx, Y, B, y_stride, incy, tol, max_iter, X, x_stride, incx, iter_out, err_out, err, errlen);
}

int ss_hip_omp_solve_batch_f64(ss_hip_ctx* ctx, const double* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, double tol, uint32_t max_iter,
                               double* X, ptrdiff_t x_stride, ptrdiff_t incx, uint32_t* iter_out, double* err_out, char* err, size_t errlen)
{
    return omp_batch_impl<double>(ctx, Y, B, y_stride, incy, tol, max_iter, X, x_stride, incx, iter_out, err_out, err, errlen);
}

size_t ss_hip_record_bytes(uint32_t kmax, int is_f64) { return record_bytes(kmax, is_f64 ? 8 : 4); }

int ss_hip_omp_solve_batch_compact_f32(ss_hip_ctx* ctx, const float* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy,
                                       float tol, uint32_t max_iter, uint32_t kmax, void* records, char* err, size_t errlen)
{
    if (!records) { set_err(err, errlen, "solve_batch_compact: records must not be null"); return SS_HIP_EINVAL; }
    return omp_batch_impl<float>(ctx, Y, B, y_stride, incy, tol, max_iter, nullptr, 0, 1, nullptr, nullptr, err, errlen, records, kmax);
}

int ss_hip_omp_solve_batch_compact_f64(ss_hip_ctx* ctx, const double* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy,
                                       double tol, uint32_t max_iter, uint32_t kmax, void* records, char* err, size_t errlen)
{
    if (!records) { set_err(err, errlen, "solve_batch_compact: records must not be null"); return SS_HIP_EINVAL; }
    return omp_batch_impl<double>(ctx, Y, B, y_stride, incy, tol, max_iter, nullptr, 0, 1, nullptr, nullptr, err, errlen, records, kmax);
}

int ss_hip_homotopy_solve_batch_compact_f32(ss_hip_ctx* ctx, const float* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy,
                                            float tol, uint32_t max_iter, uint32_t kmax, void* records, char* err, size_t errlen)
{
    if (!records) { set_err(err, errlen, "solve_batch_compact: records must not be null"); return SS_HIP_EINVAL; }
    return solve_batch_impl<float>(ctx, Y, B, y_stride, incy, tol, max_iter, nullptr, 0, 1, nullptr, nullptr, err, errlen, records, kmax);
}

int ss_hip_homotopy_solve_batch_compact_f64(ss_hip_ctx* ctx, const double* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy,
                                            double tol, uint32_t max_iter, uint32_t kmax, void* records, char* err, size_t errlen)
{
    if (!records) { set_err(err, errlen, "solve_batch_compact: records must not be null"); return SS_HIP_EINVAL; }
    return solve_batch_impl<double>(ctx, Y, B, y_stride, incy, tol, max_iter, nullptr, 0, 1, nullptr, nullptr, err, errlen, records, kmax);
}

int ss_hip_gemv_t_f32(ss_hip_ctx* ctx, const float* r, float* c, int repeats, float* ms_out,
                      char* err, size_t errlen)
{
    return gemv_t_impl<float>(ctx, r, c, repeats, ms_out, err, errlen);
}

int ss_hip_gemv_t_f64(ss_hip_ctx* ctx, const double* r, double* c, int repeats, float* ms_out,
                      char* err, size_t errlen)
{
    return gemv_t_impl<double>(ctx, r, c, repeats, ms_out, err, errlen);
}

int ss_hip_gemm_t_f32(ss_hip_ctx* ctx, const float* R, size_t B, ptrdiff_t ldR, float* C, ptrdiff_t ldC,
                      int repeats, float* ms_out, char* err, size_t errlen)
{
    return gemm_t_impl(ctx, R, B, ldR, C, ldC, repeats, ms_out, err, errlen);
}

int ss_hip_gram_cols_f32(ss_hip_ctx* ctx, const uint32_t* cols, size_t S, float* G, ptrdiff_t ldG, int repeats,
                         float* ms_out, char* err, size_t errlen)
{
    return gram_cols_impl<float>(ctx, cols, S, 0, G, ldG, repeats, ms_out, err, errlen, 32);
}

int ss_hip_gram_cols_f64(ss_hip_ctx* ctx, const uint32_t* cols, size_t S, double* G, ptrdiff_t ldG, int repeats,
                         float* ms_out, char* err, size_t errlen)
{
    return gram_cols_impl<double>(ctx, cols, S, 0, G, ldG, repeats, ms_out, err, errlen, 32);
}

int ss_hip_gram_cols_wide_f32(ss_hip_ctx* ctx, const uint32_t* cols, size_t S, int tier, float* G, ptrdiff_t ldG, int repeats,
                              float* ms_out, char* err, size_t errlen)
{
    return gram_cols_impl<float>(ctx, cols, S, tier, G, ldG, repeats, ms_out, err, errlen, 64);
}

int ss_hip_gram_cols_wide_f64(ss_hip_ctx* ctx, const uint32_t* cols, size_t S, int tier, double* G, ptrdiff_t ldG, int repeats,
                              float* ms_out, char* err, size_t errlen)
{
    return gram_cols_impl<double>(ctx, cols, S, tier, G, ldG, repeats, ms_out, err, errlen, 64);
}

int ss_hip_gram_full_rows_f32(ss_hip_ctx* ctx, const uint32_t* rows, size_t count, float* out, ptrdiff_t ldout, char* err, size_t errlen)
{
    return gram_full_rows_impl(ctx, rows, count, out, ldout, err, errlen);
}

int ss_hip_subset_gram_f32(ss_hip_ctx* ctx, const uint32_t* cols, float* Gs, int repeats, float* ms_out, char* err, size_t errlen)
{
    return subset_gram_impl(ctx, cols, Gs, repeats, ms_out, err, errlen);
}

int ss_hip_reconstruct_f32(ss_hip_ctx* ctx, const float* x, float* y, char* err, size_t errlen)
{
    return reconstruct_impl<float>(ctx, x, y, err, errlen);
}

int ss_hip_reconstruct_f64(ss_hip_ctx* ctx, const double* x, double* y, char* err, size_t errlen)
{
    return reconstruct_impl<double>(ctx, x, y, err, errlen);
}

int ss_hip_set_profiling(ss_hip_ctx* ctx, int profiling)
{
    if (!ctx) return SS_HIP_EINVAL;
    ctx->profiling = profiling ? 1 : 0;
    return SS_HIP_OK;
}

int ss_hip_get_stats(ss_hip_ctx* ctx, ss_hip_stats* out)
{
    if (!ctx || !out) return SS_HIP_EINVAL;
    if (ctx->screen != nullptr && ctx->stats.screen_signals + ctx->stats.screen_redone != 0) {
        (void)hipSetDevice(ctx->device);
        ctx->stats.screen_headroom = sship::screen_read_headroom(ctx);
    }
    *out = ctx->stats;
    return SS_HIP_OK;
}

int ss_hip_reset_stats(ss_hip_ctx* ctx)
{
    if (!ctx) return SS_HIP_EINVAL;
    const uint64_t b2 = ctx->stats.sweep_bytes, b1 = ctx->stats.sweep1_bytes, b32 = ctx->stats.sweep32_bytes;
    const uint64_t tc32 = ctx->stats.sweep32_timed_cols;
    const uint64_t b64 = ctx->stats.sweep64_bytes, f64 = ctx->stats.sweep64_flops;
    ctx->stats = ss_hip_stats{};
    ctx->stats.sweep_bytes = b2;
    ctx->stats.sweep1_bytes = b1;
    ctx->stats.sweep32_bytes = b32;
    ctx->stats.sweep32_timed_cols = tc32;
    ctx->stats.sweep64_bytes = b64;
    ctx->stats.sweep64_flops = f64;
    return SS_HIP_OK;
}

// ---- options: one row per key, walked by ss_hip_set_option and ss_hip_get_option (the defaults are the member
// ---- initialisers of ss_hip_ctx; the keys are described in include/ss_hip.h) ----------------------------------------
namespace {

// how a written value is normalised before it is stored
enum class OptNorm {
    AsIs,        // stored as given
    Flag,        // value ? 1 : 0
    Clamp,       // into [lo, hi]
    Floor,       // at least lo
    Snap64,      // value > 32 ? 64 : 32
    Range,       // outside [lo, hi]: SS_HIP_EINVAL, nothing stored
    PassDebug,   // an action, not a member: write-only
};

struct OptRow {
    const char* key;
    int ss_hip_ctx::* i;       // the member: an int ...
    long ss_hip_ctx::* l;      // ... or a long (neither: an action)
    OptNorm norm;
    long lo, hi;
    constexpr OptRow(const char* k, int ss_hip_ctx::* m, OptNorm nm, long lo_ = 0, long hi_ = 0) : key(k), i(m), l(nullptr), norm(nm), lo(lo_), hi(hi_) {}
    constexpr OptRow(const char* k, long ss_hip_ctx::* m, OptNorm nm, long lo_ = 0, long hi_ = 0) : key(k), i(nullptr), l(m), norm(nm), lo(lo_), hi(hi_) {}
    constexpr OptRow(const char* k, OptNorm nm) : key(k), i(nullptr), l(nullptr), norm(nm), lo(0), hi(0) {}
};

// keys added after the rows of the table below were pinned, key for key, by tests/test_gpu_options.py: the same row type, walked by the
// same two entry points, each key covered by the tests of its feature (tc_chunk_max: tests/test_gpu_topcorr.py)
const OptRow kLaterKeys[] = {
    { "tc_chunk_max",          &ss_hip_ctx::tc_chunk_max,          OptNorm::Clamp, 0, 32768 },
};

const OptRow kOptions[] = {
    { "sweep_variant",         &ss_hip_ctx::sweep_variant,         OptNorm::AsIs },
    { "lookahead",             &ss_hip_ctx::lookahead,             OptNorm::AsIs },
    { "strict_sign",           &ss_hip_ctx::strict_sign,           OptNorm::Flag },
    { "screen_first8",         &ss_hip_ctx::screen_first8,         OptNorm::Flag },
    { "screen_rescue",         &ss_hip_ctx::screen_rescue,         OptNorm::Flag },
    { "trace",                 &ss_hip_ctx::tracing,               OptNorm::Flag },
    { "zero_on_removal",       &ss_hip_ctx::zero_on_removal,       OptNorm::Flag },
    { "tie_guard",             &ss_hip_ctx::tie_guard,             OptNorm::Flag },
    { "profile_every",         &ss_hip_ctx::profile_every,         OptNorm::Floor, 1 },
    { "profile_solve_every",   &ss_hip_ctx::profile_solve_every,   OptNorm::Floor, 1 },      // (+ the tick starts again)
    { "engine",                &ss_hip_ctx::engine,                OptNorm::Clamp, 0, 3 },
    { "tie_rerun",             &ss_hip_ctx::tie_rerun,             OptNorm::Flag },
    { "ro_force_resweep",      &ss_hip_ctx::ro_force_resweep,      OptNorm::Flag },
    { "ro_staged",             &ss_hip_ctx::ro_staged,             OptNorm::Flag },
    { "batch_subset",          &ss_hip_ctx::batch_subset,          OptNorm::Flag },
    { "ro_slots",              &ss_hip_ctx::ro_slots,              OptNorm::Range, 1, 8 },
    { "batch_fused_scan",      &ss_hip_ctx::batch_fused_scan,      OptNorm::Flag },
    { "sweep32_variant",       &ss_hip_ctx::sweep32_variant,       OptNorm::Clamp, 0, 9 },
    { "first_sweep_cols",      &ss_hip_ctx::first_sweep_cols,      OptNorm::Snap64 },
    { "early_solo",            &ss_hip_ctx::early_solo,            OptNorm::Flag },
    { "early_pass",            &ss_hip_ctx::early_pass,            OptNorm::AsIs },
    { "early_adapt",           &ss_hip_ctx::early_adapt,           OptNorm::Flag },
    { "early_se",              &ss_hip_ctx::early_se,              OptNorm::Clamp, 0, 3 },
    { "pass_dbg_ptr",          OptNorm::PassDebug },
    { "la_fused",              &ss_hip_ctx::la_fused,              OptNorm::Clamp, 0, 3 },
    { "solo_subset",           &ss_hip_ctx::solo_subset,           OptNorm::Clamp, 0, 256 },
    { "solo_full_gram",        &ss_hip_ctx::solo_full_gram,        OptNorm::Flag },
    { "cache_mib",             &ss_hip_ctx::cache_mib,             OptNorm::Floor, 16 },
    { "batch_min",             &ss_hip_ctx::batch_min,             OptNorm::Floor, 2 },
    { "batch_gram_min",        &ss_hip_ctx::batch_gram_min,        OptNorm::Floor, 0 },
    { "batch_cols_min",        &ss_hip_ctx::batch_cols_min,        OptNorm::Floor, 0 },
    { "gram_full_gib",         &ss_hip_ctx::gram_full_gib,         OptNorm::Floor, 0 },
    { "gram_full_after",       &ss_hip_ctx::gram_full_after,       OptNorm::Floor, 0 },
    { "gram_single",           &ss_hip_ctx::gram_single,           OptNorm::Flag },
    { "gram_symmetric",        &ss_hip_ctx::gram_symmetric,        OptNorm::Flag },
    { "batch_chunk",           &ss_hip_ctx::batch_chunk,           OptNorm::Floor, 4 },
    { "irls_batch_max",        &ss_hip_ctx::irls_batch_max,        OptNorm::Clamp, 1, 65535 },
    { "dl_chunk_max",          &ss_hip_ctx::dl_chunk_max,          OptNorm::Clamp, 0, 32768 },
    { "screen_single",         &ss_hip_ctx::screen_single,         OptNorm::Clamp, 0, 2 },   // (+ the step-aside counters start again)
    { "screen_first16",        &ss_hip_ctx::screen_first16,        OptNorm::Flag },
    { "batch_screen",          &ss_hip_ctx::batch_screen,          OptNorm::Flag },
    { "screen_resident",       &ss_hip_ctx::screen_resident,       OptNorm::Flag },
    { "screen_recheck",        &ss_hip_ctx::screen_recheck,        OptNorm::Flag },
    { "gram_reserve",          &ss_hip_ctx::gram_reserve,          OptNorm::Flag },
    { "colshard_fail_prepare", &ss_hip_ctx::colshard_fail_prepare, OptNorm::Flag },
};

const OptRow* find_option(const char* key)
{
    for (const OptRow& r : kOptions)
        if (!std::strcmp(key, r.key)) return &r;
    for (const OptRow& r : kLaterKeys)
        if (!std::strcmp(key, r.key)) return &r;
    return nullptr;
}

}  // namespace

int ss_hip_set_option(ss_hip_ctx* ctx, const char* key, long value)
{
    if (!ctx || !key) return SS_HIP_EINVAL;
    const OptRow* r = find_option(key);
    if (!r) return SS_HIP_EINVAL;
    switch (r->norm) {
    case OptNorm::AsIs:   break;
    case OptNorm::Flag:   value = value ? 1 : 0; break;
    case OptNorm::Clamp:  value = std::max<long>(r->lo, std::min<long>(r->hi, value)); break;
    case OptNorm::Floor:  value = std::max<long>(r->lo, value); break;
    case OptNorm::Snap64: value = value > 32 ? 64 : 32; break;
    case OptNorm::Range:  if (value < r->lo || value > r->hi) return SS_HIP_EINVAL; break;
    case OptNorm::PassDebug:   // developer aid: device buffer of 1 + 4 * 4096 u64 (0 = off), tools/probe_pass_trace.py
        (void)hipSetDevice(ctx->device);
        return sship::set_pass_debug(reinterpret_cast<uint64_t*>(static_cast<uintptr_t>(value))) == hipSuccess ? SS_HIP_OK : SS_HIP_ERUNTIME;
    }
    if (r->i) ctx->*(r->i) = (int)value;
    else ctx->*(r->l) = value;
    if (r->i == &ss_hip_ctx::profile_solve_every) ctx->prof_solve_tick = 0;
    if (r->i == &ss_hip_ctx::screen_single) {
        // (setting the option also forgets what the context has learnt about its signals: the step-aside counters start again)
        ctx->sub_aside.reset();
        ctx->res_aside.reset();
    }
    return SS_HIP_OK;
}

int ss_hip_get_trace(ss_hip_ctx* ctx, uint32_t capacity, uint32_t* idx, uint8_t* added, double* gamma,
                     double* c_inf, uint32_t* count)
{
    if (!ctx || !count) return SS_HIP_EINVAL;
    const uint32_t n = (uint32_t)std::min<size_t>(capacity, ctx->last_trace.size());
    for (uint32_t i = 0; i < n; ++i) {
        if (idx) idx[i] = ctx->last_trace[i].idx;
        if (added) added[i] = (uint8_t)ctx->last_trace[i].added;
        if (gamma) gamma[i] = ctx->last_trace[i].gamma;
        if (c_inf) c_inf[i] = ctx->last_trace[i].c_inf;
    }
    *count = (uint32_t)ctx->last_trace.size();
    return SS_HIP_OK;
}

int ss_hip_get_option(ss_hip_ctx* ctx, const char* key, long* value)
{
    if (!ctx || !key || !value) return SS_HIP_EINVAL;
    const OptRow* r = find_option(key);
    if (!r || (!r->i && !r->l)) return SS_HIP_EINVAL;      // (a key without a member is an action: write-only)
    *value = r->i ? (long)(ctx->*(r->i)) : ctx->*(r->l);
    return SS_HIP_OK;
}

int ss_hip_ctx_info(const ss_hip_ctx* ctx, size_t* m, size_t* n, int* is_f64, int* device)
{
    if (!ctx) return SS_HIP_EINVAL;
    if (m) *m = ctx->m;
    if (n) *n = ctx->n;
    if (is_f64) *is_f64 = ctx->is_f64;
    if (device) *device = ctx->device;
    return SS_HIP_OK;
}

}  // extern "C"
