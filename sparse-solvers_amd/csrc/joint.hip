// joint.hip — joint sparse coding of signal groups: the group top correlations and the group class residuals (include/ss_hip.h):
//   ss_hip_group_top_correlations_*, ss_hip_group_class_residuals_*.
//
// A group is a run of consecutive signals that share one support (simultaneous OMP, the multiple-measurement-vector model).  The
// first call scores an atom by the l2 norm of its correlations with all residuals of the group and returns the k best atoms no
// member's record stores; the second adds the class residuals up over the members.  The first call's host side is the driver of the
// top correlations (tc_driver.h: its record check, residual block, norms and copies; the MFMA tile through tc_launch_dots).  This
// unit supplies the variant: chunks of whole groups (js_chunks) whose output rows are groups, the staged offsets and a score row a
// group to carve, and what runs on a chunk behind the dots.  Kernels of this file:
//
//   k_js_check    the offsets, before anything is written: the first group whose offsets do not start at 0, ascend strictly, end at B
//                 or span more than SS_HIP_GROUP_MAX signals.  An offset is compared, never used as an address.
//   k_js_scores   grid = (block of 256 columns, group).  First a pass over the members' records marks the block's stored columns in
//                 LDS (and a truncated member); then a thread owns a column and walks the members' rows of D in ascending order —
//                 the reads are coalesced along i, 4 L n bytes a group in fp32 — and writes the group's score row [n_pad] in double,
//                 a NaN word at a stored or excluded column.  D itself is not struck into: k_js_coef reads it afterwards.
//   k_js_select   one workgroup per group: tc_select.h's selection (tc_select_sorted: k_tc_select's total order, list, tie branch and
//                 prefix property) with the stored score as the key; it strikes nothing out and writes no coef.
//   k_js_coef     one workgroup per group: the members' coef rows from D and rn at the group's columns.
//   k_gc_reduce   one workgroup per group, threads over the classes: the class reduction and the arg-min.
//
// ORDER (stated once; build flag -ffp-contract=off: products and sums are rounded separately):
//   r_b, dot(i, b), d_i, rn_i   topcorr.hip's words (its ORDER block): the same kernels on the same rows.
//   q(i, g)      = sum_b (double)dot(i, b) * (double)dot(i, b): one accumulator, started at 0, the members in ascending b; each
//                product and each sum rounded on its own.
//   s(i, g)      = sqrt(q(i, g)) * rn_i in double: one square root, one multiplication.
//   candidates   the columns with d_i finite and non-zero that no member's record stores (by index); a NaN score is never selected;
//                a group with a truncated member (K > kmax) has none.
//   coef[b][t]   = (T)((double)dot(idx[g][t], b) * (rn * rn)), member by member: topcorr.hip's coef of that column and signal.
//   selection    a maximum under a total order (score descending, index ascending): tc_select.h.  No floating-point atomics.
//   Rg[g][c]     = (T)sqrt(sum_b (double)R[b][c] * (double)R[b][c]), R the words of ss_hip_class_residuals_*: one accumulator from 0,
//                the members ascending; best[g] = the left-most arg-min of the row as stored (a NaN is never smaller).
//   A GROUP OF ONE returns top_correlations' idx, score and coef words, and class_residuals' R row and best word: in fp32 the
//   square of a dot is exact in double, and in either precision sqrt(fl(x * x)) = |x| in binary round-to-nearest as long as x * x
//   neither underflows nor overflows (fp64 only: |x| between 2^-511 and 2^511 is safe).
// A group's rows depend on A, its own signals and records in order, and k: not on B, on the other groups, on the chunking (a chunk
// holds whole groups; a row of D is a function of its own signal), on where the pointers live or on what the context did before.
#include "ss_hip_internal.h"
#include "tc_driver.h"

#include <algorithm>
#include <cmath>

namespace sship {

namespace {

constexpr uint32_t kJsGroupMax = SS_HIP_GROUP_MAX;
constexpr size_t kGcChunkBytes = (size_t)64 << 20;       // the byte budget of a chunk's per-signal class rows (never changes a result)

// the workspace of the group class residuals (ss_hip_ctx::js); the group top correlations carve the top correlations' arena
WorkArena& state_of(ss_hip_ctx* ctx)
{
    return part<WorkArena>(ctx->js);
}

// ---- kernels -------------------------------------------------------------------------------------------------------------------

// off [Gn + 1]; bad: the first group whose offsets are wrong (the last group when the end is)
__global__ __launch_bounds__(256)
void k_js_check(const uint32_t* __restrict__ off, uint32_t Gn, uint32_t B, uint32_t* __restrict__ bad)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g > Gn) return;
    const uint32_t v = off[g];
    if (g == 0u && v != 0u) atomicMin(bad, 0u);
    if (g == Gn) {
        if (v != B) atomicMin(bad, Gn - 1u);
        return;
    }
    const uint32_t w = off[g + 1u];
    if (w <= v || w - v > kJsGroupMax) atomicMin(bad, g);
}

// D: the chunk's dots; rec: the chunk's first record, nullptr: no records; off: the offsets from the chunk's first group on; b0: the
// chunk's first signal; S: the chunk's score rows [groups][n_pad]
template <typename T>
__global__ __launch_bounds__(256)
void k_js_scores(const T* __restrict__ D, uint32_t n, uint32_t n_pad, const double* __restrict__ rinv, const unsigned char* __restrict__ rec,
                 size_t rb, uint32_t kmax, const uint32_t* __restrict__ off, uint32_t b0, double* __restrict__ S)
{
    __shared__ uint32_t s_mark[256];
    __shared__ uint32_t s_trunc;
    const uint32_t g = blockIdx.y, tid = threadIdx.x, base = blockIdx.x * 256u, i = base + tid;
    const uint32_t lo = off[g] - b0, hi = off[g + 1u] - b0;      // (validated: k_js_check)
    s_mark[tid] = 0u;
    if (tid == 0) s_trunc = 0u;
    __syncthreads();
    if (rec) {
        for (uint32_t b = lo; b < hi; ++b) {
            const unsigned char* r = rec + (size_t)b * rb;
            const uint32_t K = *reinterpret_cast<const uint32_t*>(r);
            if (K > kmax) {                                      // a truncated record does not hold its support: the group has no candidates
                if (tid == 0) s_trunc = 1u;
                continue;
            }
            const uint32_t* idx = reinterpret_cast<const uint32_t*>(r + 16);
            for (uint32_t e = tid; e < K; e += 256u) {
                const uint32_t c = idx[e] - base;                // (every thread that marks writes the same word)
                if (c < 256u) s_mark[c] = 1u;
            }
        }
        __syncthreads();
    }
    double s = tc_nan(0.0);
    const double r = rinv[i];
    if (s_trunc == 0u && i < n && r != 0.0 && s_mark[tid] == 0u) {
        const T* d = D + (size_t)lo * n_pad + i;
        double q = 0.0;
        uint32_t b = lo;
        for (; b + 4u <= hi; b += 4u, d += 4u * (size_t)n_pad) {  // four loads in flight, added in ascending member order
            const double x0 = (double)d[0], x1 = (double)d[n_pad], x2 = (double)d[2u * (size_t)n_pad], x3 = (double)d[3u * (size_t)n_pad];
            q += x0 * x0;
            q += x1 * x1;
            q += x2 * x2;
            q += x3 * x3;
        }
        for (; b < hi; ++b, d += n_pad) {
            const double x = (double)d[0];
            q += x * x;
        }
        s = sqrt(q) * r;
    }
    S[(size_t)g * n_pad + i] = s;
}

__global__ __launch_bounds__(256)
void k_js_select(const double* __restrict__ S, uint32_t n, uint32_t n_pad, uint32_t k, uint32_t* __restrict__ oidx, double* __restrict__ oscore)
{
    __shared__ TcSelectLds lds;
    const uint32_t g = blockIdx.x, tid = threadIdx.x;
    const double* s = S + (size_t)g * n_pad;
    oidx += (size_t)g * k;
    oscore += (size_t)g * k;
    // the key of column i, false for a column that is no candidate (its stored score is a NaN)
    auto keyof = [&](uint32_t i, unsigned long long& key) -> bool {
        const double v = s[i];
        if (!(v == v)) return false;
        key = (unsigned long long)__double_as_longlong(v);
        return true;
    };
    const uint32_t L = tc_select_sorted(lds, n, k, keyof);
    for (uint32_t t = tid; t < k; t += 256u) {
        if (t < L) {
            oidx[t] = lds.lidx[t];
            oscore[t] = __longlong_as_double((long long)lds.lkey[t]);
        } else {
            oidx[t] = kTcNone;
            oscore[t] = 0.0;
        }
    }
}

// oidx: the chunk's group rows [groups][k]; ocoef: the chunk's signal rows [signals][k]
template <typename T>
__global__ __launch_bounds__(256)
void k_js_coef(const T* __restrict__ D, uint32_t n_pad, const double* __restrict__ rinv, const uint32_t* __restrict__ off, uint32_t b0, uint32_t k,
               const uint32_t* __restrict__ oidx, T* __restrict__ ocoef)
{
    const uint32_t g = blockIdx.x;
    const uint32_t lo = off[g] - b0, hi = off[g + 1u] - b0;
    for (uint32_t e = threadIdx.x; e < (hi - lo) * k; e += 256u) {
        const uint32_t b = lo + e / k, t = e % k, i = oidx[(size_t)g * k + t];
        T v = T(0);
        if (i != kTcNone) {
            const double r = rinv[i];
            v = (T)((double)D[(size_t)b * n_pad + i] * (r * r));
        }
        ocoef[(size_t)b * k + t] = v;
    }
}

// R [signals][C] and bestb [signals]: the chunk's rows of class_residuals; Rg [groups][C], bestg [groups]
template <typename T>
__global__ __launch_bounds__(256)
void k_gc_reduce(const T* __restrict__ R, const uint32_t* __restrict__ bestb, uint32_t C, const uint32_t* __restrict__ off, uint32_t b0,
                 T* __restrict__ Rg, uint32_t* __restrict__ bestg)
{
    __shared__ uint32_t s_trunc;
    __shared__ T s_v[4];
    __shared__ uint32_t s_c[4];
    const uint32_t g = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t lo = off[g] - b0, hi = off[g + 1u] - b0;
    T* row = Rg + (size_t)g * C;
    if (tid == 0) s_trunc = 0u;
    __syncthreads();
    if (lo + tid < hi && bestb[lo + tid] == 0xffffffffu) s_trunc = 1u;       // (a group holds at most 256 members: one a thread)
    __syncthreads();
    if (s_trunc != 0u) {                                         // a truncated member: no class is claimed
        for (uint32_t c = tid; c < C; c += 256u) row[c] = tc_nan(T(0));
        if (tid == 0) bestg[g] = 0xffffffffu;
        return;
    }
    for (uint32_t c = tid; c < C; c += 256u) {
        double q = 0.0;
        for (uint32_t b = lo; b < hi; ++b) {
            const double x = (double)R[(size_t)b * C + c];
            q += x * x;
        }
        row[c] = (T)sqrt(q);
    }
    __threadfence_block();
    __syncthreads();
    // left-most arg-min of the row as stored (a NaN is never smaller): k_cls_finish's rule
    T bv = row[0];
    uint32_t bc = 0u;
    for (uint32_t c = tid; c < C; c += 256u) {
        const T v = row[c];
        if (c != 0u && (v < bv || (v == bv && c < bc) || (bv != bv && v == v))) { bv = v; bc = c; }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const T ov = __shfl_xor(bv, o);
        const uint32_t oc = (uint32_t)__shfl_xor((int)bc, o);
        if (ov < bv || (ov == bv && oc < bc) || (bv != bv && ov == ov)) { bv = ov; bc = oc; }
    }
    if (lane == 0u) { s_v[wave] = bv; s_c[wave] = bc; }
    __syncthreads();
    if (tid == 0) {
        for (uint32_t w = 1; w < 4u; ++w) {
            const T ov = s_v[w];
            const uint32_t oc = s_c[w];
            if (ov < bv || (ov == bv && oc < bc) || (bv != bv && ov == ov)) { bv = ov; bc = oc; }
        }
        bestg[g] = bc;
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------

// the checks of the offsets the host can make without reading them, in the order they are reported (B > 0)
int js_check_groups(const char* who, const uint32_t* group_off, size_t Gn, size_t B, char* err, size_t errlen)
{
    if (!group_off || Gn == 0 || Gn > B) {
        set_err(err, errlen, std::string(who) + ": group_off must not be null and must hold 1..B groups");
        return SS_HIP_EINVAL;
    }
    return SS_HIP_OK;
}

// The offsets checked on the device (k_js_check) and fetched: hoff [Gn + 1].  Nothing of the caller's has been written when they are
// wrong.  The workspace is grown for the staging alone: the caller carves it anew afterwards.
int js_fetch_offsets(ss_hip_ctx* ctx, WorkArena& js, const char* who, const uint32_t* group_off, size_t Gn, size_t B, std::vector<uint32_t>& hoff,
                     char* err, size_t errlen)
{
    hipStream_t st = ctx->stream;
    Carver cv(nullptr);
    cv.take<uint32_t>(1);
    cv.take<uint32_t>(Gn + 1);
    if (!arena_grow(js, cv.off, who, err, errlen)) return SS_HIP_ENOMEM;
    Carver cw(js.buf);
    uint32_t* bad = cw.take<uint32_t>(1);
    uint32_t* stage = cw.take<uint32_t>(Gn + 1);
    const uint32_t* doff = group_off;
    if (!on_device(group_off)) { HIPCHK(hipMemcpyAsync(stage, group_off, (Gn + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, st)); doff = stage; }
    flag_arm(bad, st);
    hipLaunchKernelGGL(k_js_check, dim3((uint32_t)((Gn + 256) / 256)), dim3(256), 0, st, doff, (uint32_t)Gn, (uint32_t)B, bad);
    HIPCHK(hipGetLastError());
    uint32_t first_bad;
    hoff.resize(Gn + 1);
    flag_fetch(&first_bad, bad, st, 1, hoff.data(), doff, (Gn + 1) * sizeof(uint32_t));
    if (first_bad != kNoRecord) {
        set_err(err, errlen, std::string(who) + ": group_off must start at 0, ascend strictly, end at B and hold no group of more than " +
                                 std::to_string(kJsGroupMax) + " signals (first bad group: " + std::to_string(first_bad) + ")");
        return SS_HIP_EINVAL;
    }
    return SS_HIP_OK;
}

// The chunks of a call: runs of whole groups — a chunk's rows — of at most `cap` signals and `budget` bytes (per_sig a signal,
// per_grp a group); a group that exceeds either on its own is a chunk of its own
std::vector<TcChunk> js_chunks(const std::vector<uint32_t>& hoff, size_t cap, size_t budget, size_t per_sig, size_t per_grp)
{
    const size_t Gn = hoff.size() - 1;
    std::vector<TcChunk> out;
    for (size_t g0 = 0; g0 < Gn;) {
        size_t g1 = g0, sig = 0;
        while (g1 < Gn) {
            const size_t L = hoff[g1 + 1] - hoff[g1];
            if (g1 > g0 && (sig + L > cap || (sig + L) * per_sig + (g1 - g0 + 1) * per_grp > budget)) break;
            sig += L;
            g1 += 1;
        }
        out.push_back({ hoff[g0], g0, (uint32_t)sig, (uint32_t)(g1 - g0) });
        g0 = g1;
    }
    return out;
}

// the variant of the driver (tc_driver.h): a chunk's rows are its groups; the staged offsets and a score row a group; rn_i; per
// chunk the dots, the groups' scores, their selection and the members' coef rows
template <typename T> struct GroupVariant {
    const uint32_t* group_off;         // the caller's offsets, or nullptr: hoff is staged
    const std::vector<uint32_t>& hoff;
    uint32_t* offs = nullptr;
    double* S = nullptr;
    const uint32_t* doff = nullptr;

    void carve(const ss_hip_ctx* ctx, Carver& cv, size_t, size_t, size_t max_grp)
    {
        offs = group_off ? nullptr : cv.take<uint32_t>(hoff.size());
        S = cv.take<double>(max_grp * ctx->n_pad);
    }
    hipError_t prepare(ss_hip_ctx* ctx, double* rinv)
    {
        doff = group_off;
        if (!group_off) {
            const hipError_t e = hipMemcpyAsync(offs, hoff.data(), hoff.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream);
            if (e != hipSuccess) return e;
            doff = offs;
        }
        return coh_launch_norms<T>(ctx, rinv);
    }
    void chunk(ss_hip_ctx* ctx, const TcCall<T>& c, const TcChunk& ch, const TcWork<T>& w)
    {
        hipStream_t st = ctx->stream;
        const uint32_t n = (uint32_t)ctx->n, n_pad = ctx->n_pad, k = c.k;
        HIPCHK(tc_launch_dots<T>(ctx, w.R, ch.Bc, w.D));
        hipLaunchKernelGGL((k_js_scores<T>), dim3(n_pad / 256u, ch.Rc), dim3(256), 0, st, (const T*)w.D, n, n_pad, w.norms, w.recs, w.rb, c.kmax,
                           doff + ch.r0, (uint32_t)ch.b0, S);
        hipLaunchKernelGGL(k_js_select, dim3(ch.Rc), dim3(256), 0, st, (const double*)S, n, n_pad, k, w.oi + ch.r0 * k, w.os + ch.r0 * k);
        hipLaunchKernelGGL((k_js_coef<T>), dim3(ch.Rc), dim3(256), 0, st, (const T*)w.D, n_pad, w.norms, doff + ch.r0, (uint32_t)ch.b0, k,
                           (const uint32_t*)(w.oi + ch.r0 * k), w.oc + ch.b0 * k);
        HIPCHK(hipGetLastError());
    }
};

template <typename T>
int group_topcorr_entry(ss_hip_ctx* ctx, const TcCall<T>& c, const uint32_t* group_off, size_t Gn)
{
    int rc = tc_check_call<T>(ctx, c);
    if (rc != SS_HIP_OK) return rc;
    if (c.B == 0 && Gn != 0) { set_err(c.err, c.errlen, "group_top_correlations: no signals, but groups"); return SS_HIP_EINVAL; }
    return tc_run(c, [&] {
        int rg = js_check_groups(c.who, group_off, Gn, c.B, c.err, c.errlen);
        if (rg != SS_HIP_OK) return rg;
        HIPCHK(hipSetDevice(ctx->device));
        std::vector<uint32_t> hoff;
        if ((rg = js_fetch_offsets(ctx, topcorr_arena(ctx), c.who, group_off, Gn, c.B, hoff, c.err, c.errlen)) != SS_HIP_OK) return rg;
        // whole groups under topcorr.hip's byte budget and signal cap, plus a score row a group
        const bool y_dev = on_device(c.Y);
        const size_t cap = ctx->tc_chunk_max > 0 ? std::min<size_t>(kTcChunkMax, (size_t)ctx->tc_chunk_max) : kTcChunkMax;
        GroupVariant<T> v{ on_device(group_off) ? group_off : nullptr, hoff };
        return tc_drive<T>(ctx, c, y_dev, Gn, js_chunks(hoff, cap, kTcChunkBytes, tc_signal_bytes<T>(ctx, y_dev, 1), (size_t)ctx->n_pad * sizeof(double)), v);
    });
}

// the group class residuals' pieces: a host caller's offsets, the groups' rows and best, a chunk's per-signal rows and best
template <typename T> struct GroupClassWork {
    uint32_t *offs, *ob, *bb;
    T *og, *Rb;
    void carve(Carver& cv, bool off_dev, size_t Gn, uint32_t C, size_t max_sig)
    {
        offs = off_dev ? nullptr : cv.take<uint32_t>(Gn + 1);
        og = cv.take<T>(Gn * C);
        ob = cv.take<uint32_t>(Gn);
        Rb = cv.take<T>(max_sig * C);
        bb = cv.take<uint32_t>(max_sig);
    }
};

template <typename T>
int group_classes_impl(ss_hip_ctx* ctx, const T* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const void* records, uint32_t kmax,
                       const uint32_t* group_off, size_t Gn, T* Rg, ptrdiff_t rg_stride, uint32_t* best, char* err, size_t errlen)
{
    static const char* who = "group_class_residuals";
    HIPCHK(hipSetDevice(ctx->device));
    WorkArena& js = state_of(ctx);
    hipStream_t st = ctx->stream;
    const size_t rb = record_bytes(kmax, sizeof(T));
    const uint32_t C = classify_num_classes(ctx);
    const bool off_dev = on_device(group_off);

    std::vector<uint32_t> hoff;
    int rc = js_fetch_offsets(ctx, js, who, group_off, Gn, B, hoff, err, errlen);
    if (rc != SS_HIP_OK) return rc;

    // the per-signal rows never leave the context: chunks of whole groups under a fixed byte budget
    const std::vector<TcChunk> chunks = js_chunks(hoff, kTcChunkMax, kGcChunkBytes, (size_t)C * sizeof(T) + sizeof(uint32_t), 0);
    size_t max_sig = 0, max_grp = 0;
    tc_chunk_extent(chunks, max_sig, max_grp);

    GroupClassWork<T> w;
    if (!arena_grow(js, carve_into(nullptr, w, off_dev, Gn, C, max_sig), who, err, errlen)) return SS_HIP_ENOMEM;
    carve_into(js.buf, w, off_dev, Gn, C, max_sig);

    const uint32_t* doff = group_off;
    if (!off_dev) { HIPCHK(hipMemcpyAsync(w.offs, hoff.data(), (Gn + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, st)); doff = w.offs; }
    for (const TcChunk& ch : chunks) {
        const size_t b0 = ch.b0, Bc = ch.Bc;
        rc = class_residual_rows<T>(ctx, who, Y + (ptrdiff_t)b0 * y_stride, Bc, y_stride, incy, static_cast<const unsigned char*>(records) + b0 * rb,
                                    kmax, w.Rb, (ptrdiff_t)C, w.bb, err, errlen);
        if (rc != SS_HIP_OK) return rc;                   // (a record index >= n: nothing of the caller's has been written)
        hipLaunchKernelGGL((k_gc_reduce<T>), dim3(ch.Rc), dim3(256), 0, st, (const T*)w.Rb, (const uint32_t*)w.bb, C, doff + ch.r0, (uint32_t)b0,
                           w.og + ch.r0 * C, w.ob + ch.r0);
        HIPCHK(hipGetLastError());
    }
    if (Rg) HIPCHK(hipMemcpy2DAsync(Rg, (size_t)rg_stride * sizeof(T), w.og, (size_t)C * sizeof(T), (size_t)C * sizeof(T), Gn, hipMemcpyDefault, st));
    HIPCHK(hipMemcpyAsync(best, w.ob, Gn * sizeof(uint32_t), hipMemcpyDefault, st));
    HIPCHK(hipStreamSynchronize(st));
    return SS_HIP_OK;
}

template <typename T>
int group_classes_entry(ss_hip_ctx* ctx, const T* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const void* records, uint32_t kmax,
                        const uint32_t* group_off, size_t Gn, T* Rg, ptrdiff_t rg_stride, uint32_t* best, char* err, size_t errlen)
{
    static const char* who = "group_class_residuals";
    int rc = check_common<T>(ctx, who, records, true, kmax, err, errlen);
    if (rc != SS_HIP_OK) return rc;
    if (!Y || !best) { set_err(err, errlen, "group_class_residuals: Y and best must not be null"); return SS_HIP_EINVAL; }
    const uint32_t C = classify_num_classes(ctx);
    if (C == 0) { set_err(err, errlen, "group_class_residuals: no classes set (ss_hip_set_classes)"); return SS_HIP_EINVAL; }
    if (B == 0) {
        if (Gn != 0) { set_err(err, errlen, "group_class_residuals: no signals, but groups"); return SS_HIP_EINVAL; }
        return SS_HIP_OK;
    }
    if (incy <= 0 || y_stride <= 0) { set_err(err, errlen, "group_class_residuals: increments and strides must be positive"); return SS_HIP_EINVAL; }
    if (Rg && rg_stride < (ptrdiff_t)C) { set_err(err, errlen, "group_class_residuals: rg_stride must be at least num_classes"); return SS_HIP_EINVAL; }
    if ((rc = check_batch(who, B, err, errlen)) != SS_HIP_OK) return rc;
    if ((rc = js_check_groups(who, group_off, Gn, B, err, errlen)) != SS_HIP_OK) return rc;
    return guarded(err, errlen, who, [&] {
        return group_classes_impl<T>(ctx, Y, B, y_stride, incy, records, kmax, group_off, Gn, Rg, rg_stride, best, err, errlen);
    });
}

}  // namespace

// k_js_select as a launch of its own (ss_hip_internal.h), on the context's stream, every pointer on the device: the k best of the first
// n keys of every row of S [rows][pitch] — a stored score in double, a NaN word for no candidate — into oidx / oscore [rows][k].  For
// the class top correlations (blockcode.hip), whose rows are a signal's class scores: the same kernel, no second statement of it
hipError_t js_launch_select(ss_hip_ctx* ctx, const double* S, uint32_t rows, uint32_t n, uint32_t pitch, uint32_t k, uint32_t* oidx, double* oscore)
{
    hipLaunchKernelGGL(k_js_select, dim3(rows), dim3(256), 0, ctx->stream, S, n, pitch, k, oidx, oscore);
    return hipGetLastError();
}

}  // namespace sship

using namespace sship;

extern "C" {

int ss_hip_group_top_correlations_f32(ss_hip_ctx* ctx, const float* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const void* records,
                                      uint32_t kmax, const uint32_t* group_off, size_t Gn, uint32_t k, uint32_t* idx, float* coef, double* score,
                                      char* err, size_t errlen)
{
    return group_topcorr_entry<float>(ctx, { "group_top_correlations", Y, B, y_stride, incy, records, kmax, k, idx, coef, score, err, errlen }, group_off,
                                      Gn);
}
int ss_hip_group_top_correlations_f64(ss_hip_ctx* ctx, const double* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const void* records,
                                      uint32_t kmax, const uint32_t* group_off, size_t Gn, uint32_t k, uint32_t* idx, double* coef, double* score,
                                      char* err, size_t errlen)
{
    return group_topcorr_entry<double>(ctx, { "group_top_correlations", Y, B, y_stride, incy, records, kmax, k, idx, coef, score, err, errlen }, group_off,
                                       Gn);
}

int ss_hip_group_class_residuals_f32(ss_hip_ctx* ctx, const float* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const void* records,
                                     uint32_t kmax, const uint32_t* group_off, size_t Gn, float* Rg, ptrdiff_t rg_stride, uint32_t* best, char* err,
                                     size_t errlen)
{
    return group_classes_entry<float>(ctx, Y, B, y_stride, incy, records, kmax, group_off, Gn, Rg, rg_stride, best, err, errlen);
}
int ss_hip_group_class_residuals_f64(ss_hip_ctx* ctx, const double* Y, size_t B, ptrdiff_t y_stride, ptrdiff_t incy, const void* records,
                                     uint32_t kmax, const uint32_t* group_off, size_t Gn, double* Rg, ptrdiff_t rg_stride, uint32_t* best, char* err,
                                     size_t errlen)
{
    return group_classes_entry<double>(ctx, Y, B, y_stride, incy, records, kmax, group_off, Gn, Rg, rg_stride, best, err, errlen);
}

}  // extern "C"
