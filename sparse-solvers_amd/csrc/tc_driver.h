// The host side of the four top-correlation calls (topcorr.hip, nonneg.hip, weighted.hip, joint.hip) and of the robust weights
// (robust.hip, which stops behind the residual block), stated once: the checks their
// entry points share, the arena they carve from, and the driver — stage the records, check them, the norms, then chunk by chunk the
// signals and the residual block, and the copies out.  What a call adds is its VARIANT, which the driver never asks for its name:
//   the chunk list   runs of signals with their runs of output rows (tc_uniform_chunks for a row a signal, joint.hip's js_chunks for
//                    a row a group); the bytes per signal that size a chunk are the variant's own (tc_signal_bytes),
//   v.carve          the buffers only it needs, behind the common ones (the most signals of a chunk, those in whole tiles, the most rows),
//   v.prepare        the launch that fills the norms [n_pad], and whatever else it stages once for its chunks,
//   v.chunk          everything behind a chunk's residual block: its products, its selection.
// A later variant is a key function for k_tc_select (tc_select.h) plus the kernels only it needs.
// Everything sits in an unnamed namespace: each unit gets its own copy, nothing here is part of the library's link surface.
#pragma once

#include "record_common.h"
#include "tc_select.h"

#include <algorithm>
#include <string>
#include <vector>

namespace sship {

namespace {

// the arguments the four calls share, as the C ABI passes them
template <typename T> struct TcCall {
    const char* who;
    const T* Y;
    size_t B;
    ptrdiff_t y_stride, incy;
    const void* records;
    uint32_t kmax, k;
    uint32_t* idx;
    T* coef;
    double* score;
    char* err;
    size_t errlen;
};

// signals [b0, b0 + Bc) and the rows [r0, r0 + Rc) of idx / score they fill (coef always has a row a signal)
struct TcChunk { size_t b0, r0; uint32_t Bc, Rc; };

// what the driver carved and staged, as a variant's launches see it: norms [n_pad]; recs: the CHUNK's first record on the device
// (nullptr: no records), rb bytes each; R [signals of the chunk, whole tiles][ldm], D [the same][n_pad]; oi / os [rows][k], oc [B][k]
template <typename T> struct TcWork {
    const double* norms;
    const unsigned char* recs;
    size_t rb;
    T* R;
    T* D;
    uint32_t* oi;
    T* oc;
    double* os;
};

// ---- the entry points ------------------------------------------------------------------------------------------------------------

inline int tc_check_k(const char* who, uint32_t k, char* err, size_t errlen)
{
    if (k == 0 || k > (uint32_t)SS_HIP_TOPCORR_KMAX) {
        set_err(err, errlen, std::string(who) + ": k must be 1.." + std::to_string(SS_HIP_TOPCORR_KMAX));
        return SS_HIP_EINVAL;
    }
    return SS_HIP_OK;
}

// the checks the four entry points share, in the order they are reported; a variant's own follow, then tc_run
template <typename T>
int tc_check_call(const ss_hip_ctx* ctx, const TcCall<T>& c)
{
    // (without records kmax is ignored: the checks see a capacity that passes)
    int rc = check_common<T>(ctx, c.who, c.records, false, c.records ? c.kmax : 1u, c.err, c.errlen);
    if (rc != SS_HIP_OK) return rc;
    if (!c.Y || !c.idx) { set_err(c.err, c.errlen, std::string(c.who) + ": Y and idx must not be null"); return SS_HIP_EINVAL; }
    if ((rc = tc_check_k(c.who, c.k, c.err, c.errlen)) != SS_HIP_OK) return rc;
    if (c.incy <= 0 || c.y_stride <= 0) {
        set_err(c.err, c.errlen, std::string(c.who) + ": increments and strides must be positive");
        return SS_HIP_EINVAL;
    }
    return SS_HIP_OK;
}

// ... and their common end: an empty batch is done (every argument was checked all the same), the bound on B, the call itself
template <typename T, typename F>
int tc_run(const TcCall<T>& c, F&& impl)
{
    if (c.B == 0) return SS_HIP_OK;
    if (const int rc = check_batch(c.who, c.B, c.err, c.errlen)) return rc;
    return guarded(c.err, c.errlen, c.who, impl);
}

// ---- the arena and the chunks ------------------------------------------------------------------------------------------------------

// grow() with an out-of-memory failure turned into the call's SS_HIP_ENOMEM and a message that names the bytes
inline bool arena_grow(WorkArena& a, size_t need, const char* who, char* err, size_t errlen)
{
    try {
        grow(a, need, "hipMalloc(coding workspace)");
    } catch (const HipFail& f) {
        if (f.code != hipErrorOutOfMemory) throw;
        (void)hipGetLastError();
        set_err(err, errlen, std::string(who) + ": no device memory for a workspace of " + std::to_string(need) + " bytes");
        return false;
    }
    return true;
}

// the bytes a signal of a chunk takes with `blocks` residual blocks and `dots` dot blocks — as many, unless the call says otherwise
// (never changes a result)
template <typename T>
size_t tc_signal_bytes(const ss_hip_ctx* ctx, bool y_dev, size_t blocks, size_t dots = ~(size_t)0)
{
    const size_t rtiles = (ctx->m + kClsTileRows - 1) / kClsTileRows;
    if (dots == ~(size_t)0) dots = blocks;
    return blocks * (size_t)ctx->ldm * sizeof(T) + dots * (size_t)ctx->n_pad * sizeof(T) + rtiles * 4u * sizeof(double) +
           (y_dev ? 0 : ctx->m * sizeof(T));
}

// a row a signal: whole signal tiles under the byte budget, kTcChunkMax and the tc_chunk_max option
inline std::vector<TcChunk> tc_uniform_chunks(const ss_hip_ctx* ctx, size_t B, size_t per)
{
    size_t chunk = std::max<size_t>(kTcTile, std::min<size_t>(kTcChunkMax, kTcChunkBytes / per) / kTcTile * kTcTile);
    if (ctx->tc_chunk_max > 0) chunk = std::min<size_t>(chunk, (size_t)ctx->tc_chunk_max);
    chunk = std::min(chunk, B);
    std::vector<TcChunk> out;
    for (size_t b0 = 0; b0 < B; b0 += chunk) {
        const uint32_t Bc = (uint32_t)std::min(chunk, B - b0);
        out.push_back({ b0, b0, Bc, Bc });
    }
    return out;
}

// the most signals and the most rows a chunk of the list holds
inline void tc_chunk_extent(const std::vector<TcChunk>& chunks, size_t& max_sig, size_t& max_rows)
{
    max_sig = max_rows = 0;
    for (const TcChunk& ch : chunks) { max_sig = std::max<size_t>(max_sig, ch.Bc); max_rows = std::max<size_t>(max_rows, ch.Rc); }
}

// ---- the driver ----------------------------------------------------------------------------------------------------------------

// rows: the rows of idx / score (coef has B).  Nothing of the caller's has been written when a record is invalid.  The caller has
// made the context's device current: that is the first thing a call does behind its checks, before it asks where a pointer lives.
// A call that selects nothing (k == 0, idx null: robust.hip, which wants the residual block alone) has no dot block and no copies out.
template <typename T, typename V>
int tc_drive(ss_hip_ctx* ctx, const TcCall<T>& c, bool y_dev, size_t rows, const std::vector<TcChunk>& chunks, V& v)
{
    hipStream_t st = ctx->stream;
    const size_t m = ctx->m, B = c.B, k = c.k, rb = c.records ? record_bytes(c.kmax, sizeof(T)) : 0;
    const uint32_t ldm = ctx->ldm, n_pad = ctx->n_pad, rtiles = (uint32_t)((m + kClsTileRows - 1) / kClsTileRows);
    RecordPlace place(c.records, nullptr, B * rb);
    size_t max_sig = 0, max_rows = 0;
    tc_chunk_extent(chunks, max_sig, max_rows);
    const size_t sig_pad = (max_sig + kTcTile - 1) / kTcTile * kTcTile;

    TcWork<T> w{};
    double* norms = nullptr;
    double* part = nullptr;
    uint32_t* bad = nullptr;
    unsigned char* stage = nullptr;
    T* ybuf = nullptr;
    auto carve = [&](unsigned char* base) {
        Carver cv(base);
        norms = cv.take<double>(n_pad);
        bad = cv.take<uint32_t>(1);
        stage = place.carve(cv);
        w.oi = cv.take<uint32_t>(rows * k);
        w.oc = cv.take<T>(B * k);
        w.os = cv.take<double>(rows * k);
        w.R = cv.take<T>(sig_pad * ldm);
        w.D = cv.take<T>(k ? sig_pad * n_pad : 0);
        part = cv.take<double>(max_sig * rtiles * 4u);
        ybuf = y_dev ? nullptr : cv.take<T>(max_sig * m);
        v.carve(ctx, cv, max_sig, sig_pad, max_rows);
        return cv.off;
    };
    WorkArena& arena = topcorr_arena(ctx);
    if (!arena_grow(arena, carve(nullptr), c.who, c.err, c.errlen)) return SS_HIP_ENOMEM;
    carve(arena.buf);
    w.norms = norms;
    w.rb = rb;

    place.stage_in(stage, st);
    if (c.records) {
        HIPCHK(tc_launch_record_check(ctx, place.din, rb, c.kmax, (uint32_t)B, bad));
        if (const int rc = flag_verdict(bad, st, c.who, c.err, c.errlen)) return rc;      // (nothing has been written when a record is invalid)
    }
    HIPCHK(v.prepare(ctx, norms));
    std::vector<T> tmp;
    for (const TcChunk& ch : chunks) {
        const ChunkSignals<T> y = chunk_signals<T>(ctx, c.Y, c.y_stride, c.incy, y_dev, ybuf, ch.b0, ch.Bc, tmp);
        w.recs = c.records ? place.din + ch.b0 * rb : nullptr;
        HIPCHK(tc_launch_residual_block<T>(ctx, y.yd, y.ys, y.yi, w.recs, rb, c.kmax, ch.Bc, w.R, part));
        v.chunk(ctx, c, ch, w);
    }
    if (c.idx) HIPCHK(hipMemcpyAsync(c.idx, w.oi, rows * k * sizeof(uint32_t), hipMemcpyDefault, st));
    if (c.coef) HIPCHK(hipMemcpyAsync(c.coef, w.oc, B * k * sizeof(T), hipMemcpyDefault, st));
    if (c.score) HIPCHK(hipMemcpyAsync(c.score, w.os, rows * k * sizeof(double), hipMemcpyDefault, st));
    HIPCHK(hipStreamSynchronize(st));
    return SS_HIP_OK;
}

// the selection launch of a chunk whose rows are its signals: k_tc_select (tc_select.h) with the variant's scorer
template <typename T, typename Scorer>
void tc_launch_select(ss_hip_ctx* ctx, const TcCall<T>& c, const TcChunk& ch, const TcWork<T>& w, const Scorer& sc)
{
    const size_t o = ch.b0 * c.k;
    hipLaunchKernelGGL((k_tc_select<T, Scorer>), dim3(ch.Bc), dim3(256), 0, ctx->stream, w.D, (uint32_t)ctx->n, ctx->n_pad, sc, w.recs, w.rb, c.kmax, c.k,
                       w.oi + o, w.oc + o, w.os + o);
    HIPCHK(hipGetLastError());
}

// The call that needs nothing beyond the dots and rn_i (top_correlations, nonneg_top_correlations): its variant and its entry point,
// parameterised by the scorer, which holds rn
template <typename T, typename Scorer> struct TcDotsVariant {
    void carve(const ss_hip_ctx*, Carver&, size_t, size_t, size_t) {}
    hipError_t prepare(ss_hip_ctx* ctx, double* rinv) { return coh_launch_norms<T>(ctx, rinv); }
    void chunk(ss_hip_ctx* ctx, const TcCall<T>& c, const TcChunk& ch, const TcWork<T>& w)
    {
        HIPCHK(tc_launch_dots<T>(ctx, w.R, ch.Bc, w.D));
        tc_launch_select(ctx, c, ch, w, Scorer{ w.norms });
    }
};

template <typename T, typename Scorer>
int tc_dots_entry(ss_hip_ctx* ctx, const TcCall<T>& c)
{
    const int rc = tc_check_call<T>(ctx, c);
    if (rc != SS_HIP_OK) return rc;
    return tc_run(c, [&] {
        HIPCHK(hipSetDevice(ctx->device));
        const bool y_dev = on_device(c.Y);
        TcDotsVariant<T, Scorer> v;
        return tc_drive<T>(ctx, c, y_dev, c.B, tc_uniform_chunks(ctx, c.B, tc_signal_bytes<T>(ctx, y_dev, 1)), v);
    });
}

}  // namespace

}  // namespace sship
