// The host side of the three atom learning calls (dictlearn.hip, ksvd.hip, wdictlearn.hip), stated once.  Each call reads compact
// records and a list of atoms and returns atoms, usage and an objective; its driver runs these steps top to bottom, its own launches
// between them:
//   learn_check_args   the entry points' checks, in the order they are reported
//   learn_atoms        the list of atoms on the host, checked; the shapes; where each pointer lives
//   learn_carve        an index or a work struct carved out of its part of the context's one arena (learn_arena): the common pieces
//                      are LearnIndex's and LearnWork's, a unit's own are members of a small struct of its own beside them
//   learn_open         the records staged, the slot map and the columns uploaded, the counts, the one read-back
//   learn_chunk        the signals whose residuals a chunked call holds at once
//   learn_finish       the copies out, the final synchronise, the changed atoms through the column replacement
// Every call ends with its own stream synchronise, so the three share the arena and carve it anew every time.
// Everything sits in an unnamed namespace: each unit gets its own copy, nothing here is part of the library's link surface.
#pragma once

#include "record_common.h"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

namespace sship {

namespace {

constexpr size_t kDlChunkBytes = (size_t)256 << 20;      // byte budget of each block of a chunk, [chunk][ldm] (never changes a result)
constexpr uint32_t kDlChunkMax = 32768;                  // most signals per chunk (grid.y of k_dl_residual)

// one call: its arguments as the C ABI passes them, then what the steps derive from them
template <typename T> struct LearnCall {
    ss_hip_ctx* ctx;
    const char* who;
    const T* Y;
    size_t B;
    ptrdiff_t y_stride, incy;
    const void* records;
    uint32_t kmax;
    void* records_out;                 // (null: the call writes no records)
    const uint32_t* cols;
    size_t S;
    T* V;
    ptrdiff_t rs, cs;
    uint32_t* usage;
    double* objective;
    bool apply;
    char* err;
    size_t errlen;
    // learn_atoms: the list on the host, the shapes, where the pointers live
    std::vector<uint32_t> hc = {};
    size_t m = 0, n = 0, rb = 0;
    uint32_t ldm = 0, ntiles = 0, per = 0;
    bool y_dev = false, v_dev = false;
    RecordPlace place{};                 // (learn_open stages: place.din, place.dout)
    // learn_open: the slot map (it lives as long as the call: its upload is asynchronous); the lists' total and longest length
    std::vector<uint32_t> slots = {};
    uint32_t total = 0, longest = 0;
};

// ---- the entry points ------------------------------------------------------------------------------------------------------------

// what differs between the entry points' checks: texts are null where the rule is kept
struct LearnRules {
    const char* null_y;                // the words for a null Y
    const char* own;                   // the call's own rule on its pointers, where it is broken: its words
    uint32_t flags, mask;              // the flag word and the bits the call knows
    const char* nothing;               // where no output is asked for: the words
    bool weighted;                     // the weighted calls' rules for W (weights_check_args)
    const void* W;
    ptrdiff_t w_stride;
};

// the checks the three entry points share, in the order they are reported.  empty: every argument is valid and there is nothing to do
template <typename T>
int learn_check_args(const LearnCall<T>& c, const LearnRules& r, bool& empty)
{
    const std::string w(c.who);
    auto fail = [&](const char* text) { set_err(c.err, c.errlen, w + ": " + text); return SS_HIP_EINVAL; };
    int rc = check_common<T>(c.ctx, c.who, c.records, true, c.kmax, c.err, c.errlen);
    if (rc != SS_HIP_OK) return rc;
    if (!c.Y) return fail(r.null_y);
    if (r.weighted && (rc = weights_check_args(c.ctx, c.who, r.W, r.w_stride, c.err, c.errlen)) != SS_HIP_OK) return rc;
    if (r.own) return fail(r.own);
    if ((rc = check_out_aligned(c.who, c.records_out, c.err, c.errlen)) != SS_HIP_OK) return rc;
    if (r.flags & ~r.mask) return fail("unknown flag bit");
    if (r.nothing) return fail(r.nothing);
    if (c.incy <= 0 || c.y_stride <= 0 || (c.V && (c.rs <= 0 || c.cs <= 0))) return fail("increments and strides must be positive");
    if (c.B >= 0x80000000ull || (unsigned long long)c.B * c.kmax >= 0xffffffffull) return fail("B * kmax must stay below 2^32");
    if ((rc = check_overlap(c.who, c.records, c.records_out, c.B * record_bytes(c.kmax, sizeof(T)), c.err, c.errlen)) != SS_HIP_OK) return rc;
    empty = c.B == 0 || (c.cols && c.S == 0);               // (every argument above was checked all the same)
    if (!empty && c.cols && c.S > c.ctx->n) return fail("more columns than the dictionary has (a column is named twice)");
    return SS_HIP_OK;
}

// ---- the steps -------------------------------------------------------------------------------------------------------------------

// the list of atoms on a host copy (without one: every column, S = n), the shapes and where each pointer lives.  Nothing has been
// written when it fails
template <typename T>
int learn_atoms(LearnCall<T>& c)
{
    HIPCHK(hipSetDevice(c.ctx->device));
    c.m = c.ctx->m;
    c.n = c.ctx->n;
    c.rb = record_bytes(c.kmax, sizeof(T));
    c.ldm = c.ctx->ldm;
    c.ntiles = (uint32_t)((c.m + kClsTileRows - 1) / kClsTileRows);
    c.per = c.ntiles * 4u;
    if (c.cols) {
        c.hc.resize(c.S);
        if (on_device(c.cols)) HIPCHK(hipMemcpy(c.hc.data(), c.cols, c.S * sizeof(uint32_t), hipMemcpyDeviceToHost));
        else std::memcpy(c.hc.data(), c.cols, c.S * sizeof(uint32_t));
        std::vector<uint32_t> sorted(c.hc);
        std::sort(sorted.begin(), sorted.end());
        if (sorted.back() >= c.n) { set_err(c.err, c.errlen, std::string(c.who) + ": column index out of range"); return SS_HIP_EINVAL; }
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) {
            set_err(c.err, c.errlen, std::string(c.who) + ": a column is named twice");
            return SS_HIP_EINVAL;
        }
    } else {
        c.S = c.n;
    }
    c.place = RecordPlace(c.records, c.records_out, c.B * c.rb);
    c.y_dev = on_device(c.Y);
    c.v_dev = c.V != nullptr && on_device(c.V);
    return SS_HIP_OK;
}

// the bytes x.carve takes, then x carved out of the arena (grown to them)
template <typename X, typename T> size_t learn_bytes(X& x, const LearnCall<T>& c) { return carve_into(nullptr, x, c); }
template <typename X, typename T>
void learn_carve(WorkArena& a, X& x, const LearnCall<T>& c, const char* what)
{
    grow(a, learn_bytes(x, c), what);
    carve_into(a.buf, x, c);
}

// the index's common pieces.  A unit's struct derives from it and states carve(): head, its own partial sums, tail
template <typename T> struct LearnIndex {
    unsigned char* stage;              // a host caller's records, in and out
    uint32_t *slot_of, *dcols, *counts, *off, *bad;
    double *part, *sig, *obj;
    T* s2;
    uint32_t *dusage, *sel;
    void head(Carver& cv, const LearnCall<T>& c, size_t nobj)
    {
        stage = c.place.carve(cv);
        slot_of = c.cols ? cv.take<uint32_t>(c.n) : nullptr;
        dcols = c.cols ? cv.take<uint32_t>(c.S) : nullptr;
        counts = cv.take<uint32_t>(c.S);
        off = cv.take<uint32_t>(c.S + 2);                 // (+ the total, + the longest list)
        bad = cv.take<uint32_t>(1);
        part = cv.take<double>(c.B * c.per);
        sig = cv.take<double>(c.B);
        obj = cv.take<double>(nobj);
        s2 = cv.take<T>(c.S);
    }
    void tail(Carver& cv, const LearnCall<T>& c)
    {
        dusage = cv.take<uint32_t>(c.S);
        sel = cv.take<uint32_t>(2 * c.S);                 // apply: positions of the changed atoms, then their columns
    }
};

// the workspace's common pieces: the lists in front of a unit's blocks, a host caller's signals ([rows][m]) behind them
template <typename T> struct LearnWork {
    uint32_t *pair_b, *pair_e, *sb;
    T *sw, *ybuf;
    void lists(Carver& cv, const LearnCall<T>& c)
    {
        pair_b = cv.take<uint32_t>(c.total);
        pair_e = cv.take<uint32_t>(c.total);
        sb = cv.take<uint32_t>(c.total);
        sw = cv.take<T>(c.total);
    }
    void signals(Carver& cv, const LearnCall<T>& c, size_t rows) { ybuf = c.y_dev ? nullptr : cv.take<T>(rows * c.m); }
};

// a host caller's records staged, the slot map and the columns uploaded, the counts and offsets; then the one read-back: is a record
// invalid (nothing has been written then), how long are the lists
template <typename T>
int learn_open(LearnCall<T>& c, const LearnIndex<T>& ix)
{
    hipStream_t st = c.ctx->stream;
    c.place.stage_in(ix.stage, st);
    if (c.cols) {
        c.slots.assign(c.n, kDlNone);
        for (size_t s = 0; s < c.S; ++s) c.slots[c.hc[s]] = (uint32_t)s;
        HIPCHK(hipMemcpyAsync(ix.slot_of, c.slots.data(), c.n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(ix.dcols, c.hc.data(), c.S * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    }
    HIPCHK(dl_launch_count(c.ctx, c.place.din, c.rb, c.kmax, (uint32_t)c.B, ix.slot_of, (uint32_t)c.S, ix.counts, ix.off, ix.bad));
    uint32_t first_bad, tail[2] = { 0u, 0u };
    flag_fetch(&first_bad, ix.bad, st, 1, tail, ix.off + c.S, sizeof(tail));
    c.total = tail[0];
    c.longest = tail[1];
    return first_bad != kNoRecord ? bad_index(first_bad, c.who, c.err, c.errlen) : SS_HIP_OK;
}

// the signals whose residuals a chunked call holds at once: the byte budget, kDlChunkMax, the dl_chunk_max option
template <typename T>
size_t learn_chunk(const LearnCall<T>& c)
{
    size_t chunk = std::max<size_t>(1, std::min<size_t>(kDlChunkMax, kDlChunkBytes / ((size_t)c.ldm * sizeof(T))));
    if (c.ctx->dl_chunk_max > 0) chunk = std::min<size_t>(chunk, (size_t)c.ctx->dl_chunk_max);
    return std::min(chunk, c.B);
}

// where a call's last kernel left the atoms: (i, s) at p[i * rs + s * cs].  learn_out: straight in a device V, else in the [S][ldm] block
template <typename T> struct LearnOut { T* p; long long rs, cs; };
template <typename T>
LearnOut<T> learn_out(const LearnCall<T>& c, T* block)
{
    return c.v_dev ? LearnOut<T>{ c.V, (long long)c.rs, (long long)c.cs } : LearnOut<T>{ block, 1ll, (long long)c.ldm };
}

// the copies out (nobj words of the objective; a host V from `block`, [S][ldm]), the final synchronise; with apply the changed atoms
// of `out` as a device column list + a contiguous device V, through the column replacement
template <typename T>
int learn_finish(const LearnCall<T>& c, const LearnIndex<T>& ix, size_t nobj, const T* block, const LearnOut<T>& out)
{
    hipStream_t st = c.ctx->stream;
    const size_t m = c.m, S = c.S;
    if (c.objective) HIPCHK(hipMemcpyAsync(c.objective, ix.obj, nobj * sizeof(double), hipMemcpyDefault, st));
    if (c.usage) HIPCHK(hipMemcpyAsync(c.usage, ix.dusage, S * sizeof(uint32_t), hipMemcpyDefault, st));
    std::vector<uint32_t> hus;
    if (c.apply) {
        hus.resize(S);
        HIPCHK(hipMemcpyAsync(hus.data(), ix.dusage, S * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    }
    c.place.copy_out(ix.stage, st);
    if (c.V && !c.v_dev) {
        std::vector<T> tmp(S * m);
        HIPCHK(hipMemcpy2DAsync(tmp.data(), m * sizeof(T), block, (size_t)c.ldm * sizeof(T), m * sizeof(T), S, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (size_t s = 0; s < S; ++s)
            for (size_t i = 0; i < m; ++i) c.V[(ptrdiff_t)i * c.rs + (ptrdiff_t)s * c.cs] = tmp[s * m + i];
    }
    HIPCHK(hipStreamSynchronize(st));
    if (!c.apply) return SS_HIP_OK;
    std::vector<uint32_t> pos, ccols;
    for (size_t s = 0; s < S; ++s)
        if (hus[s] != 0u && (hus[s] & kDlLeft) == 0u) { pos.push_back((uint32_t)s); ccols.push_back(c.cols ? c.hc[s] : (uint32_t)s); }
    if (pos.empty()) return SS_HIP_OK;
    const size_t nc = pos.size();
    WorkArena& vc = learn_arena(c.ctx).vc;
    grow(vc, nc * m * sizeof(T), "hipMalloc(atom learning: changed atoms)");
    T* Vc = reinterpret_cast<T*>(vc.buf);
    HIPCHK(hipMemcpyAsync(ix.sel, pos.data(), nc * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ix.sel + S, ccols.data(), nc * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIPCHK(dl_launch_gather<T>(c.ctx, (const T*)out.p, out.rs, out.cs, (const uint32_t*)ix.sel, (uint32_t)nc, Vc));
    HIPCHK(hipStreamSynchronize(st));
    return replace_columns_device<T>(c.ctx, ix.sel + S, ccols, Vc, 1ll, (long long)m, c.err, c.errlen);
}

}  // namespace

}  // namespace sship
