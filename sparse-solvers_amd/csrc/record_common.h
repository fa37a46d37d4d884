// What the units that read compact records share (classify.hip, refit.hip, topcorr.hip, joint.hip, the learners; tc_driver.h and
// learn_driver.h include it): the 1024-row register tile of the streaming kernels and its fixed reduction order, a record's values read
// and written, its index check on the device, the entry points' common checks and repeated clauses (check_*), and the host steps a record
// call runs between its own launches, each stated once: a workspace grown and carved into the call's named pieces (grow, Carver,
// carve_into), where the records live (RecordPlace), the bad-record flag (flag_*), a chunk's signals (chunk_signals, upload_rows).  Errors
// and pointers come from host_common.h.  Unnamed namespace: each unit gets its own copy, nothing here is part of the library's link surface.
#pragma once

#include "host_common.h"

#include <string>
#include <vector>

namespace sship {

namespace {

constexpr uint32_t kClsThreads = 256;
constexpr uint32_t kClsTileRows = 1024;                  // rows of y a workgroup holds: four per thread
constexpr uint32_t kClsInFlight = 8;                     // columns whose loads a thread has in flight

inline void grow(Holdings& own, unsigned char*& p, size_t& have, size_t need, const char* what)
{
    if (have >= need) return;
    HIPCHK(own.drop(p));
    have = 0;
    held(own.device(&p, need), what);
    have = need;
}

inline void grow(WorkArena& a, size_t need, const char* what) { grow(a.own, a.buf, a.bytes, need, what); }

// carves 256-byte aligned pieces out of the arena; with base == nullptr it only adds up
struct Carver {
    unsigned char* base;
    size_t off = 0;
    explicit Carver(unsigned char* b) : base(b) {}
    template <typename P> P* take(size_t count)
    {
        P* p = base ? reinterpret_cast<P*>(base + off) : nullptr;
        off += (count * sizeof(P) + 255) & ~(size_t)255;
        return p;
    }
};

// a call's pieces are the members of a struct x with x.carve(Carver&, args...): carved at `base` (nullptr: only sized) -> their bytes
template <typename X, typename... A> size_t carve_into(unsigned char* base, X& x, const A&... a)
{
    Carver cv(base);
    x.carve(cv, a...);
    return cv.off;
}

// (the values of a fp64 record sit at 16 + 4 kmax: 4-byte aligned only when kmax is odd)
__device__ inline float load_val(const unsigned char* p, uint32_t e, float) { return reinterpret_cast<const float*>(p)[e]; }
__device__ inline double load_val(const unsigned char* p, uint32_t e, double)
{
    const uint32_t* w = reinterpret_cast<const uint32_t*>(p) + 2u * e;
    return __longlong_as_double((long long)(((unsigned long long)w[1] << 32) | w[0]));
}

__device__ inline void store_val(unsigned char* p, uint32_t e, float v) { reinterpret_cast<float*>(p)[e] = v; }
__device__ inline void store_val(unsigned char* p, uint32_t e, double v)
{
    uint32_t* w = reinterpret_cast<uint32_t*>(p) + 2u * e;
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    w[0] = (uint32_t)u;
    w[1] = (uint32_t)(u >> 32);
}

template <typename T> struct ClsVec;
template <> struct ClsVec<float> { typedef float4 type; static constexpr uint32_t W = 4, L = 1; };
template <> struct ClsVec<double> { typedef double2 type; static constexpr uint32_t W = 2, L = 2; };
__device__ inline float vget(const float4& v, uint32_t e) { return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }
__device__ inline double vget(const double2& v, uint32_t e) { return e == 0 ? v.x : v.y; }

// a thread's W values of the register tile: stored as one vector at dst (16-byte aligned), or as the vector itself.  cls_store packs
// into a local that it then copies out: in that form the compiler keeps the pair / quad as one vector up to a single 16-byte store
template <typename T> __device__ inline void cls_store(T* dst, const T* d)
{
    typename ClsVec<T>::type out;
    if constexpr (sizeof(T) == 4) out = typename ClsVec<T>::type{ d[0], d[1], d[2], d[3] };
    else out = typename ClsVec<T>::type{ d[0], d[1] };
    *reinterpret_cast<typename ClsVec<T>::type*>(dst) = out;
}
template <typename T> __device__ inline typename ClsVec<T>::type cls_pack(const T* d)
{
    typename ClsVec<T>::type out;
    cls_store<T>(reinterpret_cast<T*>(&out), d);
    return out;
}

// a stored index >= n of the record at r (Krec: its word 0) puts b into *bad; the workgroup's 64 lanes stride over them, none is an address
__device__ inline void rec_check_indices(const unsigned char* r, uint32_t Krec, uint32_t kmax, uint32_t n, uint32_t b, uint32_t* bad)
{
    const uint32_t K = Krec < kmax ? Krec : kmax;
    const uint32_t* idx = reinterpret_cast<const uint32_t*>(r + 16);
    for (uint32_t e = threadIdx.x; e < K; e += 64u)
        if (idx[e] >= n) atomicMin(bad, b);
}

// the atom learners' words (dictlearn.hip, ksvd.hip, wdictlearn.hip): a column that is not requested; the usage bit of an atom that
// had users but was left as it is; the first position in sb[lo .. hi) whose signal is >= b (an atom's list is ascending)
constexpr uint32_t kDlNone = 0xffffffffu;
constexpr uint32_t kDlLeft = 0x80000000u;
__device__ inline uint32_t dl_lower_bound(const uint32_t* __restrict__ sb, uint32_t lo, uint32_t hi, uint32_t b)
{
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (sb[mid] < b) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

__device__ inline double wave_sum(double s)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    return s;
}

// the checks the record entry points share, in the order they are reported
template <typename T>
int check_common(const ss_hip_ctx* ctx, const char* who, const void* records, bool need_records, uint32_t kmax, char* err, size_t errlen)
{
    const std::string w(who);
    if (!ctx) { set_err(err, errlen, w + ": null context"); return SS_HIP_EINVAL; }
    if (ctx->kind != 0) { set_err(err, errlen, w + ": this context was created for IRLS"); return SS_HIP_EINVAL; }
    if (ctx->colshard != nullptr) { set_err(err, errlen, w + ": not available on a column-sharded context"); return SS_HIP_EINVAL; }
    if (ctx->is_f64 != (sizeof(T) == 8)) { set_err(err, errlen, w + ": element type mismatch"); return SS_HIP_ETYPE; }
    if (need_records && !records) { set_err(err, errlen, w + ": records must not be null"); return SS_HIP_EINVAL; }
    if (kmax == 0 || kmax > kKcapLimit || (reinterpret_cast<uintptr_t>(records) & 7u)) {
        set_err(err, errlen, w + ": kmax must be 1..4096 and records 8-byte aligned");
        return SS_HIP_EINVAL;
    }
    return SS_HIP_OK;
}

// the clauses several entry points repeat, each called at the position where that call reports it
inline int clause(bool broken, const char* who, const char* text, char* err, size_t errlen)
{
    if (broken) set_err(err, errlen, std::string(who) + ": " + text);
    return broken ? SS_HIP_EINVAL : SS_HIP_OK;
}
inline int check_out_aligned(const char* who, const void* out, char* err, size_t errlen) { return clause(reinterpret_cast<uintptr_t>(out) & 7u, who, "records_out must be 8-byte aligned", err, errlen); }
inline int check_overlap(const char* who, const void* records, const void* out, size_t bytes, char* err, size_t errlen)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(records), b = reinterpret_cast<uintptr_t>(out);     // (out null or the records themselves: fine)
    return clause(b && b != a && a < b + bytes && b < a + bytes, who, "records and records_out overlap in part", err, errlen);
}
inline int check_batch(const char* who, size_t B, char* err, size_t errlen) { return clause(B >= 0x80000000ull, who, "B must stay below 2^31", err, errlen); }
inline int check_r_stride(const char* who, const void* R, ptrdiff_t r_stride, uint32_t C, char* err, size_t errlen)
{
    return clause(R && r_stride < (ptrdiff_t)C, who, "r_stride must be at least num_classes", err, errlen);
}

inline int bad_index(uint32_t first_bad, const char* who, char* err, size_t errlen)
{
    set_err(err, errlen, std::string(who) + ": record " + std::to_string(first_bad) + " holds a column index >= n");
    return SS_HIP_EINVAL;
}

// rows b0 .. b0 + Bc - 1 of a HOST matrix (row stride / increment in elements) into dst [Bc][m], contiguous
template <typename T>
void upload_rows(ss_hip_ctx* ctx, T* dst, const T* src, ptrdiff_t stride, ptrdiff_t inc, size_t b0, size_t Bc, std::vector<T>& tmp)
{
    const size_t m = ctx->m;
    if (inc == 1 && stride >= (ptrdiff_t)m) {
        HIPCHK(hipMemcpy2DAsync(dst, m * sizeof(T), src + (ptrdiff_t)b0 * stride, (size_t)stride * sizeof(T), m * sizeof(T), Bc,
                                hipMemcpyHostToDevice, ctx->stream));
        return;
    }
    tmp.resize(Bc * m);
    for (size_t b = 0; b < Bc; ++b)
        for (size_t i = 0; i < m; ++i) tmp[b * m + i] = src[(ptrdiff_t)(b0 + b) * stride + (ptrdiff_t)i * inc];
    HIPCHK(hipMemcpyAsync(dst, tmp.data(), Bc * m * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));        // (tmp is filled again for the next chunk)
}

// Where a call's records live on the device.  din: the input records there; dout: where the output records are written there.  A
// host caller's records are staged and written in place when the input is staged too: one staging of `bytes` serves both.  in null:
// the call reads no records; out null: it writes none
struct RecordPlace {
    const void* in = nullptr;
    void* out = nullptr;
    size_t bytes = 0;
    bool in_dev = false, out_dev = false;
    const unsigned char* din = nullptr;
    unsigned char* dout = nullptr;
    explicit RecordPlace(const void* records = nullptr, void* records_out = nullptr, size_t nbytes = 0)
        : in(records), out(records_out), bytes(nbytes), in_dev(records && on_device(records)), out_dev(records_out && on_device(records_out)) {}
    unsigned char* carve(Carver& cv) const { return (in && !in_dev) || (out && !out_dev) ? cv.take<unsigned char>(bytes) : nullptr; }
    void stage_in(unsigned char* stage, hipStream_t st)
    {
        din = static_cast<const unsigned char*>(in);
        if (in && !in_dev) { HIPCHK(hipMemcpyAsync(stage, in, bytes, hipMemcpyHostToDevice, st)); din = stage; }
        dout = !out ? nullptr : out_dev ? static_cast<unsigned char*>(out) : stage;
    }
    void copy_out(const unsigned char* stage, hipStream_t st) const { if (out && !out_dev) HIPCHK(hipMemcpyAsync(out, stage, bytes, hipMemcpyDeviceToHost, st)); }
};

// The bad-record flag: words a check kernel lowers by atomicMin (kNoRecord: nothing found), armed in front of the launches; fetched
// behind them with the stream synchronised (also_*: a second read-back that rides the same synchronise); a call's verdict from one word
constexpr uint32_t kNoRecord = 0xffffffffu;
inline void flag_arm(uint32_t* bad, hipStream_t st, size_t words = 1) { HIPCHK(hipMemsetAsync(bad, 0xff, words * sizeof(uint32_t), st)); }
inline void flag_fetch(uint32_t* out, const uint32_t* bad, hipStream_t st, size_t words = 1, void* also_dst = nullptr, const void* also_src = nullptr,
                       size_t also_bytes = 0)
{
    HIPCHK(hipMemcpyAsync(out, bad, words * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (also_dst) HIPCHK(hipMemcpyAsync(also_dst, also_src, also_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
}

inline int flag_verdict(const uint32_t* bad, hipStream_t st, const char* who, char* err, size_t errlen)
{
    uint32_t first_bad;
    flag_fetch(&first_bad, bad, st);
    return first_bad != kNoRecord ? bad_index(first_bad, who, err, errlen) : SS_HIP_OK;
}

// the signals [b0, b0 + Bc) where the kernels read them: the caller's on the device, or uploaded into ybuf ([Bc][m], contiguous)
template <typename T> struct ChunkSignals { const T* yd; long long ys, yi; };
template <typename T>
ChunkSignals<T> chunk_signals(ss_hip_ctx* ctx, const T* Y, ptrdiff_t y_stride, ptrdiff_t incy, bool y_dev, T* ybuf, size_t b0, size_t Bc, std::vector<T>& tmp)
{
    if (y_dev) return { Y + (ptrdiff_t)b0 * y_stride, (long long)y_stride, (long long)incy };
    upload_rows<T>(ctx, ybuf, Y, y_stride, incy, b0, Bc, tmp);
    return { ybuf, (long long)ctx->m, 1ll };
}

}  // namespace

}  // namespace sship
