// What the translation units that read compact records share (classify.hip, dictlearn.hip): the 1024-row register tile of the
// streaming kernels and its fixed reduction order, a record's values read and written, the entry points' common checks, and the host
// helpers around a chunked workspace (grow, Carver, upload_rows).  Errors, pointers and the record's size come from host_common.h.
// Everything sits in an unnamed namespace: each unit gets its own copy, nothing here is part of the library's link surface.
#pragma once

#include "host_common.h"

#include <string>
#include <vector>

namespace sship {

namespace {

constexpr uint32_t kClsThreads = 256;
constexpr uint32_t kClsTileRows = 1024;                  // rows of y a workgroup holds: four per thread
constexpr uint32_t kClsInFlight = 8;                     // columns whose loads a thread has in flight

inline void grow(unsigned char*& p, size_t& have, size_t need, const char* what)
{
    if (have >= need) return;
    if (p) HIPCHK(hipFree(p));
    p = nullptr;
    have = 0;
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), need);
    if (e != hipSuccess) { p = nullptr; throw HipFail{ e, what }; }
    have = need;
}

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

}  // namespace

}  // namespace sship
