// The host side every C-ABI entry point has around its kernels, stated once: a failed HIP call as an exception and as the C-ABI's
// status + message, where a caller's pointer lives, the size of a compact record, the owner of a call's scratch allocation.
// Host code only.  Everything sits in an unnamed namespace: each unit gets its own copy, nothing here is part of the library's link surface.
#pragma once

#include "ss_hip_internal.h"

#include <cstring>
#include <new>
#include <string>

namespace sship {

namespace {

struct HipFail { hipError_t code; const char* what; };
#define HIPCHK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) throw sship::HipFail{ e_, #expr }; } while (0)

inline std::string hip_msg(const HipFail& f) { return std::string("HIP error: ") + hipGetErrorString(f.code) + " in " + f.what; }

// Runs `body` (which returns a status) and turns what it throws into the C-ABI's codes: a failed HIP call (HIPCHK) into its text and
// SS_HIP_ERUNTIME — `oom_status` when the call ran out of device memory — and std::bad_alloc into "<prefix>: out of host memory"
// and SS_HIP_ENOMEM.  The runtime's sticky error is cleared: the next call starts clean.
template <typename F>
int guarded(char* err, size_t errlen, const char* prefix, F&& body, int oom_status = SS_HIP_ENOMEM)
{
    try {
        return body();
    } catch (const HipFail& f) {
        (void)hipGetLastError();
        set_err(err, errlen, hip_msg(f));
        return f.code == hipErrorOutOfMemory ? oom_status : SS_HIP_ERUNTIME;
    } catch (const std::bad_alloc&) {
        set_err(err, errlen, std::string(prefix) + ": out of host memory");
        return SS_HIP_ENOMEM;
    }
}

// true for device, managed and unified memory; memory the runtime does not know is the host's
inline bool on_device(const void* p)
{
    hipPointerAttribute_t attr;
    std::memset(&attr, 0, sizeof(attr));
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();       // unregistered host memory: clear the sticky error
        return false;
    }
    return attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged || attr.type == hipMemoryTypeUnified;
}

// compact record (include/ss_hip.h): u32 K, u32 iter, f64 err, u32 idx[kmax], T val[kmax], padded to 8 bytes
inline size_t record_bytes(uint32_t kmax, size_t elem) { return (16 + (size_t)kmax * (4 + elem) + 7) & ~(size_t)7; }

// Owner of one hipMalloc allocation for the length of a CALL: declare it outside the scope that synchronises the stream, so the
// memory is freed after the call's last synchronisation or on its way out with an error.  Not for anything a context keeps.
class DeviceBuf {
public:
    DeviceBuf() = default;
    DeviceBuf(DeviceBuf&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    DeviceBuf& operator=(DeviceBuf&&) = delete;
    ~DeviceBuf() { reset(); }

    // `what`: the text a failure reports ("HIP error: out of memory in <what>").  Where a caller passes the text of a hipMalloc call,
    // that is the message its entry point reported when it still made the call through HIPCHK: callers match on these texts.
    void alloc(size_t bytes, const char* what)
    {
        reset();
        const hipError_t e = hipMalloc(&p_, bytes);
        if (e != hipSuccess) { p_ = nullptr; throw HipFail{ e, what }; }
    }
    template <typename T> T* get() const { return static_cast<T*>(p_); }

private:
    void reset() { if (p_) (void)hipFree(p_); p_ = nullptr; }
    void* p_ = nullptr;
};

}  // namespace

}  // namespace sship
