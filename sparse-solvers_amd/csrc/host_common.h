// The host side every C-ABI entry point has around its kernels, stated once: a failed HIP call as an exception and as the C-ABI's
// status + message, where a caller's pointer lives, the size of a compact record, the owner of a call's scratch allocation, the owner
// of what a context keeps.  Host code only.  Everything but Holdings sits in an unnamed namespace: each unit gets its own copy;
// Holdings is a member of types the units share, so it is one type with hidden visibility.  Nothing here is part of the library's
// link surface.  (ss_hip_internal.h includes this header: it needs nothing from there.)
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "ss_hip.h"

namespace sship {

// msg into the caller's buffer, cut to errlen - 1 characters and always terminated; a null or empty buffer is left alone (homotopy.hip)
void set_err(char* err, size_t errlen, const std::string& msg);

// Owner of what lives as long as a CONTEXT or one of its parts: device memory, pinned host memory, events and streams.  It remembers
// what it handed out and gives all of it back in release() or its destructor — memory first, then events, then streams, each kind
// in the reverse of the order it was taken — so whoever allocates has nothing else to write down.  The pointers themselves stay
// with their structs (kernels and launchers read them); drop() frees one of them early, for a buffer that regrows.  The takes return
// the runtime's error, leave the pointer null on failure and clear the runtime's sticky error; held_* below are the throwing takes.
#pragma GCC visibility push(hidden)
class Holdings {
public:
    Holdings() = default;
    Holdings(const Holdings&) = delete;
    Holdings& operator=(const Holdings&) = delete;
    Holdings(Holdings&& o) noexcept : held_(std::move(o.held_)) { o.held_.clear(); }
    Holdings& operator=(Holdings&& o) noexcept { if (this != &o) { release(); held_ = std::move(o.held_); o.held_.clear(); } return *this; }
    ~Holdings() { release(); }

    template <typename P> hipError_t device(P** p, size_t bytes) { return keep(p, Device, hipMalloc(reinterpret_cast<void**>(p), bytes)); }
    template <typename P> hipError_t pinned(P** p, size_t bytes, unsigned flags) { return keep(p, Pinned, hipHostMalloc(reinterpret_cast<void**>(p), bytes, flags)); }
    hipError_t event(hipEvent_t* e) { return keep(e, Event, hipEventCreate(e)); }
    hipError_t event(hipEvent_t* e, unsigned flags) { return keep(e, Event, hipEventCreateWithFlags(e, flags)); }
    hipError_t stream(hipStream_t* s, unsigned flags) { return keep(s, Stream, hipStreamCreateWithFlags(s, flags)); }
    hipError_t stream(hipStream_t* s, unsigned flags, int priority) { return keep(s, Stream, hipStreamCreateWithPriority(s, flags, priority)); }
    // device memory somebody else obtained (the reserve thread's allocation, after the join)
    void adopt_device(void* p) { if (p) held_.push_back({ p, Device }); }

    // gives one of them back now and nulls the caller's pointer; a null pointer is nobody's
    template <typename P> hipError_t drop(P*& p)
    {
        hipError_t e = hipSuccess;
        for (size_t i = held_.size(); i-- > 0;)
            if (held_[i].h == static_cast<void*>(p) && p != nullptr) { e = give_back(held_[i]); held_.erase(held_.begin() + (ptrdiff_t)i); break; }
        p = nullptr;
        return e;
    }
    void release()
    {
        for (Kind k : { Device, Event, Stream })
            for (size_t i = held_.size(); i-- > 0;)
                if (held_[i].kind == k || (k == Device && held_[i].kind == Pinned)) (void)give_back(held_[i]);
        held_.clear();
    }
    size_t size() const { return held_.size(); }

private:
    enum Kind : uint8_t { Device, Pinned, Event, Stream };
    struct Held { void* h; Kind kind; };
    template <typename H> hipError_t keep(H* h, Kind kind, hipError_t e)
    {
        if (e == hipSuccess) held_.push_back({ static_cast<void*>(*h), kind });
        else { (void)hipGetLastError(); *h = nullptr; }
        return e;
    }
    static hipError_t give_back(const Held& x)
    {
        switch (x.kind) {
        case Device: return hipFree(x.h);
        case Pinned: return hipHostFree(x.h);
        case Event:  return hipEventDestroy(static_cast<hipEvent_t>(x.h));
        default:     return hipStreamDestroy(static_cast<hipStream_t>(x.h));
        }
    }
    std::vector<Held> held_;
};
#pragma GCC visibility pop

namespace {

struct HipFail { hipError_t code; const char* what; };
#define HIPCHK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) throw sship::HipFail{ e_, #expr }; } while (0)

inline std::string hip_msg(const HipFail& f) { return std::string("HIP error: ") + hipGetErrorString(f.code) + " in " + f.what; }

// The throwing takes of a Holdings, named after the calls they make.  HELD(own, hipMalloc, &p, bytes) reports a failure with the text
// HIPCHK(hipMalloc(&p, bytes)) reported: "HIP error: ... in hipMalloc(&p, bytes)".
inline void held(hipError_t e, const char* what) { if (e != hipSuccess) throw HipFail{ e, what }; }
template <typename P> void held_hipMalloc(Holdings& own, P** p, size_t bytes, const char* what) { held(own.device(p, bytes), what); }
template <typename P> void held_hipHostMalloc(Holdings& own, P** p, size_t bytes, unsigned flags, const char* what) { held(own.pinned(p, bytes, flags), what); }
inline void held_hipEventCreate(Holdings& own, hipEvent_t* e, const char* what) { held(own.event(e), what); }
inline void held_hipEventCreateWithFlags(Holdings& own, hipEvent_t* e, unsigned flags, const char* what) { held(own.event(e, flags), what); }
inline void held_hipStreamCreateWithFlags(Holdings& own, hipStream_t* s, unsigned flags, const char* what) { held(own.stream(s, flags), what); }
// (stringified here, not in a helper macro: hipHostMallocMapped and its like are macros, and the text names them as the call did)
#define HELD(own, call, ...) sship::held_##call(own, __VA_ARGS__, #call "(" #__VA_ARGS__ ")")

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
