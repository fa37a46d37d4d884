// Host program over csrc/host_common.h (tests/test_host_common.py builds and runs it): what guarded() returns and writes for
// everything a body can throw, set_err's truncation, on_device for host memory, record_bytes, the text HELD makes, and, where a device
// is visible, one DeviceBuf allocated, moved from and destroyed and one Holdings that takes each kind, drops one, is moved from and
// released.  No kernel is launched and no allocation is sized to fail.
#include "host_common.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

using namespace sship;

// a "call" for HELD that takes nothing: it hands back the text the macro made for it
namespace sship { namespace {
inline void held_Probe(Holdings&, const char** out, const char* what) { *out = what; }
template <typename P> void held_Probe(Holdings&, const char** out, P**, size_t, unsigned, const char* what) { *out = what; }
} }

static int g_failed = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); g_failed += 1; } } while (0)

// one guarded() call around `body`: the status, and what it left in the message buffer
template <typename F>
static int run(std::string& msg, F&& body, int oom_status = -1)
{
    char buf[256] = "untouched";
    const int rc = oom_status == -1 ? guarded(buf, sizeof(buf), "prefix", body) : guarded(buf, sizeof(buf), "prefix", body, oom_status);
    msg = buf;
    return rc;
}

int main()
{
    std::string msg;

    // ---- guarded: the body's value untouched, nothing written, when nothing throws
    for (int v : { (int)SS_HIP_OK, (int)SS_HIP_EINVAL, (int)SS_HIP_ETYPE, 12345, -7 }) {
        CHECK(run(msg, [&] { return v; }) == v);
        CHECK(msg == "untouched");
        CHECK(run(msg, [&] { return v; }, SS_HIP_ERUNTIME) == v);
        CHECK(msg == "untouched");
    }

    // ---- guarded: out of device memory is `oom_status` (SS_HIP_ENOMEM unless said otherwise), with the one text
    CHECK(run(msg, []() -> int { throw HipFail{ hipErrorOutOfMemory, "X" }; }) == SS_HIP_ENOMEM);
    CHECK(msg == "HIP error: out of memory in X");
    CHECK(run(msg, []() -> int { throw HipFail{ hipErrorOutOfMemory, "X" }; }, SS_HIP_ERUNTIME) == SS_HIP_ERUNTIME);
    CHECK(msg == "HIP error: out of memory in X");
    CHECK(run(msg, []() -> int { throw HipFail{ hipErrorOutOfMemory, "X" }; }, SS_HIP_ENOMEM) == SS_HIP_ENOMEM);
    CHECK(msg == "HIP error: out of memory in X");
    // ... every other failed call is SS_HIP_ERUNTIME under either mapping
    CHECK(run(msg, []() -> int { throw HipFail{ hipErrorInvalidValue, "X" }; }) == SS_HIP_ERUNTIME);
    CHECK(msg == std::string("HIP error: ") + hipGetErrorString(hipErrorInvalidValue) + " in X");
    CHECK(run(msg, []() -> int { throw HipFail{ hipErrorInvalidValue, "X" }; }, SS_HIP_ERUNTIME) == SS_HIP_ERUNTIME);
    CHECK(msg == hip_msg(HipFail{ hipErrorInvalidValue, "X" }));
    // ... and the macro throws what it names
    CHECK(run(msg, []() -> int { HIPCHK(hipErrorInvalidValue); return SS_HIP_OK; }) == SS_HIP_ERUNTIME);
    CHECK(msg == std::string("HIP error: ") + hipGetErrorString(hipErrorInvalidValue) + " in hipErrorInvalidValue");
    CHECK(run(msg, []() -> int { HIPCHK(hipSuccess); return 77; }) == 77);
    // ---- guarded: out of host memory is SS_HIP_ENOMEM under either mapping
    CHECK(run(msg, []() -> int { throw std::bad_alloc(); }) == SS_HIP_ENOMEM);
    CHECK(msg == "prefix: out of host memory");
    CHECK(run(msg, []() -> int { throw std::bad_alloc(); }, SS_HIP_ERUNTIME) == SS_HIP_ENOMEM);
    CHECK(msg == "prefix: out of host memory");
    // ... also with no buffer to write to
    CHECK(guarded(nullptr, 0, "prefix", []() -> int { throw HipFail{ hipErrorOutOfMemory, "X" }; }) == SS_HIP_ENOMEM);

    // ---- set_err: truncates to errlen - 1, always terminates, leaves a null or empty buffer alone
    {
        const std::string text = "0123456789";
        for (size_t len = 1; len <= 12; ++len) {
            char buf[16];
            std::memset(buf, '#', sizeof(buf));
            set_err(buf, len, text);
            const size_t k = len - 1 < text.size() ? len - 1 : text.size();
            CHECK(buf[k] == '\0');
            CHECK(std::memcmp(buf, text.data(), k) == 0);
            for (size_t i = k + 1; i < sizeof(buf); ++i) CHECK(buf[i] == '#');
        }
        char buf[4] = { '#', '#', '#', '#' };
        set_err(buf, 0, text);
        CHECK(std::memcmp(buf, "####", 4) == 0);
        set_err(nullptr, 16, text);
        set_err(nullptr, 0, text);
    }

    // ---- on_device: memory the runtime does not know is the host's
    {
        int on_stack = 0;
        CHECK(!on_device(&on_stack));
        void* heap = std::malloc(4096);
        CHECK(heap != nullptr && !on_device(heap));
        std::free(heap);
        CHECK(!on_device(&on_stack));       // (the first answer left no error behind that would change the second)
    }

    // ---- record_bytes: 16 bytes of header, kmax indices and values, padded to 8
    for (uint32_t kmax : { 1u, 2u, 3u, 96u, 4096u })
        for (size_t elem : { (size_t)4, (size_t)8 }) {
            CHECK(record_bytes(kmax, elem) == ((16 + (size_t)kmax * (4 + elem) + 7) & ~(size_t)7));
            CHECK(record_bytes(kmax, elem) == ss_hip_record_bytes(kmax, elem == 8));
            std::printf("record_bytes %u %zu %zu\n", kmax, elem, record_bytes(kmax, elem));
        }

    // ---- DeviceBuf: needs a device
    if (ss_hip_device_count() > 0) {
        {
            DeviceBuf a;
            CHECK(a.get<char>() == nullptr);
            a.alloc(1024, "test buffer");
            char* p = a.get<char>();
            CHECK(p != nullptr && on_device(p));
            DeviceBuf b(std::move(a));
            CHECK(a.get<char>() == nullptr);
            CHECK(b.get<char>() == p);
        }
        CHECK(hipGetLastError() == hipSuccess);
        std::printf("DeviceBuf: checked\n");
    } else {
        std::printf("DeviceBuf: skipped (no HIP device)\n");
    }

    // ---- Holdings: nothing to take is nothing held; the rest needs a device
    {
        Holdings none;
        CHECK(none.size() == 0);
        int* p = nullptr;
        CHECK(none.drop(p) == hipSuccess && p == nullptr);      // a null pointer is nobody's
        none.release();
        CHECK(none.size() == 0);
    }
    if (ss_hip_device_count() > 0) {
        {
            Holdings own;
            float* d0 = nullptr; unsigned char* d1 = nullptr; uint32_t* pin = nullptr;
            hipEvent_t e0 = nullptr, e1 = nullptr;
            hipStream_t s0 = nullptr, s1 = nullptr;
            // the non-throwing takes, one of each kind
            CHECK(own.device(&d0, 1024) == hipSuccess && d0 != nullptr && on_device(d0));
            CHECK(own.pinned(&pin, 256, hipHostMallocDefault) == hipSuccess && pin != nullptr);
            CHECK(own.event(&e0) == hipSuccess && e0 != nullptr);
            CHECK(own.event(&e1, hipEventDisableTiming) == hipSuccess && e1 != nullptr);
            CHECK(own.stream(&s0, hipStreamNonBlocking) == hipSuccess && s0 != nullptr);
            CHECK(own.stream(&s1, hipStreamNonBlocking, 0) == hipSuccess && s1 != nullptr);
            CHECK(own.size() == 6);
            // the throwing takes through the macro: they take, and a failure would carry the call's text
            CHECK(run(msg, [&]() -> int { HELD(own, hipMalloc, &d1, 4096); return 5; }) == 5);
            CHECK(d1 != nullptr && own.size() == 7);
            pin[0] = 7u;
            CHECK(hipMemcpyAsync(d0, pin, 4, hipMemcpyHostToDevice, s0) == hipSuccess && hipEventRecord(e0, s0) == hipSuccess);
            CHECK(hipEventSynchronize(e0) == hipSuccess);
            // drop of one (the pointer is nulled, the rest stays), of one it does not hold (nothing happens)
            CHECK(own.drop(d0) == hipSuccess && d0 == nullptr && own.size() == 6);
            int on_stack = 0;
            int* stranger = &on_stack;
            CHECK(own.drop(stranger) == hipSuccess && stranger == nullptr && own.size() == 6);
            CHECK(own.drop(e1) == hipSuccess && e1 == nullptr && own.size() == 5);
            // moved from: holds nothing; the new owner holds all of it
            Holdings heir(std::move(own));
            CHECK(own.size() == 0 && heir.size() == 5);
            own.release();
            Holdings third;
            third = std::move(heir);
            CHECK(heir.size() == 0 && third.size() == 5);
            // released: holds nothing, and may be released again and used again
            third.release();
            CHECK(third.size() == 0);
            third.release();
            CHECK(third.device(&d0, 64) == hipSuccess && third.size() == 1);
        }
        CHECK(hipGetLastError() == hipSuccess);
        CHECK(std::string(hip_msg(HipFail{ hipErrorOutOfMemory, "hipMalloc(&p, bytes)" })) == "HIP error: out of memory in hipMalloc(&p, bytes)");
        std::printf("Holdings: checked\n");
    } else {
        std::printf("Holdings: skipped (no HIP device)\n");
    }
    // the macro's text is the text of the call it stands for (no device needed: the take is never made)
    {
        Holdings own;
        struct { uint32_t* host_flags = nullptr; } c, *ctx = &c;
        const char* text = nullptr;
        HELD(own, Probe, &text, &ctx->host_flags, 64 * sizeof(uint32_t), hipHostMallocMapped);
        CHECK(std::string(text) == "Probe(&text, &ctx->host_flags, 64 * sizeof(uint32_t), hipHostMallocMapped)");
        HELD(own, Probe, &text);
        CHECK(std::string(text) == "Probe(&text)");
        CHECK(own.size() == 0);
    }

    std::printf(g_failed ? "%d check(s) failed\n" : "all checks passed\n", g_failed);
    return g_failed ? 1 : 0;
}
