// Host program over csrc/host_common.h (tests/test_host_common.py builds and runs it): what guarded() returns and writes for
// everything a body can throw, set_err's truncation, on_device for host memory, record_bytes, and, where a device is visible, one
// DeviceBuf allocated, moved from and destroyed.  No kernel is launched and no allocation is sized to fail.
#include "host_common.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

using namespace sship;

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

    std::printf(g_failed ? "%d check(s) failed\n" : "all checks passed\n", g_failed);
    return g_failed ? 1 : 0;
}
