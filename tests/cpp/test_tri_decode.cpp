// Host program over csrc/tri_decode.h (tests/test_tri_decode.py builds and runs it): the tile pair (bm, bn), bm <= bn, that the
// symmetric Gram build's workgroup b works on, b = bn (bn + 1) / 2 + bm.  The kernel calls the same function; here it is held to
// the integer definition at every panel boundary the launcher admits (b < 2^31) and on a full sweep of the first 2^22 blocks.
// No kernel is launched.
#include "tri_decode.h"

#include <cstdint>
#include <cstdio>

static int g_failed = 0;

static void check(uint64_t b, uint32_t want_bm, uint32_t want_bn)
{
    uint32_t bm = 0xdeadbeefu, bn = 0xdeadbeefu;
    sship::tri_tile_decode((uint32_t)b, bm, bn);
    if (bm != want_bm || bn != want_bn) {
        if (g_failed < 20)
            std::printf("FAILED b = %llu: decoded (%u, %u), the definition gives (%u, %u)\n", (unsigned long long)b, bm, bn, want_bm, want_bn);
        g_failed += 1;
    }
}

int main()
{
    const uint64_t limit = 1ull << 31;            // launch_gemm_sym_f32 refuses more blocks than 2^31 - 1
    uint64_t boundaries = 0;

    // every panel t: the block before its first, its first (0, t), its last (t, t)
    for (uint64_t t = 0; t <= 65535; ++t) {
        const uint64_t first = t * (t + 1) / 2;
        if (t > 0 && first - 1 < limit) { check(first - 1, (uint32_t)(t - 1), (uint32_t)(t - 1)); boundaries += 1; }
        if (first < limit) { check(first, 0u, (uint32_t)t); boundaries += 1; }
        if (first + t < limit) { check(first + t, (uint32_t)t, (uint32_t)t); boundaries += 1; }
    }
    // ... and the largest block index a launch can carry
    {
        const uint64_t b = limit - 1;
        uint64_t t = 0;
        while ((t + 1) * (t + 2) / 2 <= b) ++t;
        check(b, (uint32_t)(b - t * (t + 1) / 2), (uint32_t)t);
        boundaries += 1;
    }

    // the first 2^22 blocks, against a count that walks the panels
    uint32_t bm = 0, bn = 0;
    for (uint64_t b = 0; b < (1ull << 22); ++b) {
        check(b, bm, bn);
        if (bm == bn) { bn += 1; bm = 0; } else bm += 1;
    }

    std::printf("boundaries checked %llu\n", (unsigned long long)boundaries);
    std::printf("sweep checked %llu\n", (unsigned long long)(1ull << 22));
    std::printf(g_failed ? "%d check(s) failed\n" : "all checks passed\n", g_failed);
    return g_failed ? 1 : 0;
}
