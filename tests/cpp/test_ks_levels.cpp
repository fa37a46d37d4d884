// Host program over sparse-solvers_amd/csrc/ks_levels.h (the level schedule of the K-SVD sweep): random atom -> user lists, then the
// four properties tests/test_ks_levels.py names.  No HIP call, no kernel.
#include "ks_levels.h"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

struct Lists { std::vector<uint32_t> off, sb; size_t S, B; };

// S atoms over B signals; every atom's users ascending and distinct; `empty` of every 8 atoms have none; atom 0 may hold every signal
static Lists make(std::mt19937& rng, size_t S, size_t B, unsigned density, bool popular)
{
    Lists L;
    L.S = S;
    L.B = B;
    L.off.assign(S + 1, 0u);
    for (size_t s = 0; s < S; ++s) {
        L.off[s] = (uint32_t)L.sb.size();
        if (B == 0 || rng() % 8u == 0u) continue;
        for (size_t b = 0; b < B; ++b)
            if ((popular && s == S / 2) || rng() % 1000u < density) L.sb.push_back((uint32_t)b);
    }
    L.off[S] = (uint32_t)L.sb.size();
    return L;
}

static bool share(const Lists& L, size_t s, size_t t)
{
    uint32_t p = L.off[s], q = L.off[t];
    while (p < L.off[s + 1] && q < L.off[t + 1]) {
        if (L.sb[p] == L.sb[q]) return true;
        if (L.sb[p] < L.sb[q]) ++p; else ++q;
    }
    return false;
}

int main()
{
    std::mt19937 rng(20241);
    size_t cases = 0, atoms = 0, pairs = 0, userless = 0;
    const size_t shapes[][2] = { { 0, 0 }, { 1, 1 }, { 1, 0 }, { 7, 3 }, { 40, 25 }, { 200, 600 }, { 64, 1 }, { 150, 90 } };
    const unsigned densities[] = { 0u, 5u, 40u, 300u, 1000u };
    for (const auto& shp : shapes)
        for (unsigned d : densities)
            for (int popular = 0; popular < 2; ++popular) {
                const Lists L = make(rng, shp[0], shp[1], d, popular != 0);
                std::vector<uint32_t> level, order, first;
                const uint32_t nl = sship::ks_levels(L.off.data(), L.sb.data(), L.S, L.B, false, level);
                CHECK(level.size() == L.S, "level has %zu entries for %zu atoms", level.size(), L.S);
                uint32_t top = 0;
                for (size_t s = 0; s < L.S; ++s) {
                    // 1 + the largest level of an earlier atom that shares a signal: both "different levels, in cols order" and "the smallest"
                    uint32_t want = 1;
                    for (size_t t = 0; t < s; ++t)
                        if (share(L, s, t)) {
                            ++pairs;
                            CHECK(level[t] < level[s], "atoms %zu and %zu share a signal: levels %u, %u", t, s, level[t], level[s]);
                            want = std::max(want, level[t] + 1u);
                        }
                    CHECK(level[s] == want, "atom %zu: level %u, the smallest allowed is %u", s, level[s], want);
                    if (L.off[s] == L.off[s + 1]) { ++userless; CHECK(level[s] == 1u, "atom %zu has no user: level %u", s, level[s]); }
                    top = std::max(top, level[s]);
                }
                CHECK(nl == top, "%u levels returned, the largest is %u", nl, top);
                // the order: every atom once, by (level, s), the levels' ranges
                sship::ks_order(level, nl, order, first);
                CHECK(order.size() == L.S && first.size() == (size_t)nl + 1u, "order / first sizes");
                std::set<uint32_t> seen(order.begin(), order.end());
                CHECK(seen.size() == L.S, "order is not a permutation");
                for (size_t i = 0; i + 1 < order.size(); ++i) {
                    const uint32_t a = order[i], b = order[i + 1];
                    CHECK(level[a] < level[b] || (level[a] == level[b] && a < b), "order[%zu], order[%zu] are not by (level, s)", i, i + 1);
                }
                for (uint32_t l = 0; l < nl; ++l) {
                    CHECK(first[l] < first[l + 1], "level %u is empty", l + 1);
                    for (uint32_t i = first[l]; i < first[l + 1] && i < order.size(); ++i) CHECK(level[order[i]] == l + 1u, "order[%u] is not of level %u", i, l + 1);
                }
                if (nl) CHECK(first[0] == 0u && first[nl] == L.S, "first does not span the atoms");
                // the serial flag: s + 1
                const uint32_t ns = sship::ks_levels(L.off.data(), L.sb.data(), L.S, L.B, true, level);
                CHECK(ns == L.S, "serial: %u levels for %zu atoms", ns, L.S);
                for (size_t s = 0; s < L.S; ++s) CHECK(level[s] == s + 1u, "serial: atom %zu has level %u", s, level[s]);
                CHECK(sship::ks_first_duplicate(L.off.data(), L.sb.data(), L.S) == L.S, "a duplicate where there is none");
                ++cases;
                atoms += L.S;
            }
    // a list that names a signal twice is found, at the right atom
    {
        const uint32_t off[] = { 0u, 2u, 5u, 5u, 7u }, sb[] = { 1u, 4u, 0u, 3u, 3u, 2u, 6u };
        CHECK(sship::ks_first_duplicate(off, sb, 4) == 1u, "the duplicate of atom 1 was not found");
        const uint32_t sb2[] = { 1u, 4u, 4u, 3u, 5u, 2u, 6u };      // equal neighbours across two atoms' lists are not one
        CHECK(sship::ks_first_duplicate(off, sb2, 4) == 4u, "equal signals of two different atoms taken for a duplicate");
    }
    std::printf("cases checked %zu\natoms checked %zu\nsharing pairs checked %zu\natoms without users %zu\n", cases, atoms, pairs, userless);
    if (failures) { std::printf("%d checks FAILED\n", failures); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
