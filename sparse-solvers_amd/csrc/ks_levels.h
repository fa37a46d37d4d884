// The level schedule of the K-SVD sweep (ksvd.hip), on the host: plain C++, no HIP types (tests/cpp/test_ks_levels.cpp).
//
// The sweep is DEFINED as sequential over the requested atoms s = 0 .. S - 1.  An atom's step reads and writes only the residual rows
// and the record values of its own users, so two atoms that share no signal commute exactly: the words of both are the same in
// either order, or side by side.  The schedule puts every atom in the earliest level in which all earlier atoms it shares a signal
// with are done:
//     level[s] = 1 + max over b in U_s of last[b],     then last[b] = level[s] for those b       (last[b] starts at 0)
// so an atom without users takes level 1.  The atoms are processed by (level, s); the atoms of one level share no signal.
// With `serial` level[s] = s + 1: the plain sequential order (a test aid).
//
// off[0 .. S]: the offsets of the atoms' user lists, sb[off[s] .. off[s + 1]): the users (signals < B) of atom s.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace sship {

// level[0 .. S) as above -> the number of levels (0 when S == 0)
inline uint32_t ks_levels(const uint32_t* off, const uint32_t* sb, size_t S, size_t B, bool serial, std::vector<uint32_t>& level)
{
    level.assign(S, 0u);
    if (serial) {
        for (size_t s = 0; s < S; ++s) level[s] = (uint32_t)s + 1u;
        return (uint32_t)S;
    }
    std::vector<uint32_t> last(B, 0u);
    uint32_t top = 0;
    for (size_t s = 0; s < S; ++s) {
        uint32_t lv = 0;
        for (uint32_t p = off[s]; p < off[s + 1]; ++p) lv = std::max(lv, last[sb[p]]);
        lv += 1u;
        for (uint32_t p = off[s]; p < off[s + 1]; ++p) last[sb[p]] = lv;
        level[s] = lv;
        top = std::max(top, lv);
    }
    return top;
}

// order[0 .. S): the atoms by (level, s); first[l] .. first[l + 1]: the atoms of level l + 1 in it (first has nlevels + 1 entries)
inline void ks_order(const std::vector<uint32_t>& level, uint32_t nlevels, std::vector<uint32_t>& order, std::vector<uint32_t>& first)
{
    const size_t S = level.size();
    first.assign((size_t)nlevels + 1u, 0u);
    for (size_t s = 0; s < S; ++s) first[level[s]] += 1u;               // (the count of level l, 1-based, at first[l])
    uint32_t run = 0;
    for (uint32_t l = 0; l <= nlevels; ++l) { const uint32_t c = first[l]; first[l] = run; run += c; }    // first[l] = atoms in levels < l
    std::vector<uint32_t> next(first.begin(), first.end());
    order.assign(S, 0u);
    for (size_t s = 0; s < S; ++s) order[next[level[s]]++] = (uint32_t)s;
    for (uint32_t l = 0; l < nlevels; ++l) first[l] = first[l + 1u];   // 0-based: level l + 1 starts at first[l]
    first[nlevels] = (uint32_t)S;
}

// the first atom whose sorted user list names a signal twice (equal neighbours), S when there is none
inline size_t ks_first_duplicate(const uint32_t* off, const uint32_t* sb, size_t S)
{
    for (size_t s = 0; s < S; ++s)
        for (uint32_t p = off[s]; p + 1u < off[s + 1]; ++p)
            if (sb[p] == sb[p + 1u]) return s;
    return S;
}

}  // namespace sship
