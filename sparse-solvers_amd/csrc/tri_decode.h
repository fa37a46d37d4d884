// The tile pair of a workgroup of the symmetric product G = At · At^T (gemm.hip, k_gemm_tn_f32<SYM>): the tiles on and above the
// diagonal are enumerated column panel by column panel, b = bn (bn + 1) / 2 + bm with bm <= bn.  The square root is a first guess
// only — two integer loops correct it — so the pair is exact for every b the launcher admits (b < 2^31); tests/cpp/test_tri_decode.cpp
// checks that on the host.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define SS_TRI_HD __host__ __device__
#else
#define SS_TRI_HD
#endif

namespace sship {

SS_TRI_HD inline void tri_tile_decode(uint32_t b, uint32_t& bm, uint32_t& bn)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const float root = __fsqrt_rn(8.f * (float)b + 1.f);
#else
    const float root = std::sqrt(8.f * (float)b + 1.f);
#endif
    uint32_t t = (uint32_t)((root - 1.f) * 0.5f);
    while ((uint64_t)t * (t + 1u) / 2u > b) --t;
    while ((uint64_t)(t + 1u) * (t + 2u) / 2u <= b) ++t;
    bn = t;
    bm = b - (uint32_t)((uint64_t)t * (t + 1u) / 2u);
}

}  // namespace sship
