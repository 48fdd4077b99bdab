// The keyed coin stream of the tied samples, shared by the pair kernels (kernels.hip) and the masked pair kernel (maskedpairs.hip): a draw
// depends on (seed, i, j, group) and on the number of tied samples only, so every unit that classifies a pair draws the same coins.
// Host restatement: oracle/reo_numpy.py, tie_wins.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace reo {

__device__ __forceinline__ uint64_t mix64(uint64_t z)
{
    z += 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

// Binomial(n_eq, 1/2) draw standing in for n_eq calls of rand(Bool) in
// is_greater (:72-73): one bit of a counter-based stream keyed by
// (seed, i, j, group) per tied sample.
__device__ inline uint32_t tie_wins(uint64_t seed, uint32_t i, uint32_t j, uint32_t g, uint32_t n_eq)
{
    uint64_t base = mix64(seed ^ mix64((static_cast<uint64_t>(i) << 32) | j)) + (static_cast<uint64_t>(g) << 40);
    uint32_t wins = 0;
    for (uint64_t w = 0; n_eq > 0; ++w) {
        uint64_t bits = mix64(base + w);
        uint32_t take = n_eq < 64 ? n_eq : 64;
        if (take < 64) bits &= (1ULL << take) - 1;
        wins += __popcll(bits);
        n_eq -= take;
    }
    return wins;
}

}  // namespace reo
