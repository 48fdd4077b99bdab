// What the borrow chain of the query kernels (samplecounts.hip, pairsupport.hip) reads: how the pos planes and the band edges of one gene and
// block of 32 sample slots lie (transform.hip).  k1_counts / k1_counts_big of kernels.hip run the same chain and keep their own copy.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace reo {

template <bool BIG>   // BIG: more than 65 535 genes, 17 or 18 planes
struct BandLayout {
    static constexpr int NQ = BIG ? 5 : 4;   // uint4 of pos planes per gene and block
    static constexpr int EQ = BIG ? 8 : 4;   // uint4 per edge row
    // the word of an edge row that holds plane k: the 16-plane layout keeps plane k in word (k + 15) % 16
    static __device__ __forceinline__ constexpr int edge_word(int k) { return BIG ? k : ((k + 15) & 15); }
};

// Quarter q of a gene's planes (one uint4: planes 4q .. 4q + 3) into its words.
template <int N>
__device__ __forceinline__ void band_unpack(const uint4 v, uint32_t (&w)[N], int q)
{
    w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
}

}  // namespace reo
