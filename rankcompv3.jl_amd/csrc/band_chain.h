// The borrow chain of the plane-reading kernels, stated once: how the pos planes and the band edges of one gene and block of 32 sample slots
// lie (transform.hip), the loads of one column's planes and one row's edges, and the chain lt <- majority(~p_k, edge_k, lt) over the planes.
// Users: k_sample_counts (samplecounts.hip), k_pair_support (pairsupport.hip), k_pairs_masked / k_counts_masked (maskedpairs.hip),
// k_pairs_permuted (permpairs.hip), k_top_pairs (toppairs.hip) and k_top_partners_count (toppartners.hip) through top_count.h,
// k_rank_shift (toppairs.hip), k_top_pairs_null (toppairsnull.hip), k_loo_words / k_loo_select (toppairsloo.hip) and k1_counts<BIG>
// (kernels.hip).  A kernel takes the loaders where they leave its code as it was (the register comparison names the ones that unpack
// their own loads), and every kernel takes the chain or its plane step from here.  The staged count loop of the pair kernel (kernels.hip,
// k1_loop_gen.inc) is a different walk over the same planes and is not built on this.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace reo {

template <bool BIG>   // BIG: more than 65 535 genes, 17 or 18 planes
struct BandLayout {
    static constexpr int NQ = BIG ? 5 : 4;   // uint4 of pos planes per gene and block
    static constexpr int EQ = BIG ? 8 : 4;   // uint4 per edge row
    static constexpr int NW = 4 * NQ;        // plane words that a kernel holds per gene and block
    // the word of an edge row that holds plane k: the 16-plane layout keeps plane k in word (k + 15) % 16
    static __device__ __forceinline__ constexpr int edge_word(int k) { return BIG ? k : ((k + 15) & 15); }
};

// Quarter q of a gene's planes (one uint4: planes 4q .. 4q + 3) into its words.
template <int N>
__device__ __forceinline__ void band_unpack(const uint4 v, uint32_t (&w)[N], int q)
{
    w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
}

// The pos planes of column j in block b.
template <bool BIG>
__device__ __forceinline__ void band_load_pos(const uint4 *__restrict__ P, int Gp, int b, int j, uint32_t (&p)[BandLayout<BIG>::NW])
{
    const uint4 *pb = P + static_cast<size_t>(b) * BandLayout<BIG>::NQ * Gp + j;
#pragma unroll
    for (int q = 0; q < BandLayout<BIG>::NQ; ++q) band_unpack(pb[static_cast<size_t>(q) * Gp], p, q);
}

// The band edges of one gene and block: lo and, with LE, hi (without it hi is left alone and AH is not read).  `row` counts uint4 from AL /
// AH (band_edge_row); a caller that holds the row's pointers passes them with row = 0.  With __restrict__ kernel arguments and a
// wave-uniform gene these are scalar loads.
template <bool BIG>
__device__ __forceinline__ size_t band_edge_row(int Gp, int b, int i) { return (static_cast<size_t>(b) * Gp + i) * BandLayout<BIG>::EQ; }

template <bool BIG, bool LE>
__device__ __forceinline__ void band_load_edges(const uint4 *__restrict__ AL, const uint4 *__restrict__ AH, size_t row,
                                                uint32_t (&lo)[BandLayout<BIG>::NW], uint32_t (&hi)[BandLayout<BIG>::NW])
{
#pragma unroll
    for (int q = 0; q < BandLayout<BIG>::NQ; ++q) {
        band_unpack(AL[row + q], lo, q);
        if constexpr (LE) band_unpack(AH[row + q], hi, q);
    }
}

// One plane of a chain: acc <- majority(~p, edge, acc), with p the column's pos word of plane k and edge the row's edge word of that plane
// (edge_word(k)).  The one place that states the operation.
__device__ __forceinline__ uint32_t band_borrow(uint32_t p, uint32_t edge, uint32_t acc) { return __builtin_amdgcn_bitop3_b32(p, edge, acc, 0x8e); }

// The chain over the planes: lt = the slots where the column's position is below the row's lower edge, le (with LE) = below the upper
// edge, one bit per slot.  Two forms of the loop, one body:
//   NB = 12 / 15 / 16   a constant trip count: the kernels that are instantiated per plane_bits(G) (with_plane_bits, reo_internal.h).
//   NB = kBandGuard     nbits at run time, a guard per plane and not a break: the trip count stays constant and every p[k] a fixed register.
// A third form is not in here.  The compiler unrolls the loop of a helper before it inlines the helper, and the loop of a kernel in the
// kernel; for k_sample_counts and k1_counts (runtime nbits, break), k_pair_support (runtime nbits, guard) and k_top_pairs_null (constant
// NB) the two do not give the same code -- k_pair_support<false, true, false> goes from 100 to 102 SGPRs and loses a wave of occupancy.
// These four keep the three-line loop over band_borrow in the kernel; profiles/band_chain_refactor_registers.txt has the comparison.
constexpr int kBandGuard = 0;

template <bool BIG, bool LE, int NB>
__device__ __forceinline__ void band_chain(const uint32_t (&p)[BandLayout<BIG>::NW], const uint32_t (&lo)[BandLayout<BIG>::NW],
                                           const uint32_t (&hi)[BandLayout<BIG>::NW], uint32_t &lt, uint32_t &le, int nbits)
{
    static_assert(NB >= 0 && NB <= BandLayout<BIG>::NW, "the chain reads the planes that the layout holds");
    lt = 0; le = 0;
#pragma unroll
    for (int k = 0; k < (NB > 0 ? NB : BandLayout<BIG>::NW); ++k) {
        if constexpr (NB == kBandGuard) { if (k >= nbits) continue; }
        const int ew = BandLayout<BIG>::edge_word(k);
        lt = band_borrow(p[k], lo[ew], lt);
        if constexpr (LE) le = band_borrow(p[k], hi[ew], le);
    }
}

// The constant form without the argument it does not read; the guarded form has no such default: it must be given nbits.
template <bool BIG, bool LE, int NB>
__device__ __forceinline__ void band_chain(const uint32_t (&p)[BandLayout<BIG>::NW], const uint32_t (&lo)[BandLayout<BIG>::NW],
                                           const uint32_t (&hi)[BandLayout<BIG>::NW], uint32_t &lt, uint32_t &le)
{
    static_assert(NB > 0, "the guarded chain takes the number of planes at run time");
    band_chain<BIG, LE, NB>(p, lo, hi, lt, le, NB);
}

// lt / le of one pair and block for the kernels that use a row's edges once: the edge rows al / ah of the row gene against the column's
// pos planes p.
template <bool BIG, bool LE, int NB>
__device__ __forceinline__ void band_compare(const uint32_t (&p)[BandLayout<BIG>::NW], const uint4 *__restrict__ al, const uint4 *__restrict__ ah,
                                             uint32_t &lt, uint32_t &le, int nbits)
{
    uint32_t lo[BandLayout<BIG>::NW], hi[BandLayout<BIG>::NW];
    band_load_edges<BIG, LE>(al, ah, 0, lo, hi);
    band_chain<BIG, LE, NB>(p, lo, hi, lt, le, nbits);
}

// Plane k of a gene's edge sum: 2^k (f(lo plane k) + f(hi plane k)), 16-plane layout; the sum over k = 0 .. 15 is lo + hi (the planes above
// plane_bits(G) are zero: lo and hi are at most G).  f = popcount: of the block's slots together; f = bit t: of slot t.
struct BandPopcount { __device__ __forceinline__ int operator()(uint32_t w) const { return __builtin_popcount(w); } };
struct BandBit {
    int t;
    __device__ __forceinline__ uint32_t operator()(uint32_t w) const { return (w >> t) & 1u; }
};

template <typename T, typename F>
__device__ __forceinline__ T band_edge_term(const uint32_t (&lo)[16], const uint32_t (&hi)[16], int k, F f)
{
    const int ew = BandLayout<false>::edge_word(k);
    return static_cast<T>(f(lo[ew]) + f(hi[ew])) << k;
}

}  // namespace reo
