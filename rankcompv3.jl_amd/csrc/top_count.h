// The count loop that k_top_pairs (toppairs.hip) and k_top_partners_count (toppartners.hip) share: a wave's kTpRows rows against the 64
// columns of its lanes over the blocks of one side's groups.  The chain itself: band_chain.h.
#pragma once

#include "band_chain.h"
#include "top_pairs.h"

namespace reo {

// The rows of a wave as tp_count_side takes them: consecutive from i0 (k_top_pairs).  A named type and not a lambda: with a lambda
// k_top_pairs<EMIT, 12> alone came out with another instruction schedule.
struct TpRowsFrom {
    int i0;
    __device__ __forceinline__ int operator()(int r) const { return i0 + r; }
};

// The counts of one side: gt[r] += popcount(lt), le[r] += popcount(le) of the rows row_of(r) against column j.  row_of(r) is wave-uniform
// and below Gp -- i0 + r in k_top_pairs, the r-th query gene in k_top_partners_count -- so the band edges of a row are scalar loads.
template <int NB, typename Rows, typename Args>
__device__ __forceinline__ void tp_count_side(const uint4 *__restrict__ P, const uint4 *__restrict__ AL, const uint4 *__restrict__ AH,
                                              const int32_t *__restrict__ goff, const int32_t *__restrict__ gside, int side, int j, Rows row_of,
                                              const Args &a, uint32_t (&gt)[kTpRows], uint32_t (&le)[kTpRows])
{
    for (int g = 0; g < a.ngroups; ++g) {
        if (gside[g] != side) continue;   // (wave-uniform)
        const int b1 = goff[g + 1];
        for (int b = goff[g]; b < b1; ++b) {
            uint32_t p[16];
            band_load_pos<false>(P, a.Gp, b, j, p);
#pragma unroll
            for (int r = 0; r < kTpRows; ++r) {
                uint32_t lo[16], hi[16], lt, lq;
                band_load_edges<false, true>(AL, AH, band_edge_row<false>(a.Gp, b, row_of(r)), lo, hi);
                band_chain<false, true, NB>(p, lo, hi, lt, lq);
                gt[r] += static_cast<uint32_t>(__builtin_popcount(lt));
                le[r] += static_cast<uint32_t>(__builtin_popcount(lq));
            }
        }
    }
}

}  // namespace reo
