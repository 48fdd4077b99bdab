// reo_pair_support: how strongly a listed pair supports a call.  For every entry of a CSR of pairs (gene i of the row, partner j of the
// entry) the per-group counts of "x_i > x_j and not tied" and of "tied", and optionally the outcome byte of every sample.  The same
// O(pairs x samples) comparison as the pair kernel's, for a sparse list of pairs instead of dense rectangles.
//   k_pair_support<BIG, WITH_EQ, WITH_OUTCOME>   one wave per work item (pair_support.h: at most 64 consecutive entries of one row), four
//     waves per workgroup, one lane per entry.  The wave walks the groups and, within a group, its blocks of 32 sample slots: the band edges
//     lo_i / hi_i of the block are wave-uniform (the item's gene), a lane loads the pos planes of its own partner and runs the borrow chain
//     of band_chain.h over plane_bits(G) planes; popcount(lt) / popcount(le) go into two registers, stored at the group's end
//     (n_eq = le - lt).  Padding slots read as zero in the planes (transform.hip): the counts need no mask word.
//     WITH_OUTCOME: the lane expands lt / le of the block into bytes at outcome[e * S + slot2col[slot]] for the slots with a column in
//     [0, S); padding slots are never written.  These byte stores are NOT coalesced across lanes (a lane walks its own row of S bytes):
//     accepted and not tuned -- outcome lists are signatures of hundreds of pairs, not whole pair lists.
//     The le chain is compiled in when the tied counts or the outcomes need it.
// Integer arithmetic only and a fixed assignment of entries to lanes: deterministic.  Addresses: genes and partners are checked on the host
// (pair_support_check_args) before they are uploaded, so every row of the planes that is read lies in [0, G); items, entries and blocks
// are bounded by the counts the host passes; lanes past the item's count load the planes of the item's own gene and store nothing.
#include "pair_support.h"
#include "reo_internal.h"
#include "band_chain.h"

namespace reo {

namespace {

constexpr int kPsThreads = 256;
constexpr int kPsWaves = kPsThreads / kPsLanes;

struct PsArgs {
    int n_items, ngroups, Gp, nbits;
    int64_t S;
};

// The read-only arrays are kernel arguments of their own, __restrict__: nothing the kernel stores can alias them, so the compiler may fetch
// what is wave-uniform (the item, the group offsets, the edge rows, the slot map) with scalar loads and keep it in SGPRs.
template <bool BIG, bool WITH_EQ, bool WITH_OUTCOME>
__global__ __launch_bounds__(kPsThreads) void k_pair_support(const PsItem *__restrict__ items, const int32_t *__restrict__ partner,
                                                             const int32_t *__restrict__ goff, const int32_t *__restrict__ slot2col,
                                                             const uint4 *__restrict__ P, const uint4 *__restrict__ AL,
                                                             const uint4 *__restrict__ AH, int32_t *__restrict__ out_gt,
                                                             int32_t *__restrict__ out_eq, uint8_t *__restrict__ outcome, PsArgs a)
{
    constexpr int NW = BandLayout<BIG>::NW;   // plane words per gene and block
    constexpr bool LE = WITH_EQ || WITH_OUTCOME;
    const int lane = threadIdx.x & (kPsLanes - 1);
    const int item = static_cast<int>(blockIdx.x) * kPsWaves + __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
    if (item >= a.n_items) return;   // (wave-uniform; the kernel has no barrier)
    const PsItem it = items[item];
    const int gene = __builtin_amdgcn_readfirstlane(it.gene), first = __builtin_amdgcn_readfirstlane(it.first);
    const int count = __builtin_amdgcn_readfirstlane(it.count);
    const bool active = lane < count;
    const size_t e = static_cast<size_t>(first) + (active ? lane : 0);
    const int j = active ? partner[e] : gene;
    for (int g = 0; g < a.ngroups; ++g) {
        uint32_t n_lt = 0, n_le = 0;
        const int b1 = goff[g + 1];
        for (int b = goff[g]; b < b1; ++b) {
            uint32_t lo[NW], hi[NW], p[NW];   // (hi: unused and gone without the le chain)
            const size_t row = band_edge_row<BIG>(a.Gp, b, gene);
            const uint4 *al = AL + row, *ah = AH + row;
            const uint4 *pb = P + static_cast<size_t>(b) * BandLayout<BIG>::NQ * a.Gp + j;
#pragma unroll
            for (int q = 0; q < BandLayout<BIG>::NQ; ++q) {   // (one loop for the three: the loads of a quarter are issued together)
                band_unpack(al[q], lo, q);
                if constexpr (LE) band_unpack(ah[q], hi, q);
                band_unpack(pb[static_cast<size_t>(q) * a.Gp], p, q);
            }
            uint32_t lt = 0, le = 0;
#pragma unroll
            for (int k = 0; k < NW; ++k) {
                if (k >= a.nbits) continue;   // (a guard per plane, not a break: the trip count stays constant and every p[k] a fixed register)
                const int ew = BandLayout<BIG>::edge_word(k);
                lt = band_borrow(p[k], lo[ew], lt);
                if constexpr (LE) le = band_borrow(p[k], hi[ew], le);
            }
            n_lt += static_cast<uint32_t>(__builtin_popcount(lt));
            if constexpr (WITH_EQ) n_le += static_cast<uint32_t>(__builtin_popcount(le));
            if constexpr (WITH_OUTCOME) {
                uint8_t *row = outcome + e * static_cast<size_t>(a.S);
#pragma clang loop unroll(disable)
                for (int s = 0; s < 32; ++s) {
                    const int col = slot2col[b * 32 + s];   // (wave-uniform)
                    if (active && col >= 0 && col < a.S) row[col] = ps_outcome_byte(lt, le, s);
                }
            }
        }
        if (active) {
            const size_t o = e * static_cast<size_t>(a.ngroups) + g;
            out_gt[o] = static_cast<int32_t>(n_lt);
            if constexpr (WITH_EQ) out_eq[o] = static_cast<int32_t>(n_le - n_lt);
        }
    }
}

struct PsPtrs {
    const PsItem *items;
    const int32_t *partner, *goff, *slot2col;
    const uint4 *P, *AL, *AH;
    int32_t *gt, *eq;
    uint8_t *outcome;
};

template <bool BIG, bool WITH_EQ>
void launch_ps(const PsPtrs &p, const PsArgs &a, dim3 g, hipStream_t st)
{
    if (p.outcome)
        k_pair_support<BIG, WITH_EQ, true><<<g, kPsThreads, 0, st>>>(p.items, p.partner, p.goff, p.slot2col, p.P, p.AL, p.AH, p.gt, p.eq, p.outcome, a);
    else
        k_pair_support<BIG, WITH_EQ, false><<<g, kPsThreads, 0, st>>>(p.items, p.partner, p.goff, p.slot2col, p.P, p.AL, p.AH, p.gt, p.eq, p.outcome, a);
}

}  // namespace

int32_t launch_pair_support(reo_ctx *c, const PsItem *d_items, int64_t n_items, const int32_t *d_partner, const int32_t *d_slot2col,
                            int32_t *d_gt, int32_t *d_eq, uint8_t *d_outcome)
{
    if (!c->pos.p || !c->lo.p || !c->hi.p || !c->goff_dev.p || c->goff32.empty() || c->ngroups < 1) {
        set_error("reo_pair_support: no bit planes");
        return REO_EINVAL;
    }
    if (const int32_t rp = ensure_planes(c)) return rp;
    if (n_items < 1 || n_items > (int64_t(1) << 24) || (d_outcome && !d_slot2col)) {
        set_error("reo_pair_support: a batch of %lld work items cannot be launched", (long long)n_items);
        return REO_EINVAL;
    }
    PsPtrs p;
    p.items = d_items; p.partner = d_partner; p.goff = c->goff_dev.p; p.slot2col = d_slot2col;
    p.P = c->pos.p; p.AL = c->lo.p; p.AH = c->hi.p;
    p.gt = d_gt; p.eq = d_eq; p.outcome = d_outcome;
    PsArgs a;
    a.n_items = static_cast<int>(n_items); a.ngroups = c->ngroups; a.Gp = c->Gp; a.nbits = plane_bits(c->G);
    a.S = c->S;
    const dim3 g(static_cast<unsigned>((n_items + kPsWaves - 1) / kPsWaves));
    if (c->G > 65535) {
        if (d_eq) launch_ps<true, true>(p, a, g, c->stream);
        else launch_ps<true, false>(p, a, g, c->stream);
    } else {
        if (d_eq) launch_ps<false, true>(p, a, g, c->stream);
        else launch_ps<false, false>(p, a, g, c->stream);
    }
    REO_HIP_CHECK(hipGetLastError());
    return REO_OK;
}

}  // namespace reo
