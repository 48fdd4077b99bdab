// reo_top_pairs / reo_rank_shift: the best n of all gene pairs, selected on the device (semantics, the key, the pass loop and the host
// checks: top_pairs.h; entry points: queries.hip).
//   k_rank_shift     one thread per gene.  It walks the blocks of 32 sample slots of side A and of side B and adds, per block,
//     sum_k 2^k (popcount(lo plane k) + popcount(hi plane k)) -- the block's sum of lo + hi over its live slots; padding slots are rows of
//     zeros in both edges (transform.hip) -- and stores D = sum_A S_B - sum_B S_A as int64.  128 bytes per gene and block.  With `sums`
//     it also stores sum_A and sum_B themselves ([2][Gp]; reo_top_pairs_loo forms D of a fold from them); D is the same either way.
//   k_top_pairs<MODE, NB>   (NB = plane_bits(G) planes: a constant trip count of the chain)  the hot path, in the geometry of k_pairs_masked: a wave owns 64 columns (lane = gene j) and kTpRows rows, four
//     waves per workgroup take four neighbouring column tiles of the same rows.  Only tiles that touch i < j are walked (tp_tile_live), and
//     inside a tile on the diagonal the lanes with j <= i are dead.  Side A's groups, then side B's; groups of neither side are skipped
//     whole.  A lane loads the 16 pos planes of its column once per block and keeps them for all rows; the band edges of a row are
//     wave-uniform (__restrict__ arguments: scalar loads).  The borrow chain of band_chain.h gives lt and le, whose popcounts add up to gt
//     and gt + eq per row and side.  At the end the lane forms N from the counts, Gamma from D[i] (uniform) and D[j], and the key.
//       MODE = HIST: the key's digit below the pass's prefix goes into a histogram of the workgroup in LDS (atomicAdd on 32-bit bins; keys
//         above / below the prefix into two extra counters); the histogram is flushed once, one 64-bit global atomicAdd per non-zero bin.
//       MODE = EMIT: a key at or above the cut is appended to the candidate buffer: a ballot, one global atomicAdd per wave and row, every
//         lane stores its own record.  A record is stored only below the capacity; the counter alone runs on, and the host reads it.
// Integer atomics only: the histogram and the set of candidates are deterministic; the order of the candidates is not, and the host sort
// removes it.  No kernel keeps state between launches; there is no grid-wide synchronisation and no spinning.  Addresses: rows end at the
// next multiple of kTpRows and columns at the next multiple of 64, both below Gp (a multiple of 1024); D and the mask words are sized for
// Gp genes; blocks are bounded by the group offsets of the transform; bins by the 12 bits of a digit.
#include "top_pairs.h"
#include "reo_internal.h"
#include "top_count.h"

namespace reo {

namespace {

constexpr int kTpThreads = 256;
static_assert(kTpThreads == kTpWaves * 64, "one wave per column tile of the workgroup");
constexpr int kTpHist = 0, kTpEmit = 1;
static_assert(kGenePad % kTpRows == 0 && kGenePad % 64 == 0, "row and column tiles end inside the padded gene count");

struct TpArgs {
    int G, Gp, ngroups;
    int s_a, s_b;       // the sides' sizes
    int shift;          // HIST: the digit's lowest bit; EMIT: key >> shift is compared with ref
    uint32_t capacity;  // EMIT: records of the candidate buffer
    TpKey ref;          // HIST: the prefix; EMIT: the cut
};

__global__ __launch_bounds__(256) void k_rank_shift(const uint4 *__restrict__ AL, const uint4 *__restrict__ AH, const int32_t *__restrict__ goff,
                                                    const int32_t *__restrict__ gside, int G, int Gp, int ngroups, int s_a, int s_b,
                                                    int64_t *__restrict__ D, int64_t *__restrict__ sums)
{
    const int gene = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    if (gene >= Gp) return;
    int64_t sum[2] = {0, 0};
    if (gene < G) {
        for (int g = 0; g < ngroups; ++g) {
            const int side = gside[g];
            if (side > 1) continue;
            int64_t acc = 0;
            const int b1 = goff[g + 1];
            for (int b = goff[g]; b < b1; ++b) {
                uint32_t lo[16], hi[16];
                band_load_edges<false, true>(AL, AH, band_edge_row<false>(Gp, b, gene), lo, hi);
#pragma unroll
                for (int k = 0; k < 16; ++k) acc += band_edge_term<int64_t>(lo, hi, k, BandPopcount{});
            }
            if (side == 0) sum[0] += acc; else sum[1] += acc;
        }
    }
    D[gene] = tp_shift(sum[0], sum[1], s_a, s_b);   // (genes >= G: 0)
    if (sums) { sums[gene] = sum[0]; sums[Gp + gene] = sum[1]; }   // (reo_top_pairs_loo: D of a fold needs the two sums apart)
}

template <int MODE, int NB>   // NB = plane_bits(G): 12, 15 or 16 planes
__global__ __launch_bounds__(kTpThreads) void k_top_pairs(const uint4 *__restrict__ P, const uint4 *__restrict__ AL, const uint4 *__restrict__ AH,
                                                          const int32_t *__restrict__ goff, const int32_t *__restrict__ gside,
                                                          const int64_t *__restrict__ D, const uint32_t *__restrict__ maskbits,
                                                          unsigned long long *__restrict__ hist, TpRec *__restrict__ cand,
                                                          uint32_t *__restrict__ cand_n, TpArgs a)
{
    __shared__ uint32_t bins[MODE == kTpHist ? kTpHistWords : 1];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
    const int ctile = static_cast<int>(blockIdx.x) * kTpWaves + wave;
    const int i0 = static_cast<int>(blockIdx.y) * kTpRows;
    if (!tp_group_live(static_cast<int>(blockIdx.x), i0)) return;   // (workgroup-uniform, in front of every barrier)
    if constexpr (MODE == kTpHist) {
        for (int b = static_cast<int>(threadIdx.x); b < kTpHistWords; b += kTpThreads) bins[b] = 0;
        __syncthreads();
    }
    if (tp_tile_live(ctile, i0, a.G)) {   // (wave-uniform)
        const int j = ctile * 64 + lane;   // < Gp
        uint32_t gt_a[kTpRows], le_a[kTpRows], gt_b[kTpRows], le_b[kTpRows];
#pragma unroll
        for (int r = 0; r < kTpRows; ++r) { gt_a[r] = 0; le_a[r] = 0; gt_b[r] = 0; le_b[r] = 0; }
        const TpRowsFrom row_of{i0};   // (i0 + r < Gp)
        tp_count_side<NB>(P, AL, AH, goff, gside, 0, j, row_of, a, gt_a, le_a);
        tp_count_side<NB>(P, AL, AH, goff, gside, 1, j, row_of, a, gt_b, le_b);
        const int64_t dj = D[j];
        const bool col_ok = tp_mask_bit(maskbits, j);
#pragma unroll
        for (int r = 0; r < kTpRows; ++r) {
            const int i = i0 + r;
            if (i >= a.G) break;   // (wave-uniform)
            const bool live = tp_lane_live(i, j, a.G) && col_ok && tp_mask_bit(maskbits, i);
            const int32_t eq_a = static_cast<int32_t>(le_a[r] - gt_a[r]), eq_b = static_cast<int32_t>(le_b[r] - gt_b[r]);
            const int64_t n = tp_num(static_cast<int32_t>(gt_a[r]), eq_a, static_cast<int32_t>(gt_b[r]), eq_b, a.s_a, a.s_b);
            const TpKey key = tp_pack(tp_abs(n), tp_gamma(D[i], dj), i, j, a.G);
            if constexpr (MODE == kTpHist) {
                if (live) {
                    const int c = tp_cmp(tp_top(key, a.shift), a.ref);
                    atomicAdd(&bins[c > 0 ? kTpAbove : (c < 0 ? kTpBelow : static_cast<int>(tp_digit(key, a.shift)))], 1u);
                }
            } else {
                const bool take = live && tp_cmp(tp_shr(key, a.shift), a.ref) >= 0;
                const unsigned long long m = __ballot(take);
                if (m != 0) {   // (wave-uniform)
                    const int leader = __builtin_ctzll(m);
                    uint32_t base = 0;
                    if (lane == leader) base = atomicAdd(cand_n, static_cast<uint32_t>(__builtin_popcountll(m)));
                    base = static_cast<uint32_t>(__shfl(static_cast<int>(base), leader));
                    const uint32_t at = base + static_cast<uint32_t>(__builtin_popcountll(m & ((1ull << lane) - 1ull)));
                    if (take && at < a.capacity) cand[at] = TpRec{i, j, static_cast<int32_t>(gt_a[r]), eq_a, static_cast<int32_t>(gt_b[r]), eq_b};
                }
            }
        }
    }
    if constexpr (MODE == kTpHist) {
        __syncthreads();
        for (int b = static_cast<int>(threadIdx.x); b < kTpHistWords; b += kTpThreads) {
            const uint32_t v = bins[b];
            if (v) atomicAdd(&hist[b], static_cast<unsigned long long>(v));
        }
    }
}

TpArgs tp_args(reo_ctx *c, int s_a, int s_b)
{
    TpArgs a;
    a.G = static_cast<int>(c->G); a.Gp = c->Gp; a.ngroups = c->ngroups;
    a.s_a = s_a; a.s_b = s_b; a.shift = 0; a.capacity = 0; a.ref = TpKey{0, 0};
    return a;
}

template <int MODE>
void tp_launch(reo_ctx *c, const int32_t *d_gside, const int64_t *d_D, const uint32_t *d_maskbits, unsigned long long *d_hist, TpRec *d_cand,
               uint32_t *d_cand_n, const TpArgs &a)
{
    with_plane_bits(c->G, [&](auto nb) {
        k_top_pairs<MODE, decltype(nb)::value><<<tile_grid(c->G, c->G, kTpRows, kTpWaves), kTpThreads, 0, c->stream>>>(
            c->pos.p, c->lo.p, c->hi.p, c->goff_dev.p, d_gside, d_D, d_maskbits, d_hist, d_cand, d_cand_n, a);
    });
}

}  // namespace

int32_t launch_rank_shift(reo_ctx *c, const int32_t *d_gside, int s_a, int s_b, int64_t *d_D, int64_t *d_sums)
{
    int32_t rc = need_planes(c, "reo_rank_shift", kTpMaxGenes);
    if (rc) return rc;
    k_rank_shift<<<static_cast<unsigned>(c->Gp / 256), 256, 0, c->stream>>>(c->lo.p, c->hi.p, c->goff_dev.p, d_gside, static_cast<int>(c->G), c->Gp,
                                                                            c->ngroups, s_a, s_b, d_D, d_sums);
    REO_HIP_CHECK(hipGetLastError());
    return REO_OK;
}

int32_t launch_top_hist(reo_ctx *c, const int32_t *d_gside, int s_a, int s_b, const int64_t *d_D, const uint32_t *d_maskbits, const TpKey &prefix,
                        int shift, unsigned long long *d_hist)
{
    int32_t rc = need_planes(c, "reo_top_pairs", kTpMaxGenes);
    if (rc) return rc;
    if (shift < 0 || shift > kTpKeyBits - kTpDigitBits || shift % kTpDigitBits) { set_error("reo_top_pairs: no digit at bit %d", shift); return REO_EINVAL; }
    TpArgs a = tp_args(c, s_a, s_b);
    a.shift = shift; a.ref = prefix;
    tp_launch<kTpHist>(c, d_gside, d_D, d_maskbits, d_hist, nullptr, nullptr, a);
    REO_HIP_CHECK(hipGetLastError());
    return REO_OK;
}

int32_t launch_top_emit(reo_ctx *c, const int32_t *d_gside, int s_a, int s_b, const int64_t *d_D, const uint32_t *d_maskbits, const TpKey &cut,
                        int shift, TpRec *d_cand, int64_t capacity, uint32_t *d_cand_n)
{
    int32_t rc = need_planes(c, "reo_top_pairs", kTpMaxGenes);
    if (rc) return rc;
    if (shift < 0 || shift > kTpKeyBits - kTpDigitBits || capacity < 1 || capacity > (int64_t(1) << 30) || !d_cand || !d_cand_n) {
        set_error("reo_top_pairs: a candidate buffer of %lld records at bit %d cannot be filled", (long long)capacity, shift);
        return REO_EINVAL;
    }
    TpArgs a = tp_args(c, s_a, s_b);
    a.shift = shift; a.ref = cut; a.capacity = static_cast<uint32_t>(capacity);
    tp_launch<kTpEmit>(c, d_gside, d_D, d_maskbits, nullptr, d_cand, d_cand_n, a);
    REO_HIP_CHECK(hipGetLastError());
    return REO_OK;
}

}  // namespace reo
