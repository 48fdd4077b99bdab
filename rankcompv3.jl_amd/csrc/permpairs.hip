// Label-permutation null: the class tables of a batch of permutations from ONE walk over the bit planes (reo_perm_null, reo_perm_codes;
// semantics, shared arithmetic and host checks: perm_null.h; entry points: api.hip).
//   k_perm_words       the label bytes [n_perm][S] (caller's column order) into one A-word per (permutation, block of 32 sample slots), through
//     the slot -> column map as k_valid_words does, laid out [launch group][block][kPermQ] (pn_word_index), and one live word per block
//     (bit = the slot has a column).  Padding slots are 0 in both, so A is a subset of live.
//   k_pairs_permuted   the hot path, on the tiling of k_pairs_masked.  A wave owns 64 table columns (lane = gene j) and kPermRows table rows;
//     four waves per workgroup take four neighbouring column tiles of the same rows; blockIdx.z is the launch group of kPermQ permutations.
//     The wave walks ALL sample blocks of all groups: a lane loads the 16 pos planes of its column once per block and keeps them for all
//     rows of the tile; the band edges of a row, the live word and the kPermQ A-words of the block are wave-uniform (__restrict__
//     arguments, wave-uniform addresses: scalar loads).  Per (row, block) there is one borrow chain (band_chain.h; the tie-free form reads no
//     upper edges and runs the lt chain alone), then
//     gt_all += popc(lt & live), eq_all += popc(le & ~lt & live), and per permutation q  gtA[q] += popc(lt & A[q]), eqA[q] likewise: two
//     VALU instructions per counter instead of the whole chain per permutation.  Side B is all - A.  The tie-free form (the transform
//     reported no ties) carries no eq counters.  At the end every permutation is classified as k_pairs_masked classifies: EVERY ordered
//     pair from its own row -- below the diagonal (i > j) the lane forms the counts of (j, i) from its own, gt(j, i) = n - gt - eq, the coin
//     keyed by the smaller index first and by the SIDE (0 = A, 1 = B), and stores 8 minus its class -- so there is no mirror store and no
//     atomic.  Ballots make the four plane words of the 64 columns; lanes 0 .. 7 store the eight 32-bit words into row i of table q of
//     the batch buffer [P][G][4][Wp].  The diagonal and the columns >= G stay 0; the table words of the columns past the last tile are
//     cleared once by the caller's memset and never written.
//   k_perm_accumulate  per permutation, behind its pass: n_ge[i] += |delta1_p(i)| >= |delta1_obs(i)| (pn_exceeds), the permutation's n_up /
//     n_down among the genes with pval <= pval_deg && padj <= padj_deg by the sign of z1, and its se.
// Integer arithmetic only (the counts of n_up / n_down are integer atomics) and a fixed assignment of pairs to lanes: deterministic.
// Addresses: rows and columns of the planes are below Gp (the row tiles end at the next multiple of kPermRows, the column tiles at the next
// multiple of 64, Gp is a multiple of 1024); blocks run over [0, nblk), the number of blocks the transform sliced and the A / live words
// were sized for; a launch group z < ceil(np / kPermQ) reads the words of its own group, which pn_word_count allocates whole
// (rows past np are zero, and nothing of them is stored); table q of the batch is written only for z kPermQ + q < np <= P, rows
// i < G, words ctile 2 + {0, 1} < Wp; the thresholds are two scalars.  Counts are at most S <= 65535.
#include "perm_null.h"
#include "reo_internal.h"
#include "band_chain.h"
#include "tie_coin.h"

namespace reo {

namespace {

constexpr int kPnThreads = 256;
constexpr int kPnWaves = kPnThreads / 64;
static_assert(kGenePad % kPermRows == 0 && kGenePad % 64 == 0, "row and column tiles end inside the padded gene count");

__global__ __launch_bounds__(256) void k_perm_words(const uint8_t *__restrict__ side, const int32_t *__restrict__ slot2col, int64_t S, int64_t n_perm,
                                                    int nblk, uint32_t *__restrict__ aw, uint32_t *__restrict__ live)
{
    const int64_t p = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    const int b = static_cast<int>(blockIdx.y);
    if (p >= n_perm || b >= nblk) return;
    const int32_t *map = slot2col + static_cast<size_t>(b) * 32;
    aw[pn_word_index(p, b, nblk)] = pn_side_word(side + p * S, S, map);
    if (p == 0) live[b] = pn_live_word(S, map);
}

struct PnArgs {
    int G, Gp, Wp, nbits, nblk;
    int n1, n2, m1, m2;   // the sides' sizes and thresholds: kept under every permutation
    int np;               // permutations of this launch (tables 0 .. np - 1 of the batch buffer)
    uint64_t seed;
    size_t table_words;   // G * 4 * Wp
};

template <bool TIES>
__global__ __launch_bounds__(kPnThreads) void k_pairs_permuted(const uint4 *__restrict__ P, const uint4 *__restrict__ AL, const uint4 *__restrict__ AH,
                                                               const uint32_t *__restrict__ AW, const uint32_t *__restrict__ LW,
                                                               uint32_t *__restrict__ tables, PnArgs a)
{
    const int lane = threadIdx.x & 63;
    const int ctile = static_cast<int>(blockIdx.x) * kPnWaves + __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
    const int i0 = static_cast<int>(blockIdx.y) * kPermRows;
    const int z = static_cast<int>(blockIdx.z);
    if (ctile * 64 >= a.G || i0 >= a.G || z * kPermQ >= a.np) return;   // (wave-uniform; the kernel has no barrier)
    const int j = ctile * 64 + lane;                                    // < Gp
    const uint32_t *__restrict__ aw = AW + static_cast<size_t>(z) * a.nblk * kPermQ;
    constexpr int kEq = TIES ? kPermQ : 1;
    uint32_t gtA[kPermRows][kPermQ], eqA[kPermRows][kEq], gtAll[kPermRows], eqAll[kPermRows];
#pragma unroll
    for (int r = 0; r < kPermRows; ++r) {
        gtAll[r] = 0; eqAll[r] = 0;
#pragma unroll
        for (int q = 0; q < kPermQ; ++q) gtA[r][q] = 0;
#pragma unroll
        for (int q = 0; q < kEq; ++q) eqA[r][q] = 0;
    }
    for (int b = 0; b < a.nblk; ++b) {
        uint32_t p[16];
        const uint4 *pb = P + static_cast<size_t>(b) * 4 * a.Gp + j;
#pragma unroll
        for (int q = 0; q < 4; ++q) band_unpack(pb[static_cast<size_t>(q) * a.Gp], p, q);
        const uint32_t live = LW[b];
        uint32_t A[kPermQ];
#pragma unroll
        for (int q = 0; q < kPermQ; ++q) A[q] = aw[static_cast<size_t>(b) * kPermQ + q];
#pragma unroll
        for (int r = 0; r < kPermRows; ++r) {
            // (i0 + r < Gp; row * EQ and not band_edge_row, which multiplies before it adds the pointer and reorders this kernel)
            const size_t row = static_cast<size_t>(b) * a.Gp + (i0 + r);
            uint32_t lt, le;
            band_compare<false, TIES, kBandGuard>(p, AL + row * BandLayout<false>::EQ, AH + row * BandLayout<false>::EQ, lt, le, a.nbits);
            lt &= live;
            gtAll[r] += static_cast<uint32_t>(__builtin_popcount(lt));
#pragma unroll
            for (int q = 0; q < kPermQ; ++q) gtA[r][q] += static_cast<uint32_t>(__builtin_popcount(lt & A[q]));
            if (TIES) {
                const uint32_t e = le & ~lt & live;
                eqAll[r] += static_cast<uint32_t>(__builtin_popcount(e));
#pragma unroll
                for (int q = 0; q < kEq; ++q) eqA[r][q] += static_cast<uint32_t>(__builtin_popcount(e & A[q]));
            }
        }
    }
#pragma unroll
    for (int r = 0; r < kPermRows; ++r) {
        const int i = i0 + r;
        if (i >= a.G) break;   // (wave-uniform)
        // the pair with the smaller index first: above the diagonal the lane's own counts, below it those of (j, i)
        const uint32_t first = static_cast<uint32_t>(i < j ? i : j), second = static_cast<uint32_t>(i < j ? j : i);
        const bool live_pair = j < a.G && j != i;
#pragma unroll
        for (int q = 0; q < kPermQ; ++q) {
            if (z * kPermQ + q >= a.np) continue;   // (wave-uniform; a guard, not a break: the counters stay fixed registers)
            const uint32_t gA = gtA[r][q], eA = TIES ? eqA[r][TIES ? q : 0] : 0u;
            const uint32_t gB = gtAll[r] - gA, eB = eqAll[r] - eA;
            const uint32_t upA = i < j ? gA : static_cast<uint32_t>(a.n1) - gA - eA;
            const uint32_t upB = i < j ? gB : static_cast<uint32_t>(a.n2) - gB - eB;
            const uint32_t na = upA + ((TIES && eA) ? tie_wins(a.seed, first, second, 0u, eA) : 0u);
            const uint32_t nb = upB + ((TIES && eB) ? tie_wins(a.seed, first, second, 1u, eB) : 0u);
            int ic = mp_side_class(static_cast<int32_t>(na), a.n1, a.m1, 0);
            int it = mp_side_class(static_cast<int32_t>(nb), a.n2, a.m2, 0);
            if (i > j) { ic = mp_mirror_side(ic); it = mp_mirror_side(it); }   // the class of (i, j) is 8 minus that of (j, i)
            const uint64_t cl = __ballot(live_pair && ic == 1), ch = __ballot(live_pair && ic == 3);
            const uint64_t tl = __ballot(live_pair && it == 1), th = __ballot(live_pair && it == 3);
            if (lane < 8) {
                const int plane = lane >> 1;
                const uint64_t w = plane == 0 ? cl : (plane == 1 ? ch : (plane == 2 ? tl : th));
                uint32_t *table = tables + static_cast<size_t>(z * kPermQ + q) * a.table_words;
                table[(static_cast<size_t>(i) * kPlanes + plane) * a.Wp + ctile * 2 + (lane & 1)] = static_cast<uint32_t>((lane & 1) ? (w >> 32) : w);
            }
        }
    }
}

// result: [15][G] of the pass that has just run on the permuted table (rows 0 pval, 1 padj, 11 delta1, 13 se, 14 z1)
__global__ __launch_bounds__(256) void k_perm_accumulate(const double *__restrict__ result, const double *__restrict__ d_obs, int64_t G, double pval_deg,
                                                         double padj_deg, int32_t *__restrict__ n_ge, int32_t *__restrict__ n_up,
                                                         int32_t *__restrict__ n_down, double *__restrict__ se)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    bool up = false, down = false;
    if (i < G) {
        if (pn_exceeds(result[11 * G + i], d_obs[i])) n_ge[i] += 1;   // (one thread per gene, one permutation per launch)
        const bool sig = result[i] <= pval_deg && result[G + i] <= padj_deg;
        const double z1 = result[14 * G + i];
        up = sig && z1 > 0.0;
        down = sig && z1 < 0.0;
        if (i == 0) *se = result[13 * G];
    }
    const uint64_t bu = __ballot(up), bd = __ballot(down);
    if ((threadIdx.x & 63) == 0) {
        if (bu) atomicAdd(n_up, static_cast<int32_t>(__popcll(bu)));
        if (bd) atomicAdd(n_down, static_cast<int32_t>(__popcll(bd)));
    }
}

}  // namespace

int32_t launch_perm_words(reo_ctx *c, const uint8_t *d_side, int64_t n_perm, const int32_t *d_slot2col, uint32_t *d_aw, uint32_t *d_live)
{
    if (!d_side || !d_slot2col || !d_aw || !d_live || n_perm < 1 || c->goff32.empty()) { set_error("reo_perm_null: no label rows on the device"); return REO_EINVAL; }
    const int nblk = c->goff32.back() / 32;
    if (nblk < 1 || nblk > 65535) { set_error("reo_perm_null: %d sample blocks cannot be launched", nblk); return REO_EINVAL; }
    REO_HIP_CHECK(hipMemsetAsync(d_aw, 0, pn_word_count(n_perm, nblk) * sizeof(uint32_t), c->stream));
    k_perm_words<<<dim3(static_cast<unsigned>((n_perm + 255) / 256), static_cast<unsigned>(nblk)), 256, 0, c->stream>>>(d_side, d_slot2col, c->S, n_perm, nblk,
                                                                                                                       d_aw, d_live);
    REO_HIP_CHECK(hipGetLastError());
    return REO_OK;
}

int32_t launch_pairs_permuted(reo_ctx *c, const uint32_t *d_aw, const uint32_t *d_live, int np, int n1, int n2, int m1, int m2,
                              uint32_t *d_tables)
{
    int32_t rc = need_planes(c, "reo_perm_null", kMpMaxGenes);
    if (rc) return rc;
    if (!d_aw || !d_live || !d_tables || np < 1) { set_error("reo_perm_null: bad batch"); return REO_EINVAL; }
    PnArgs a;
    a.G = static_cast<int>(c->G); a.Gp = c->Gp; a.Wp = c->Wp; a.nbits = plane_bits(c->G); a.nblk = c->goff32.back() / 32;
    a.n1 = n1; a.n2 = n2; a.m1 = m1; a.m2 = m2; a.np = np; a.seed = c->seed;
    a.table_words = static_cast<size_t>(c->G) * kPlanes * c->Wp;
    const dim3 grid = tile_grid(c->G, c->G, kPermRows, kPnWaves, (np + kPermQ - 1) / kPermQ);
    if (c->has_ties)
        k_pairs_permuted<true><<<grid, kPnThreads, 0, c->stream>>>(c->pos.p, c->lo.p, c->hi.p, d_aw, d_live, d_tables, a);
    else
        k_pairs_permuted<false><<<grid, kPnThreads, 0, c->stream>>>(c->pos.p, c->lo.p, c->hi.p, d_aw, d_live, d_tables, a);
    REO_HIP_CHECK(hipGetLastError());
    return REO_OK;
}

int32_t launch_perm_accumulate(reo_ctx *c, const double *d_obs, double pval_deg, double padj_deg, int32_t *d_n_ge, int32_t *d_n_up, int32_t *d_n_down,
                               double *d_se)
{
    if (!c->result.p || !d_obs || !d_n_ge || !d_n_up || !d_n_down || !d_se) { set_error("reo_perm_null: no pass result on the device"); return REO_EINVAL; }
    k_perm_accumulate<<<static_cast<unsigned>((c->G + 255) / 256), 256, 0, c->stream>>>(c->result.p, d_obs, c->G, pval_deg, padj_deg, d_n_ge, d_n_up, d_n_down, d_se);
    REO_HIP_CHECK(hipGetLastError());
    return REO_OK;
}

}  // namespace reo
