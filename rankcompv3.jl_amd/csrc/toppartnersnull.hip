// reo_top_partners_null: per (label permutation, query gene) the largest |N| over the gene's partners, the smallest partner that attains it
// and how many partners reach the row's cut, for a batch of permutations from ONE walk over the bit planes (semantics, the key, the batch
// rule and the host checks: top_partners_null.h; entry point: queries.hip; the A-words and the live word: launch_top_null_words of
// toppairsnull.hip, as they are).
//   k_top_partners_null<TIES, NB>   (NB = plane_bits(G) planes: a constant trip count of the chain)  the walk of k_top_pairs_null with the
//     query genes as its rows, as k_top_partners_count reads them: a wave owns 64 columns (lane = partner p) and kTnRows query rows, four
//     waves per workgroup take four neighbouring column tiles of the same rows, blockIdx.z is the launch group of kPermQ permutations.  The
//     rows are the genes genes[row0 + r], read through the row index -- wave-uniform, so a row's band edges, the live word and the kPermQ
//     A-words of the block stay scalar loads.  No i < j restriction and no tile skip: a query row meets every column.  The wave walks the
//     sample blocks with a live slot: a lane loads the 16 pos planes of its column once per block and keeps them for all rows.  Per (row,
//     block) there is one borrow chain (two with ties), then gt_all += popc(lt & live), gtA[q] += popc(lt & A[q]) and, with ties, the eq
//     counterparts from le & ~lt.  Side B is all - A.  The tie-free form (the transform reported no ties) carries no le chain and no eq
//     counters.  At the end, per (row, permutation): |N| through tp_num; the wave's maximum of |N| + 1 over its eligible lanes (0: none) by
//     shuffles, and the first lane that holds it -- lanes ascend with p, so that is the wave's smallest p and tprn_key of the two is the
//     wave's largest key; one LDS atomicMax per wave, and ONE 64-bit global atomicMax per workgroup into keys[perm][row]; with cuts a
//     ballot + popcount against the row's cut (a wave-uniform scalar) into a 32-bit LDS counter, flushed with one 32-bit global atomicAdd
//     per workgroup into reach[perm][row].
// Integer atomics only (max and add commute: the results do not depend on their arrival order); the kernel keeps no state between launches;
// there is no grid-wide synchronisation and no spinning; both barriers sit behind conditions on blockIdx and the arguments alone.
// Addresses: the query genes were checked on the host (0 <= q < G) and the array is padded with gene 0 up to a multiple of kTnRows: a
// launch reads genes[0 .. rows_padded), rows_padded = kTnRows gridDim.y; columns end at the next multiple of 64, below Gp (a multiple of
// 1024); the mask words are sized for Gp genes; the cuts have a word per padded row; blocks run over [0, nblk), the number of blocks the
// transform sliced and the A / live words were sized for; a launch group z < ceil(np / kPermQ) reads the words of its own group, which
// pn_word_count allocates whole (rows past np are zero, and nothing of them is stored); keys[(z kPermQ + q) stride + row] and reach[the same]
// are written only for z kPermQ + q < np <= the permutations the arrays hold and row < n_rows <= stride: padding rows store nothing.
// Counts are at most S <= 65535; a workgroup counts at most 4 * 64 partners per cell.
#include <algorithm>

#include "top_partners_null.h"
#include "reo_internal.h"
#include "band_chain.h"

namespace reo {

namespace {

constexpr int kTprnThreads = kTpWaves * 64;
constexpr int kTprnCells = kTnRows * kPermQ;   // (row, permutation) cells of a workgroup
static_assert(kGenePad % 64 == 0, "column tiles end inside the padded gene count");
static_assert(kTprnCells <= kTprnThreads, "a thread per cell flushes the workgroup's results");

struct TprnArgs {
    int G, Gp, nblk;
    int s_a, s_b;   // the sides' sizes: kept under every permutation
    int np;         // permutations of this launch
    int n_rows;     // query rows of this launch that are no padding
    int64_t stride; // rows of keys / reach per permutation
};

template <bool TIES, int NB>   // NB = plane_bits(G): 12, 15 or 16 planes
__global__ __launch_bounds__(kTprnThreads) void k_top_partners_null(const uint4 *__restrict__ P, const uint4 *__restrict__ AL, const uint4 *__restrict__ AH,
                                                                    const uint32_t *__restrict__ AW, const uint32_t *__restrict__ LW,
                                                                    const int32_t *__restrict__ genes, const uint32_t *__restrict__ maskbits,
                                                                    const uint32_t *__restrict__ cuts, unsigned long long *__restrict__ keys,
                                                                    uint32_t *__restrict__ reach, TprnArgs a)
{
    __shared__ unsigned long long best[kTprnCells];
    __shared__ uint32_t hits[kTprnCells];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
    const int ctile = static_cast<int>(blockIdx.x) * kTpWaves + wave;
    const int row0 = static_cast<int>(blockIdx.y) * kTnRows;   // of the launch; genes has a gene for every row of the grid
    const int z = static_cast<int>(blockIdx.z);
    if (z * kPermQ >= a.np) return;   // (workgroup-uniform, in front of every barrier)
    if (threadIdx.x < kTprnCells) { best[threadIdx.x] = 0; hits[threadIdx.x] = 0; }
    __syncthreads();
    if (ctile * 64 < a.G) {   // (wave-uniform)
        const int j = ctile * 64 + lane;   // < Gp
        int rows[kTnRows];
#pragma unroll
        for (int r = 0; r < kTnRows; ++r) rows[r] = __builtin_amdgcn_readfirstlane(genes[row0 + r]);   // (< G)
        const uint32_t *__restrict__ aw = AW + static_cast<size_t>(z) * a.nblk * kPermQ;
        constexpr int kEq = TIES ? kPermQ : 1;
        uint32_t gtA[kTnRows][kPermQ], eqA[kTnRows][kEq], gtAll[kTnRows], eqAll[kTnRows];
#pragma unroll
        for (int r = 0; r < kTnRows; ++r) {
            gtAll[r] = 0; eqAll[r] = 0;
#pragma unroll
            for (int q = 0; q < kPermQ; ++q) gtA[r][q] = 0;
#pragma unroll
            for (int q = 0; q < kEq; ++q) eqA[r][q] = 0;
        }
        for (int b = 0; b < a.nblk; ++b) {
            const uint32_t live = LW[b];
            if (live == 0) continue;   // (wave-uniform: a block of a group on neither side, or of padding alone)
            uint32_t p[16];
            const uint4 *pb = P + static_cast<size_t>(b) * 4 * a.Gp + j;
#pragma unroll
            for (int q = 0; q < 4; ++q) band_unpack(pb[static_cast<size_t>(q) * a.Gp], p, q);
            uint32_t A[kPermQ];
#pragma unroll
            for (int q = 0; q < kPermQ; ++q) A[q] = aw[static_cast<size_t>(b) * kPermQ + q];
#pragma unroll
            for (int r = 0; r < kTnRows; ++r) {
                const size_t row = (static_cast<size_t>(b) * a.Gp + rows[r]) * 4;
                uint32_t lo[16], hi[16];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    band_unpack(AL[row + q], lo, q);
                    if (TIES) band_unpack(AH[row + q], hi, q);
                }
                uint32_t lt = 0, le = 0;
#pragma unroll
                for (int k = 0; k < NB; ++k) {
                    const int ew = BandLayout<false>::edge_word(k);
                    lt = band_borrow(p[k], lo[ew], lt);
                    if (TIES) le = band_borrow(p[k], hi[ew], le);
                }
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
        bool elig[kTnRows];
        uint32_t cut[kTnRows];
#pragma unroll
        for (int r = 0; r < kTnRows; ++r) {
            elig[r] = row0 + r < a.n_rows && tprn_eligible(j, rows[r], a.G, maskbits);
            cut[r] = cuts ? cuts[row0 + r] : 0u;   // (wave-uniform; read only with cuts)
        }
#pragma unroll
        for (int q = 0; q < kPermQ; ++q) {
            if (z * kPermQ + q >= a.np) continue;   // (wave-uniform; a guard, not a break: the counters stay fixed registers)
#pragma unroll
            for (int r = 0; r < kTnRows; ++r) {
                uint32_t gA = gtA[r][q], eA = TIES ? eqA[r][TIES ? q : 0] : 0u;
                // a COPY of the counters goes into tp_num's 64-bit arithmetic, as in k_top_pairs_null: widened where they stand, every
                // counter is the low half of a register pair through the whole count loop
                if (TIES) asm volatile("" : "+v"(gA), "+v"(eA));
                else asm volatile("" : "+v"(gA));
                const uint32_t gB = gtAll[r] - gA, eB = eqAll[r] - eA;
                const uint32_t n = static_cast<uint32_t>(tp_abs(tp_num(static_cast<int32_t>(gA), static_cast<int32_t>(eA), static_cast<int32_t>(gB),
                                                                       static_cast<int32_t>(eB), a.s_a, a.s_b)));   // |N| < 2^31
                if (cuts) {   // (wave-uniform)
                    const uint32_t cnt = static_cast<uint32_t>(__builtin_popcountll(__ballot(elig[r] && n >= cut[r])));
                    if (cnt != 0 && lane == 0) atomicAdd(&hits[r * kPermQ + q], cnt);
                }
                const uint32_t mine = elig[r] ? n + 1u : 0u;
                uint32_t top = mine;
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) {
                    const uint32_t o = __shfl_xor(top, d);
                    top = o > top ? o : top;
                }
                if (top != 0) {   // (wave-uniform: every lane holds the wave's maximum)
                    const int first = __builtin_ctzll(__ballot(mine == top));   // (lanes ascend with p: the smallest p of the maximum)
                    if (lane == 0) atomicMax(&best[r * kPermQ + q], static_cast<unsigned long long>(tprn_key(top - 1u, ctile * 64 + first)));
                }
            }
        }
    }
    __syncthreads();
    const int t = static_cast<int>(threadIdx.x);
    if (t < kTprnCells) {
        const int r = t / kPermQ, q = t % kPermQ;
        if (row0 + r < a.n_rows && z * kPermQ + q < a.np) {
            const size_t at = static_cast<size_t>(z * kPermQ + q) * static_cast<size_t>(a.stride) + static_cast<size_t>(row0 + r);
            if (best[t] != 0) atomicMax(&keys[at], best[t]);
            if (cuts && hits[t] != 0) atomicAdd(&reach[at], hits[t]);
        }
    }
}

template <bool TIES>
void tprn_launch(reo_ctx *c, const dim3 &g, const uint32_t *d_aw, const uint32_t *d_live, const int32_t *d_genes, const uint32_t *d_maskbits,
                 const uint32_t *d_cuts, unsigned long long *d_keys, uint32_t *d_reach, const TprnArgs &a)
{
    with_plane_bits(c->G, [&](auto nb) {
        k_top_partners_null<TIES, decltype(nb)::value><<<g, kTprnThreads, 0, c->stream>>>(c->pos.p, c->lo.p, c->hi.p, d_aw, d_live, d_genes, d_maskbits,
                                                                                         d_cuts, d_keys, d_reach, a);
    });
}

}  // namespace

int32_t launch_top_partners_null(reo_ctx *c, const uint32_t *d_aw, const uint32_t *d_live, int np, int s_a, int s_b, const int32_t *d_genes,
                                 int64_t n_genes, const uint32_t *d_maskbits, const uint32_t *d_cuts, unsigned long long *d_keys, uint32_t *d_reach)
{
    int32_t rc = need_planes(c, "reo_top_partners_null", kTpMaxGenes);
    if (rc) return rc;
    if (!d_aw || !d_live || !d_genes || !d_keys || !d_reach || np < 1 || np > kTprnBatchCap || n_genes < 1 || n_genes > kTprnMaxGenes) {
        set_error("reo_top_partners_null: bad batch");
        return REO_EINVAL;
    }
    const int64_t padded = tprn_padded_rows(n_genes);
    constexpr int64_t kRowsPerLaunch = int64_t(65535) * kTnRows;   // (grid y)
    TprnArgs a;
    a.G = static_cast<int>(c->G); a.Gp = c->Gp; a.nblk = c->goff32.back() / 32;
    a.s_a = s_a; a.s_b = s_b; a.np = np; a.stride = padded;
    for (int64_t r0 = 0; r0 < padded; r0 += kRowsPerLaunch) {
        const int64_t rows = std::min(kRowsPerLaunch, padded - r0);   // (a multiple of kTnRows)
        a.n_rows = static_cast<int>(std::min(rows, n_genes - r0));
        const dim3 grid = tile_grid(c->G, rows, kTnRows, kTpWaves, (np + kPermQ - 1) / kPermQ);
        const uint32_t *cuts = d_cuts ? d_cuts + r0 : nullptr;
        if (c->has_ties) tprn_launch<true>(c, grid, d_aw, d_live, d_genes + r0, d_maskbits, cuts, d_keys + r0, d_reach + r0, a);
        else tprn_launch<false>(c, grid, d_aw, d_live, d_genes + r0, d_maskbits, cuts, d_keys + r0, d_reach + r0, a);
        REO_HIP_CHECK(hipGetLastError());
    }
    return REO_OK;
}

}  // namespace reo
