// reo_top_partners: the best m partner genes of every query gene (semantics, the cell, the row key, the batch rule and the host checks:
// top_partners.h; entry point: queries.hip).
//   k_top_partners_count<NB>   (NB = plane_bits(G) planes)  the walk of k_top_pairs (toppairs.hip) with the query genes as its rows: a wave owns
//     64 columns (lane = partner p) and kTpRows query rows, four waves per workgroup take four neighbouring column tiles of the same rows.
//     The rows are the genes genes[row0 + r], read through the row index instead of blockIdx.y * kTpRows -- wave-uniform, so the band edges
//     of a row are still scalar loads; the count loop is tp_count_side (top_count.h) with that row index.  No i < j
//     restriction and no tile skip: a query row meets every column.  Side A's groups, then side B's; per (row, column) the lane packs
//     gt_A, eq_A, gt_B, eq_B of "query above column" into one TprCell and stores it at cells[row of the batch][Gp]: one coalesced 64-bit
//     store per lane.
//   k_top_partners_select   one workgroup per query row, m_want rounds.  A round strides over the row's cells, forms the key (|N|, Gamma, p)
//     of every eligible column (p != q, p < G, inside the mask) from the cell, D[q] and D[p], and keeps the one that comes first in the
//     row's order among those strictly behind the previous round's winner; a reduction through LDS finds the workgroup's.  The keys of a
//     row are unique (they hold p), so the rounds enumerate the order exactly, whatever the thread count.  Thread 0 stores partner, counts
//     and key of the round.  A round that finds nothing ends the row; thread 0 fills what is left with -1 / 0 and stores n_found.
// Integer arithmetic only, no atomics, no state between launches, no grid-wide synchronisation.  Addresses: the query genes were checked on
// the host (0 <= q < G) and the array is padded with gene 0 up to a multiple of kTpRows; columns end at the next multiple of 64, below Gp
// (a multiple of 1024); a batch's cells have tpr_padded_rows rows of Gp columns; D is sized for Gp genes; blocks are bounded by the group
// offsets of the transform; the outputs have m_want entries per row of the batch.
#include "top_partners.h"
#include "reo_internal.h"
#include "top_count.h"

namespace reo {

namespace {

constexpr int kTprCountThreads = kTpWaves * 64;
static_assert(kGenePad % 64 == 0, "column tiles end inside the padded gene count");
static_assert(kTprThreads % 64 == 0 && (kTprThreads & (kTprThreads - 1)) == 0, "the tree reduction halves the workgroup");

struct TprArgs {
    int G, Gp, ngroups;
    int s_a, s_b;
    int m_want;
};

template <int NB>   // NB = plane_bits(G): 12, 15 or 16 planes
__global__ __launch_bounds__(kTprCountThreads) void k_top_partners_count(const uint4 *__restrict__ P, const uint4 *__restrict__ AL,
                                                                         const uint4 *__restrict__ AH, const int32_t *__restrict__ goff,
                                                                         const int32_t *__restrict__ gside, const int32_t *__restrict__ genes,
                                                                         unsigned long long *__restrict__ cells, TprArgs a)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
    const int ctile = static_cast<int>(blockIdx.x) * kTpWaves + wave;
    if (ctile * 64 >= a.G) return;   // (wave-uniform; no barrier in this kernel)
    const int row0 = static_cast<int>(blockIdx.y) * kTpRows;   // of the batch; genes has a gene for every row of the grid
    const int j = ctile * 64 + lane;                           // < Gp
    int rows[kTpRows];
#pragma unroll
    for (int r = 0; r < kTpRows; ++r) rows[r] = __builtin_amdgcn_readfirstlane(genes[row0 + r]);
    uint32_t gt_a[kTpRows], le_a[kTpRows], gt_b[kTpRows], le_b[kTpRows];
#pragma unroll
    for (int r = 0; r < kTpRows; ++r) { gt_a[r] = 0; le_a[r] = 0; gt_b[r] = 0; le_b[r] = 0; }
    const auto row_of = [&rows](int r) { return rows[r]; };   // (rows[r] < G)
    tp_count_side<NB>(P, AL, AH, goff, gside, 0, j, row_of, a, gt_a, le_a);
    tp_count_side<NB>(P, AL, AH, goff, gside, 1, j, row_of, a, gt_b, le_b);
#pragma unroll
    for (int r = 0; r < kTpRows; ++r)
        cells[static_cast<size_t>(row0 + r) * a.Gp + j] = tpr_pack(gt_a[r], le_a[r] - gt_a[r], gt_b[r], le_b[r] - gt_b[r]);
}

__global__ __launch_bounds__(kTprThreads) void k_top_partners_select(const unsigned long long *__restrict__ cells, const int32_t *__restrict__ genes,
                                                                     const int64_t *__restrict__ D, const uint32_t *__restrict__ maskbits,
                                                                     int32_t *__restrict__ partner, int32_t *__restrict__ counts,
                                                                     int64_t *__restrict__ key, int32_t *__restrict__ n_found, TprArgs a)
{
    __shared__ TprKey best[kTprThreads];
    const int t = static_cast<int>(threadIdx.x);
    const size_t row = blockIdx.x;   // of the batch
    const int32_t q = genes[row];
    const int64_t dq = D[q];
    const unsigned long long *cell = cells + row * static_cast<size_t>(a.Gp);
    TprKey prev{0, 0, -1};
    int found = 0;
    for (; found < a.m_want; ++found) {   // (every exit of the loop is workgroup-uniform: it follows what best[0] holds)
        TprKey mine{0, 0, -1};
        for (int p = t; p < a.G; p += kTprThreads) {
            if (!tpr_eligible(p, q, a.G, maskbits)) continue;
            const TprKey cand = tpr_key(tpr_unpack(cell[p]), dq, D[p], p, a.s_a, a.s_b);
            if (tpr_takes(cand, prev, mine)) mine = cand;
        }
        best[t] = mine;
        __syncthreads();
        for (int half = kTprThreads / 2; half > 0; half >>= 1) {
            if (t < half) {
                const TprKey other = best[t + half];
                if (other.p >= 0 && (best[t].p < 0 || tpr_before(other, best[t]))) best[t] = other;
            }
            __syncthreads();
        }
        const TprKey win = best[0];
        __syncthreads();   // (best is written again in the next round)
        if (win.p < 0) break;
        if (t == 0) {
            const size_t at = row * static_cast<size_t>(a.m_want) + static_cast<size_t>(found);
            const TprCell c = tpr_unpack(cell[win.p]);
            partner[at] = win.p;
            counts[4 * at] = c.gt_a; counts[4 * at + 1] = c.eq_a; counts[4 * at + 2] = c.gt_b; counts[4 * at + 3] = c.eq_b;
            key[2 * at] = tpr_num(c, a.s_a, a.s_b);
            key[2 * at + 1] = static_cast<int64_t>(win.gamma);
        }
        prev = win;
    }
    if (t == 0) {
        for (int e = found; e < a.m_want; ++e) {
            const size_t at = row * static_cast<size_t>(a.m_want) + static_cast<size_t>(e);
            partner[at] = -1;
            counts[4 * at] = 0; counts[4 * at + 1] = 0; counts[4 * at + 2] = 0; counts[4 * at + 3] = 0;
            key[2 * at] = 0; key[2 * at + 1] = 0;
        }
        n_found[row] = found;
    }
}

TprArgs tpr_args(reo_ctx *c, int s_a, int s_b, int m_want)
{
    TprArgs a;
    a.G = static_cast<int>(c->G); a.Gp = c->Gp; a.ngroups = c->ngroups;
    a.s_a = s_a; a.s_b = s_b; a.m_want = m_want;
    return a;
}

}  // namespace

int32_t launch_top_partners_count(reo_ctx *c, const int32_t *d_gside, int s_a, int s_b, const int32_t *d_genes, int64_t n_rows,
                                  unsigned long long *d_cells)
{
    int32_t rc = need_planes(c, "reo_top_partners", kTpMaxGenes);
    if (rc) return rc;
    if (n_rows < kTpRows || n_rows % kTpRows || n_rows / kTpRows > 65535 || !d_genes || !d_cells) {   // (grid y; the budget allows 32 768 rows)
        set_error("reo_top_partners: a batch of %lld rows is no multiple of %d or more than one launch takes", (long long)n_rows, kTpRows);
        return REO_EINVAL;
    }
    const TprArgs a = tpr_args(c, s_a, s_b, 0);
    with_plane_bits(c->G, [&](auto nb) {
        k_top_partners_count<decltype(nb)::value><<<tile_grid(c->G, n_rows, kTpRows, kTpWaves), kTprCountThreads, 0, c->stream>>>(
            c->pos.p, c->lo.p, c->hi.p, c->goff_dev.p, d_gside, d_genes, d_cells, a);
    });
    REO_HIP_CHECK(hipGetLastError());
    return REO_OK;
}

int32_t launch_top_partners_select(reo_ctx *c, const unsigned long long *d_cells, const int32_t *d_genes, int64_t n_rows, const int64_t *d_D,
                                   const uint32_t *d_maskbits, int s_a, int s_b, int m_want, int32_t *d_partner, int32_t *d_counts, int64_t *d_key,
                                   int32_t *d_found)
{
    if (n_rows < 1 || n_rows > kTprMaxGenes || m_want < 1 || m_want > kTprMaxWant || !d_cells || !d_genes || !d_D || !d_partner || !d_counts || !d_key ||
        !d_found) {
        set_error("reo_top_partners: %lld rows of %d partners cannot be selected", (long long)n_rows, m_want);
        return REO_EINVAL;
    }
    k_top_partners_select<<<static_cast<unsigned>(n_rows), kTprThreads, 0, c->stream>>>(d_cells, d_genes, d_D, d_maskbits, d_partner, d_counts, d_key,
                                                                                        d_found, tpr_args(c, s_a, s_b, m_want));
    REO_HIP_CHECK(hipGetLastError());
    return REO_OK;
}

}  // namespace reo
