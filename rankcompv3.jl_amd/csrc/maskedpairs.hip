// Missing values: the class table from the samples where both genes of a pair were observed (reo_build_pairs_masked; semantics, shared
// arithmetic and host checks: masked_pairs.h; entry points: api.hip).
//   k_valid_words    the byte mask [S][G] (caller's column order) into one 32-bit validity word per (block of 32 sample slots, gene) in slot
//     order, [sample blocks][Gp]: a thread owns a gene and gathers the 32 bytes of its block's columns through the slot -> column map
//     (consecutive threads read consecutive bytes of a column), then stores the word.  Padding slots and genes >= G give 0.
//   k_pairs_masked   the hot path.  A wave owns 64 table columns (lane = gene j) and kMpRows table rows; four waves per workgroup take four
//     neighbouring column tiles of the same rows.  The wave walks the groups and their blocks of 32 sample slots: a lane loads the 16 pos
//     planes and the validity word of its column once per block and keeps them in registers for all rows of the tile; the band edges lo_i /
//     hi_i and the validity word of a row are wave-uniform (__restrict__ arguments: scalar loads).  The borrow chain of band_chain.h gives lt
//     and le, and with v = V_i & V_j the counts are popcount(lt & v), popcount(le & ~lt & v), popcount(v).  At a group's end the lane draws
//     the group's coins and adds the group to its side.  EVERY ordered pair is evaluated from its own row: below the diagonal (i > j) the
//     lane forms the counts of the pair (j, i) from its own -- gt(j, i) = n - gt - eq, the coin keyed by the smaller index first -- and
//     stores 8 minus its class, so there is no mirror store and no atomic.  The four plane words of the 64 columns come from ballots; lanes
//     0 .. 7 store the eight 32-bit words into row i of the [G][4][Wp] table (bit meaning: pair_list.h).  The diagonal and the columns >= G
//     stay 0; the table words of the columns past the last tile are cleared by the caller's memset.
//   k_counts_masked  the parity hook: the same counting code with a store instead of the classification, one thread per pair of a rectangle.
// Integer arithmetic only and a fixed assignment of pairs to lanes: deterministic.  Addresses: rows and columns of the planes and of the
// validity words are below Gp (the row tiles end at the next multiple of kMpRows, the column tiles at the next multiple of 64, Gp is a
// multiple of 1024); blocks are bounded by the group offsets of the transform; the threshold tables are indexed by a count clamped to
// the side's size; table rows >= G are never stored.
#include "masked_pairs.h"
#include "reo_internal.h"
#include "band_chain.h"
#include "tie_coin.h"

namespace reo {

namespace {

constexpr int kMpThreads = 256;
constexpr int kMpWaves = kMpThreads / 64;
static_assert(kGenePad % kMpRows == 0 && kGenePad % 64 == 0, "row and column tiles end inside the padded gene count");

__global__ __launch_bounds__(256) void k_valid_words(const uint8_t *__restrict__ valid, const int32_t *__restrict__ slot2col, int64_t G, int64_t S,
                                                     int Gp, uint32_t *__restrict__ words)
{
    const int gene = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x), b = static_cast<int>(blockIdx.y);
    if (gene >= Gp) return;
    words[static_cast<size_t>(b) * Gp + gene] = mp_valid_word(valid, G, S, gene, slot2col + static_cast<size_t>(b) * 32);
}

struct MpArgs {
    int G, Gp, Wp, nbits, ngroups, k;
    int n1, n2;        // the sides' sizes: the last index of their threshold tables
    int mc1, mc2;      // min_complete
    uint64_t seed;
};

__global__ __launch_bounds__(kMpThreads) void k_pairs_masked(const uint4 *__restrict__ P, const uint4 *__restrict__ AL, const uint4 *__restrict__ AH,
                                                             const uint32_t *__restrict__ VW, const int32_t *__restrict__ goff,
                                                             const int32_t *__restrict__ m1, const int32_t *__restrict__ m2,
                                                             uint32_t *__restrict__ table, MpArgs a)
{
    const int lane = threadIdx.x & 63;
    const int ctile = static_cast<int>(blockIdx.x) * kMpWaves + __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
    const int i0 = static_cast<int>(blockIdx.y) * kMpRows;
    if (ctile * 64 >= a.G || i0 >= a.G) return;   // (wave-uniform; the kernel has no barrier)
    const int j = ctile * 64 + lane;              // < Gp
    uint32_t A[kMpRows], N1[kMpRows], B[kMpRows], N2[kMpRows];
#pragma unroll
    for (int r = 0; r < kMpRows; ++r) { A[r] = 0; N1[r] = 0; B[r] = 0; N2[r] = 0; }
    for (int g = 0; g < a.ngroups; ++g) {
        uint32_t gt[kMpRows], eq[kMpRows], nv[kMpRows];
#pragma unroll
        for (int r = 0; r < kMpRows; ++r) { gt[r] = 0; eq[r] = 0; nv[r] = 0; }
        const int b1 = goff[g + 1];
        for (int b = goff[g]; b < b1; ++b) {
            uint32_t p[16];
            band_load_pos<false>(P, a.Gp, b, j, p);
            const uint32_t *vb = VW + static_cast<size_t>(b) * a.Gp;
            const uint32_t vj = vb[j];
#pragma unroll
            for (int r = 0; r < kMpRows; ++r) {
                const size_t row = band_edge_row<false>(a.Gp, b, i0 + r);   // (i0 + r < Gp)
                uint32_t lt, le;
                band_compare<false, true, kBandGuard>(p, AL + row, AH + row, lt, le, a.nbits);
                mp_count_block(lt, le, vb[i0 + r] & vj, gt[r], eq[r], nv[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < kMpRows; ++r) {
            const int i = i0 + r;
            // the pair with the smaller index first: above the diagonal the lane's own counts, below it those of (j, i)
            const uint32_t first = static_cast<uint32_t>(i < j ? i : j), second = static_cast<uint32_t>(i < j ? j : i);
            const uint32_t up = i < j ? gt[r] : nv[r] - gt[r] - eq[r];
            const uint32_t nre = up + (eq[r] ? tie_wins(a.seed, first, second, static_cast<uint32_t>(g), eq[r]) : 0u);
            if (g == a.k) { A[r] += nre; N1[r] += nv[r]; }
            else { B[r] += nre; N2[r] += nv[r]; }
        }
    }
#pragma unroll
    for (int r = 0; r < kMpRows; ++r) {
        const int i = i0 + r;
        if (i >= a.G) break;   // (wave-uniform)
        const int n1 = static_cast<int>(N1[r]) < a.n1 ? static_cast<int>(N1[r]) : a.n1, n2 = static_cast<int>(N2[r]) < a.n2 ? static_cast<int>(N2[r]) : a.n2;
        int ic = mp_side_class(static_cast<int32_t>(A[r]), n1, m1[n1], a.mc1);
        int it = mp_side_class(static_cast<int32_t>(B[r]), n2, m2[n2], a.mc2);
        if (i > j) { ic = mp_mirror_side(ic); it = mp_mirror_side(it); }   // the class of (i, j) is 8 minus that of (j, i)
        const bool live = j < a.G && j != i;
        const uint64_t cl = __ballot(live && ic == 1), ch = __ballot(live && ic == 3);
        const uint64_t tl = __ballot(live && it == 1), th = __ballot(live && it == 3);
        if (lane < 8) {
            const int plane = lane >> 1;
            const uint64_t w = plane == 0 ? cl : (plane == 1 ? ch : (plane == 2 ? tl : th));
            table[(static_cast<size_t>(i) * kPlanes + plane) * a.Wp + ctile * 2 + (lane & 1)] = static_cast<uint32_t>((lane & 1) ? (w >> 32) : w);
        }
    }
}

__global__ __launch_bounds__(256) void k_counts_masked(const uint4 *__restrict__ P, const uint4 *__restrict__ AL, const uint4 *__restrict__ AH,
                                                       const uint32_t *__restrict__ VW, const int32_t *__restrict__ goff, int Gp, int nbits,
                                                       int ngroups, int ci0, int ci1, int cj0, int cj1, int32_t *__restrict__ out_gt,
                                                       int32_t *__restrict__ out_eq, int32_t *__restrict__ out_n)
{
    const int j = cj0 + static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x), i = ci0 + static_cast<int>(blockIdx.y);
    if (j >= cj1 || i >= ci1) return;
    const int nj = cj1 - cj0;
    for (int g = 0; g < ngroups; ++g) {
        uint32_t n_gt = 0, n_eq = 0, n_av = 0;
        for (int b = goff[g]; b < goff[g + 1]; ++b) {
            uint32_t p[16], lt, le;
            const uint4 *pb = P + static_cast<size_t>(b) * 4 * Gp + j;
#pragma unroll
            for (int q = 0; q < 4; ++q) band_unpack(pb[static_cast<size_t>(q) * Gp], p, q);
            const size_t row = static_cast<size_t>(b) * Gp + i;
            // (row * EQ and not band_edge_row: the row is the index of the validity words too, and the other spelling reorders this kernel)
            band_compare<false, true, kBandGuard>(p, AL + row * BandLayout<false>::EQ, AH + row * BandLayout<false>::EQ, lt, le, nbits);
            mp_count_block(lt, le, VW[row] & VW[static_cast<size_t>(b) * Gp + j], n_gt, n_eq, n_av);
        }
        const size_t o = (static_cast<size_t>(i - ci0) * nj + (j - cj0)) * ngroups + g;
        out_gt[o] = static_cast<int32_t>(n_gt);
        out_eq[o] = static_cast<int32_t>(n_eq);
        out_n[o] = static_cast<int32_t>(n_av);
    }
}

// the guard of the plane readers and the validity words on top; one text for either miss (ensure_planes never gives REO_EINVAL)
int32_t mp_need_planes(reo_ctx *c, const char *what)
{
    const int32_t rc = c->vwords.p ? need_planes(c, what, kMpMaxGenes) : REO_EINVAL;
    if (rc == REO_EINVAL) set_error("%s: no bit planes or no validity words", what);
    return rc;
}

}  // namespace

int32_t launch_valid_words(reo_ctx *c, const int32_t *d_slot2col)
{
    if (!c->vmask.p || !c->vwords.p || !d_slot2col || c->goff32.empty()) { set_error("reo_build_pairs_masked: no validity mask on the device"); return REO_EINVAL; }
    const int nblk = c->goff32.back() / 32;
    if (nblk < 1 || nblk > 65535) { set_error("reo_build_pairs_masked: %d sample blocks cannot be launched", nblk); return REO_EINVAL; }
    k_valid_words<<<dim3(static_cast<unsigned>(c->Gp / 256), static_cast<unsigned>(nblk)), 256, 0, c->stream>>>(c->vmask.p, d_slot2col, c->G, c->S, c->Gp,
                                                                                                               c->vwords.p);
    REO_HIP_CHECK(hipGetLastError());
    return REO_OK;
}

int32_t launch_pairs_masked(reo_ctx *c, int k, const int32_t *d_m1, int n1, const int32_t *d_m2, int n2, int min_complete1, int min_complete2)
{
    int32_t rc = mp_need_planes(c, "reo_build_pairs_masked");
    if (rc) return rc;
    if (!d_m1 || !d_m2 || n1 < 0 || n2 < 0 || k < 0 || k >= c->ngroups) { set_error("reo_build_pairs_masked: no threshold tables"); return REO_EINVAL; }
    MpArgs a;
    a.G = static_cast<int>(c->G); a.Gp = c->Gp; a.Wp = c->Wp; a.nbits = plane_bits(c->G); a.ngroups = c->ngroups; a.k = k;
    a.n1 = n1; a.n2 = n2; a.mc1 = min_complete1; a.mc2 = min_complete2; a.seed = c->seed;
    k_pairs_masked<<<tile_grid(c->G, c->G, kMpRows, kMpWaves), kMpThreads, 0, c->stream>>>(c->pos.p, c->lo.p, c->hi.p, c->vwords.p, c->goff_dev.p, d_m1, d_m2,
                                                                                           c->table.p, a);
    REO_HIP_CHECK(hipGetLastError());
    return REO_OK;
}

int32_t launch_counts_masked(reo_ctx *c, int64_t i0, int64_t i1, int64_t j0, int64_t j1, int32_t *d_gt, int32_t *d_eq, int32_t *d_avail)
{
    int32_t rc = mp_need_planes(c, "reo_pair_counts_masked");
    if (rc) return rc;
    if (i0 < 0 || j0 < 0 || i1 > c->G || j1 > c->G || i0 >= i1 || j0 >= j1 || i1 - i0 > 65535) { set_error("reo_pair_counts_masked: bad pair block"); return REO_EINVAL; }
    const dim3 grid(static_cast<unsigned>((j1 - j0 + 255) / 256), static_cast<unsigned>(i1 - i0));
    k_counts_masked<<<grid, 256, 0, c->stream>>>(c->pos.p, c->lo.p, c->hi.p, c->vwords.p, c->goff_dev.p, c->Gp, plane_bits(c->G), c->ngroups,
                                                 static_cast<int>(i0), static_cast<int>(i1), static_cast<int>(j0), static_cast<int>(j1), d_gt, d_eq, d_avail);
    REO_HIP_CHECK(hipGetLastError());
    return REO_OK;
}

}  // namespace reo
