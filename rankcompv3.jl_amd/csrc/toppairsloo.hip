// reo_top_pairs_loo: leave-one-out cross-validation of the k-TSP selection, every fold decided from one set of candidates (semantics, the
// fold arithmetic, the cut rule and the host checks: top_pairs_loo.h; entry point: queries.hip).
//   k_loo_words<NB>   one thread per candidate record (TpRec of the emit pass of k_top_pairs, resident on the device) and, in grid y, per
//     block of 32 sample slots.  The borrow chain of band_chain.h over NB = plane_bits(G) planes, as pairsupport.hip runs it for listed
//     pairs: lo / hi of gene_i against the pos planes of gene_j give lt and le; the thread stores the gt word (lt) and the eq word
//     (le & ~lt) as one uint2 at [block][candidate].  Padding slots read as zero in the planes: their bits are zero.
//   k_loo_select   one workgroup per sample slot; a slot without a column or of a group on neither side ends at once.  The workgroup
//     holds a used-gene bitmap in LDS (8 KB) and runs kmax rounds.  A round has two scans in which the threads stride over the candidates
//     and skip those with a used gene: the first forms the fold's counts (the full counts minus the slot's bit on its side) and reduces
//     max |N(s)|; the second computes Gamma(s) -- lo + hi of both genes in the slot, extracted from the edge planes, taken from the genes'
//     sums of k_rank_shift -- only for the candidates at that maximum and reduces (Gamma, index key).  Reductions: wave shuffles, then LDS.
//     The winner's genes are marked; thread 0 stores the pick into row slot2col[slot].
// Integer arithmetic only, no atomics, no state between launches, no grid-wide synchronisation.  The comparison is the total order of
// loo_before: the result does not depend on the order of the candidates.  Addresses: candidates are bounded by n_cand; their genes were
// checked by the emit pass (i < j < G); blocks by the group offsets of the transform (grid y = blocks, grid x of the select = 32 blocks
// slots); rows of the outputs by slot2col in [0, S); the bitmap holds 65 536 genes and G <= 65 535.
#include "top_pairs_loo.h"
#include "reo_internal.h"
#include "band_chain.h"

namespace reo {

namespace {

constexpr int kLooWaves = kLooThreads / 64;

struct LooArgs {
    int G, Gp, ngroups, kmax;
    uint32_t n_cand;
    int s_a, s_b;
    int64_t S;
};

template <int NB>
__global__ __launch_bounds__(kLooThreads) void k_loo_words(const TpRec *__restrict__ cand, const uint4 *__restrict__ P, const uint4 *__restrict__ AL,
                                                           const uint4 *__restrict__ AH, uint2 *__restrict__ words, int Gp, uint32_t n_cand)
{
    const uint32_t cnd = blockIdx.x * static_cast<uint32_t>(kLooThreads) + threadIdx.x;
    if (cnd >= n_cand) return;
    const int b = static_cast<int>(blockIdx.y);
    const TpRec r = cand[cnd];
    uint32_t p[16], lo[16], hi[16], lt, le;
    band_load_pos<false>(P, Gp, b, r.j, p);
    band_load_edges<false, true>(AL, AH, band_edge_row<false>(Gp, b, r.i), lo, hi);
    band_chain<false, true, NB>(p, lo, hi, lt, le);
    words[loo_word_index(b, cnd, n_cand)] = make_uint2(lt, le & ~lt);
}

// lo + hi of gene g in bit t of block b, from the edge planes.
__device__ __forceinline__ int64_t loo_edge_sum(const uint4 *__restrict__ AL, const uint4 *__restrict__ AH, int Gp, int b, int g, int t)
{
    uint32_t lo[16], hi[16], v = 0;
    band_load_edges<false, true>(AL, AH, band_edge_row<false>(Gp, b, g), lo, hi);
#pragma unroll
    for (int k = 0; k < 16; ++k) v += band_edge_term<uint32_t>(lo, hi, k, BandBit{t});
    return static_cast<int64_t>(v);
}

__device__ __forceinline__ unsigned long long loo_shfl_xor(unsigned long long v, int m)
{
    const int lo = __shfl_xor(static_cast<int>(v & 0xFFFFFFFFull), m), hi = __shfl_xor(static_cast<int>(v >> 32), m);
    return (static_cast<unsigned long long>(static_cast<uint32_t>(hi)) << 32) | static_cast<uint32_t>(lo);
}

__global__ __launch_bounds__(kLooThreads) void k_loo_select(const TpRec *__restrict__ cand, const uint2 *__restrict__ words,
                                                            const uint4 *__restrict__ AL, const uint4 *__restrict__ AH,
                                                            const int32_t *__restrict__ goff, const int32_t *__restrict__ gside,
                                                            const int32_t *__restrict__ slot2col, const int64_t *__restrict__ sums,
                                                            int32_t *__restrict__ out_i, int32_t *__restrict__ out_j, int64_t *__restrict__ out_n,
                                                            int64_t *__restrict__ out_g, int8_t *__restrict__ out_o, LooArgs a)
{
    __shared__ uint32_t used[kLooUsedWords];
    __shared__ unsigned long long red_x[kLooWaves], red_y[kLooWaves];
    const int slot = static_cast<int>(blockIdx.x), b = slot >> 5, t = slot & 31;
    const int col = slot2col[slot];
    if (col < 0 || col >= a.S) return;   // (workgroup-uniform, in front of every barrier: a padding slot)
    int side = 2;
    for (int g = 0; g < a.ngroups; ++g)
        if (b >= goff[g] && b < goff[g + 1]) side = gside[g];
    if (side > 1) return;                // (workgroup-uniform: a sample of neither side is no fold)
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    for (int w = tid; w < kLooUsedWords; w += kLooThreads) used[w] = 0;
    __syncthreads();
    const uint2 *wb = words + loo_word_index(b, 0, a.n_cand);
    for (int r = 0; r < a.kmax; ++r) {
        // scan 1: max |N(s)| over the candidates whose genes are free; -1 -> 0 when there is none (|N| + 1 is reduced)
        unsigned long long best = 0;
        for (uint32_t cnd = static_cast<uint32_t>(tid); cnd < a.n_cand; cnd += kLooThreads) {
            const TpRec rec = cand[cnd];
            if (((used[rec.i >> 5] >> (rec.i & 31)) | (used[rec.j >> 5] >> (rec.j & 31))) & 1u) continue;
            const uint2 w = wb[cnd];
            const unsigned long long n1 = tp_abs(loo_num(rec, side, (w.x >> t) & 1u, (w.y >> t) & 1u, a.s_a, a.s_b)) + 1ull;
            best = n1 > best ? n1 : best;
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const unsigned long long o = loo_shfl_xor(best, m);
            best = o > best ? o : best;
        }
        if (lane == 0) red_x[wave] = best;
        __syncthreads();
        best = red_x[0];
#pragma unroll
        for (int w = 1; w < kLooWaves; ++w) best = red_x[w] > best ? red_x[w] : best;
        __syncthreads();                 // (red_x is written again below)
        if (best == 0) break;            // (workgroup-uniform: every remaining candidate has a used gene; the rows keep their -1)
        // scan 2: among the candidates at that maximum, the largest (Gamma(s), index key); y = index key << 32 | candidate, never 0
        unsigned long long bx = 0, by = 0;
        for (uint32_t cnd = static_cast<uint32_t>(tid); cnd < a.n_cand; cnd += kLooThreads) {
            const TpRec rec = cand[cnd];
            if (((used[rec.i >> 5] >> (rec.i & 31)) | (used[rec.j >> 5] >> (rec.j & 31))) & 1u) continue;
            const uint2 w = wb[cnd];
            if (tp_abs(loo_num(rec, side, (w.x >> t) & 1u, (w.y >> t) & 1u, a.s_a, a.s_b)) + 1ull != best) continue;
            const int64_t di = loo_shift(sums[rec.i], sums[a.Gp + rec.i], side, loo_edge_sum(AL, AH, a.Gp, b, rec.i, t), a.s_a, a.s_b);
            const int64_t dj = loo_shift(sums[rec.j], sums[a.Gp + rec.j], side, loo_edge_sum(AL, AH, a.Gp, b, rec.j, t), a.s_a, a.s_b);
            const unsigned long long x = tp_gamma(di, dj);
            const unsigned long long y = (static_cast<unsigned long long>(loo_index_key(rec.i, rec.j, a.G)) << 32) | cnd;
            if (by == 0 || x > bx || (x == bx && y > by)) { bx = x; by = y; }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const unsigned long long ox = loo_shfl_xor(bx, m), oy = loo_shfl_xor(by, m);
            if (oy != 0 && (by == 0 || ox > bx || (ox == bx && oy > by))) { bx = ox; by = oy; }
        }
        if (lane == 0) { red_x[wave] = bx; red_y[wave] = by; }
        __syncthreads();
        bx = red_x[0]; by = red_y[0];
#pragma unroll
        for (int w = 1; w < kLooWaves; ++w) {
            const unsigned long long ox = red_x[w], oy = red_y[w];
            if (oy != 0 && (by == 0 || ox > bx || (ox == bx && oy > by))) { bx = ox; by = oy; }
        }
        __syncthreads();                 // (every thread has read the partial results and the bitmap of this round)
        if (by == 0) break;              // (cannot be: scan 1 found a candidate; workgroup-uniform)
        if (tid == 0) {
            const uint32_t cnd = static_cast<uint32_t>(by & 0xFFFFFFFFull);
            const TpRec rec = cand[cnd];
            const uint2 w = wb[cnd];
            const uint32_t gt_bit = (w.x >> t) & 1u, eq_bit = (w.y >> t) & 1u;
            const size_t o = static_cast<size_t>(col) * a.kmax + r;
            out_i[o] = rec.i; out_j[o] = rec.j;
            out_n[o] = loo_num(rec, side, gt_bit, eq_bit, a.s_a, a.s_b);
            out_g[o] = static_cast<int64_t>(bx);
            out_o[o] = static_cast<int8_t>(loo_outcome(gt_bit, eq_bit));
            used[rec.i >> 5] |= 1u << (rec.i & 31);
            used[rec.j >> 5] |= 1u << (rec.j & 31);
        }
        __syncthreads();
    }
}

}  // namespace

int32_t launch_loo_words(reo_ctx *c, const TpRec *d_cand, int64_t n_cand, uint2 *d_words)
{
    int32_t rc = need_planes(c, "reo_top_pairs_loo", kTpMaxGenes);
    if (rc) return rc;
    const int nblk = c->goff32.back() / 32;
    if (n_cand < 1 || n_cand > kLooMaxRecords || nblk < 1 || nblk > 65535 || !d_cand || !d_words) {
        set_error("reo_top_pairs_loo: the words of %lld candidates over %d sample blocks cannot be made", (long long)n_cand, nblk);
        return REO_EINVAL;
    }
    const dim3 g(static_cast<unsigned>((n_cand + kLooThreads - 1) / kLooThreads), static_cast<unsigned>(nblk));
    const uint32_t n = static_cast<uint32_t>(n_cand);
    with_plane_bits(c->G, [&](auto nb) {
        k_loo_words<decltype(nb)::value><<<g, kLooThreads, 0, c->stream>>>(d_cand, c->pos.p, c->lo.p, c->hi.p, d_words, c->Gp, n);
    });
    REO_HIP_CHECK(hipGetLastError());
    return REO_OK;
}

int32_t launch_loo_select(reo_ctx *c, const TpRec *d_cand, int64_t n_cand, const uint2 *d_words, const int32_t *d_gside, const int32_t *d_slot2col,
                          const int64_t *d_sums, int s_a, int s_b, int kmax, int32_t *d_i, int32_t *d_j, int64_t *d_n, int64_t *d_g, int8_t *d_o)
{
    int32_t rc = need_planes(c, "reo_top_pairs_loo", kTpMaxGenes);
    if (rc) return rc;
    const int slots = c->goff32.back();
    if (n_cand < 1 || n_cand > kLooMaxRecords || slots < 32 || kmax < 1 || kmax > kLooMaxK || !d_cand || !d_words || !d_gside || !d_slot2col || !d_sums) {
        set_error("reo_top_pairs_loo: %d folds over %lld candidates with kmax = %d cannot be launched", slots, (long long)n_cand, kmax);
        return REO_EINVAL;
    }
    LooArgs a;
    a.G = static_cast<int>(c->G); a.Gp = c->Gp; a.ngroups = c->ngroups; a.kmax = kmax;
    a.n_cand = static_cast<uint32_t>(n_cand); a.s_a = s_a; a.s_b = s_b; a.S = c->S;
    k_loo_select<<<static_cast<unsigned>(slots), kLooThreads, 0, c->stream>>>(d_cand, d_words, c->lo.p, c->hi.p, c->goff_dev.p, d_gside, d_slot2col, d_sums,
                                                                              d_i, d_j, d_n, d_g, d_o, a);
    REO_HIP_CHECK(hipGetLastError());
    return REO_OK;
}

}  // namespace reo
