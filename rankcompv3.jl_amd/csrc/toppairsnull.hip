// reo_top_pairs_null: per label permutation the largest |N| over all gene pairs, the pair that attains it and how many pairs reach a few
// cuts, for a batch of permutations from ONE walk over the bit planes (semantics, the key, the word packing and the host checks:
// top_pairs_null.h; entry point: queries.hip).
//   k_top_null_words   the label bytes [n_perm][S] (caller's column order) into one A-word per (permutation, block of 32 sample slots),
//     laid out [launch group][block][kPermQ] as k_perm_words lays them out (pn_word_index), and one live word per block (tn_live_word of
//     row 0: the slot has a column on one of the two sides; every row has its 2-bytes in the same columns).  A is a subset of live.
//   k_top_pairs_null<TIES, NB>   (NB = plane_bits(G) planes: a constant trip count of the chain)  the hot path, in the geometry of
//     k_pairs_permuted restricted by the tile rule of k_top_pairs: a wave owns 64 columns (lane = gene j) and kTnRows rows, four waves per
//     workgroup take four neighbouring column tiles of the same rows, blockIdx.z is the launch group of kPermQ permutations; only tiles
//     that touch i < j are walked (tp_tile_live, tp_group_live) and the lanes with j <= i are dead.  The wave walks the sample blocks with
//     a live slot: a lane loads the 16 pos planes of its column once per block and keeps them for all rows; the band edges of a row, the
//     live word and the kPermQ A-words of the block are wave-uniform (__restrict__ arguments, wave-uniform addresses: scalar loads).  Per
//     (row, block) there is one borrow chain (two with ties), then gt_all += popc(lt & live), gtA[q] += popc(lt & A[q]) and, with ties,
//     the eq counterparts from le & ~lt.  Side B is all - A.  The tie-free form (the transform reported no ties) carries no le chain and
//     no eq counters.  At the end, per permutation: |N| of every row through tp_num, the lane's best key over its rows (tn_key), a wave
//     maximum by shuffles, one LDS atomicMax per wave, and ONE 64-bit global atomicMax per workgroup; per cut a ballot + popcount per
//     row into a 32-bit LDS counter, flushed once per workgroup with a 64-bit global atomicAdd.
// Integer atomics only (max and add commute: the results do not depend on their arrival order); no kernel keeps state between launches;
// there is no grid-wide synchronisation and no spinning; both barriers sit behind conditions on blockIdx and the arguments alone.
// Addresses: rows end at the next multiple of kTnRows and columns at the next multiple of 64, both below Gp (a multiple of 1024); the
// mask words are sized for Gp genes; blocks run over [0, nblk), the number of blocks the transform sliced and the A / live words were
// sized for; a launch group z < ceil(np / kPermQ) reads the words of its own group, which pn_word_count allocates whole (rows past np are
// zero, and nothing of them is stored); keys[z kPermQ + q] and reach[(z kPermQ + q) kTnMaxCuts + t] are written only for z kPermQ + q <
// np <= kTnBatchCap, t < n_cuts <= kTnMaxCuts, and both arrays hold kTnBatchCap permutations.  Counts are at most S <= 65535; a workgroup
// counts at most 4 * 64 * kTnRows pairs per cut.
#include "top_pairs_null.h"
#include "reo_internal.h"
#include "band_chain.h"

namespace reo {

namespace {

constexpr int kTnThreads = 256;
static_assert(kTnThreads == kTpWaves * 64, "one wave per column tile of the workgroup (tp_group_live)");
static_assert(kGenePad % kTnRows == 0 && kGenePad % 64 == 0, "row and column tiles end inside the padded gene count");

__global__ __launch_bounds__(256) void k_top_null_words(const uint8_t *__restrict__ side, const int32_t *__restrict__ slot2col, int64_t S, int64_t n_perm,
                                                        int nblk, uint32_t *__restrict__ aw, uint32_t *__restrict__ live)
{
    const int64_t p = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    const int b = static_cast<int>(blockIdx.y);
    if (p >= n_perm || b >= nblk) return;
    const int32_t *map = slot2col + static_cast<size_t>(b) * 32;
    aw[pn_word_index(p, b, nblk)] = pn_side_word(side + p * S, S, map);
    if (p == 0) live[b] = tn_live_word(side, S, map);
}

struct TnArgs {
    int G, Gp, nblk;
    int s_a, s_b;   // the sides' sizes: kept under every permutation
    int np;         // permutations of this launch
    int n_cuts;
    uint32_t cuts[kTnMaxCuts];   // |N| < 2^31: a cut of 2^31 or more is 0xFFFFFFFF, which no pair reaches
};

template <bool TIES, int NB>   // NB = plane_bits(G): 12, 15 or 16 planes
__global__ __launch_bounds__(kTnThreads) void k_top_pairs_null(const uint4 *__restrict__ P, const uint4 *__restrict__ AL, const uint4 *__restrict__ AH,
                                                               const uint32_t *__restrict__ AW, const uint32_t *__restrict__ LW,
                                                               const uint32_t *__restrict__ maskbits, unsigned long long *__restrict__ keys,
                                                               unsigned long long *__restrict__ reach, TnArgs a)
{
    __shared__ unsigned long long best[kPermQ];
    __shared__ uint32_t hits[kPermQ * kTnMaxCuts];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
    const int ctile = static_cast<int>(blockIdx.x) * kTpWaves + wave;
    const int i0 = static_cast<int>(blockIdx.y) * kTnRows;
    const int z = static_cast<int>(blockIdx.z);
    if (!tp_group_live(static_cast<int>(blockIdx.x), i0) || z * kPermQ >= a.np) return;   // (workgroup-uniform, in front of every barrier)
    if (threadIdx.x < kPermQ) best[threadIdx.x] = 0;
    if (threadIdx.x < kPermQ * kTnMaxCuts) hits[threadIdx.x] = 0;
    __syncthreads();
    if (tp_tile_live(ctile, i0, a.G)) {   // (wave-uniform)
        const int j = ctile * 64 + lane;   // < Gp
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
                const size_t row = (static_cast<size_t>(b) * a.Gp + (i0 + r)) * 4;   // (i0 + r < Gp)
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
        const bool col_ok = tp_mask_bit(maskbits, j);
        bool live_pair[kTnRows];
#pragma unroll
        for (int r = 0; r < kTnRows; ++r) {
            const int i = i0 + r;
            live_pair[r] = i < a.G && tp_lane_live(i, j, a.G) && col_ok && tp_mask_bit(maskbits, i);
        }
#pragma unroll
        for (int q = 0; q < kPermQ; ++q) {
            if (z * kPermQ + q >= a.np) continue;   // (wave-uniform; a guard, not a break: the counters stay fixed registers)
            unsigned long long key = 0;
            uint32_t n[kTnRows];   // |N| < 2^31
#pragma unroll
            for (int r = 0; r < kTnRows; ++r) {
                uint32_t gA = gtA[r][q], eA = TIES ? eqA[r][TIES ? q : 0] : 0u;
                // a COPY of the counters goes into tp_num's 64-bit arithmetic: widened where they stand, every counter is the low half of a
                // register pair through the whole count loop (with ties 256 VGPRs + 27 AGPRs and an occupancy of 1 instead of 161 and 3;
                // one statement for both: with two the pairs come back -- profiles/top_pairs_null_kernel_registers.txt)
                if (TIES) asm volatile("" : "+v"(gA), "+v"(eA));
                else asm volatile("" : "+v"(gA));
                const uint32_t gB = gtAll[r] - gA, eB = eqAll[r] - eA;
                n[r] = static_cast<uint32_t>(tp_abs(tp_num(static_cast<int32_t>(gA), static_cast<int32_t>(eA), static_cast<int32_t>(gB), static_cast<int32_t>(eB), a.s_a, a.s_b)));
                if (live_pair[r]) {
                    const unsigned long long k = tn_key(n[r], i0 + r, j, a.G);
                    key = k > key ? k : key;
                }
            }
            for (int t = 0; t < a.n_cuts; ++t) {   // (wave-uniform trip count)
                uint32_t cnt = 0;
#pragma unroll
                for (int r = 0; r < kTnRows; ++r) cnt += static_cast<uint32_t>(__builtin_popcountll(__ballot(live_pair[r] && n[r] >= a.cuts[t])));
                if (cnt != 0 && lane == 0) atomicAdd(&hits[q * kTnMaxCuts + t], cnt);
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                const unsigned long long o = __shfl_xor(key, d);
                key = o > key ? o : key;
            }
            if (lane == 0 && key != 0) atomicMax(&best[q], key);
        }
    }
    __syncthreads();
    const int t = static_cast<int>(threadIdx.x);
    if (t < kPermQ && z * kPermQ + t < a.np && best[t] != 0) atomicMax(&keys[z * kPermQ + t], best[t]);
    if (t < kPermQ * kTnMaxCuts) {
        const int q = t / kTnMaxCuts, cut = t % kTnMaxCuts;
        const uint32_t v = hits[t];
        if (v != 0 && cut < a.n_cuts && z * kPermQ + q < a.np)
            atomicAdd(&reach[static_cast<size_t>(z * kPermQ + q) * kTnMaxCuts + cut], static_cast<unsigned long long>(v));
    }
}

template <bool TIES>
void tn_launch(reo_ctx *c, const dim3 &g, const uint32_t *d_aw, const uint32_t *d_live, const uint32_t *d_maskbits, unsigned long long *d_keys,
               unsigned long long *d_reach, const TnArgs &a)
{
    with_plane_bits(c->G, [&](auto nb) {
        k_top_pairs_null<TIES, decltype(nb)::value><<<g, kTnThreads, 0, c->stream>>>(c->pos.p, c->lo.p, c->hi.p, d_aw, d_live, d_maskbits, d_keys, d_reach, a);
    });
}

}  // namespace

int32_t launch_top_null_words(reo_ctx *c, const uint8_t *d_side, int64_t n_perm, const int32_t *d_slot2col, uint32_t *d_aw, uint32_t *d_live)
{
    if (!d_side || !d_slot2col || !d_aw || !d_live || n_perm < 1 || n_perm > kTnBatchCap || c->goff32.empty()) {
        set_error("reo_top_pairs_null: no label rows on the device");
        return REO_EINVAL;
    }
    const int nblk = c->goff32.back() / 32;
    if (nblk < 1 || nblk > 65535) { set_error("reo_top_pairs_null: %d sample blocks cannot be launched", nblk); return REO_EINVAL; }
    REO_HIP_CHECK(hipMemsetAsync(d_aw, 0, pn_word_count(n_perm, nblk) * sizeof(uint32_t), c->stream));
    k_top_null_words<<<dim3(static_cast<unsigned>((n_perm + 255) / 256), static_cast<unsigned>(nblk)), 256, 0, c->stream>>>(d_side, d_slot2col, c->S, n_perm,
                                                                                                                           nblk, d_aw, d_live);
    REO_HIP_CHECK(hipGetLastError());
    return REO_OK;
}

int32_t launch_top_pairs_null(reo_ctx *c, const uint32_t *d_aw, const uint32_t *d_live, int np, int s_a, int s_b, const uint32_t *d_maskbits,
                              const int64_t *cuts, int n_cuts, unsigned long long *d_keys, unsigned long long *d_reach)
{
    int32_t rc = need_planes(c, "reo_top_pairs_null", kTpMaxGenes);
    if (rc) return rc;
    if (!d_aw || !d_live || !d_keys || !d_reach || np < 1 || np > kTnBatchCap || n_cuts < 0 || n_cuts > kTnMaxCuts || (n_cuts > 0 && !cuts)) {
        set_error("reo_top_pairs_null: bad batch");
        return REO_EINVAL;
    }
    TnArgs a;
    a.G = static_cast<int>(c->G); a.Gp = c->Gp; a.nblk = c->goff32.back() / 32;
    a.s_a = s_a; a.s_b = s_b; a.np = np; a.n_cuts = n_cuts;
    for (int t = 0; t < kTnMaxCuts; ++t) a.cuts[t] = (t < n_cuts && cuts[t] < (int64_t(1) << 31)) ? static_cast<uint32_t>(cuts[t]) : 0xFFFFFFFFu;
    const dim3 grid = tile_grid(c->G, c->G, kTnRows, kTpWaves, (np + kPermQ - 1) / kPermQ);
    if (c->has_ties) tn_launch<true>(c, grid, d_aw, d_live, d_maskbits, d_keys, d_reach, a);
    else tn_launch<false>(c, grid, d_aw, d_live, d_maskbits, d_keys, d_reach, a);
    REO_HIP_CHECK(hipGetLastError());
    return REO_OK;
}

}  // namespace reo
