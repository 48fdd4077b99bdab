// reo_sample_counts: in which samples the selected pairs of a query gene put it above (or level with) its partner.  The same
// O(pairs x samples) comparison as the pair kernel's, summed over PARTNERS per sample instead of over samples per pair.
//   k_sample_counts<BIG, WITH_EQ>   one workgroup of four waves per (query, chunk of kScChunkBlocks sample blocks).
//     per tile of kScTileCols table columns:
//       select   threads 0 .. 127 form the selected-pair word of one table word each (pair_list.h, the mask as bits), a scan over the two
//                waves gives every word its place, and the set bits become a list of 16-bit column offsets in LDS;
//       chain    wave w takes blocks w, w + 4, ... of the chunk, its lanes the listed partners: the band edges lo_i / hi_i of the block are
//                wave-uniform, a lane loads its partner's pos planes and runs the borrow chain of band_chain.h over plane_bits(G)
//                planes; the 32-sample words lt (and le) are added into lane-local vertical counters (sample_counts.h), as many planes
//                as the lane's share of the tile needs;
//       reduce   per plane k and sample bit s: popcount(ballot(bit)) << k, summed over k, kept by lane s and added to the block's 32 int32
//                accumulators in LDS (a block belongs to one wave: no atomics).
//     at the end the accumulators of the REAL sample slots go to row `query` of the [batch][S] outputs in the caller's column order
//     (slot2col); padding slots are never written.  n_eq = le - lt.  WITH_EQ = false: no le chain, no counters for it.
// Integer arithmetic only; every sum is over a fixed assignment of partners to lanes: deterministic.  Addresses: the query row is checked
// by the host (sample_counts_check_args), listed columns are < G by pair_valid_word, words are < Wp, blocks < the transform's block count;
// stores go to columns slot2col[slot] in [0, S) of the workgroup's own query row.
#include "sample_counts.h"
#include "reo_internal.h"
#include "band_chain.h"

namespace reo {

namespace {

constexpr int kScThreads = 256;
constexpr int kScWaves = kScThreads / kScLanes;
static_assert(kScTileWords <= kScThreads && kScTileWords == 2 * kScLanes, "two waves select a tile, one table word per thread");
static_assert(kScChunkBlocks * 32 == kScThreads, "one thread per sample slot of the chunk at write-out");
static_assert(kScTileCols / kScLanes < (1 << kScMaxPlanes), "the counters hold a lane's share of a tile");

struct ScArgs {
    const uint32_t *table, *maskbits;
    const int32_t *genes, *slot2col;
    const uint4 *P, *AL, *AH;
    int32_t *sel, *gt, *eq;
    int n_queries, G, Gp, Wp, S, nbits, nblk, nchunks;
    uint32_t class_mask;
};

// the lanes' vertical counters -> the wave's count of sample bit `lane` (lanes 32 .. 63: of bit lane - 32, unused)
__device__ __forceinline__ uint32_t wave_counts(const uint32_t (&c)[kScMaxPlanes], int planes, int lane)
{
    uint32_t mine = 0;
#pragma clang loop unroll(disable)
    for (int s = 0; s < 32; ++s) {
        uint32_t t = 0;
#pragma unroll
        for (int k = 0; k < kScMaxPlanes; ++k) {
            if (k >= planes) break;
            t += static_cast<uint32_t>(__popcll(__ballot((c[k] >> s) & 1u))) << k;
        }
        if ((lane & 31) == s) mine = t;
    }
    return mine;
}

template <bool BIG, bool WITH_EQ>
__global__ __launch_bounds__(kScThreads) void k_sample_counts(ScArgs a)
{
    constexpr int NW = BandLayout<BIG>::NW;   // plane words per gene and block
    __shared__ uint16_t list[kScTileCols];
    __shared__ int32_t acc_lt[kScThreads], acc_le[WITH_EQ ? kScThreads : 1];
    __shared__ int32_t wave_tot[2];
    const int tid = threadIdx.x, lane = tid & (kScLanes - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int query = static_cast<int>(blockIdx.x / static_cast<unsigned>(a.nchunks));
    const int chunk = static_cast<int>(blockIdx.x) - query * a.nchunks;
    if (query >= a.n_queries) return;   // (workgroup-uniform; the grid is exact)
    const int row = a.genes[query];
    const int b0 = chunk * kScChunkBlocks;
    const uint32_t *r = a.table + static_cast<size_t>(row) * kPlanes * a.Wp;
    acc_lt[tid] = 0;
    if constexpr (WITH_EQ) acc_le[tid] = 0;
    int n_sel = 0;
    for (int t0 = 0; t0 < a.G; t0 += kScTileCols) {
        // ---- select: the partners of this tile
        const int w = (t0 >> 5) + tid;
        uint32_t sel = 0;
        if (tid < kScTileWords && w < a.Wp)
            sel = pair_select_word(r[w], r[a.Wp + w], r[2 * a.Wp + w], r[3 * a.Wp + w], pair_valid_word(row, w, a.G) & a.maskbits[w], a.class_mask);
        const int cnt = __popc(sel);
        int incl = cnt;
#pragma unroll
        for (int o = 1; o < kScLanes; o <<= 1) {
            const int up = __shfl_up(incl, o, kScLanes);
            if (lane >= o) incl += up;
        }
        if (wave < 2 && lane == kScLanes - 1) wave_tot[wave] = incl;
        __syncthreads();   // (also: every wave has left the chain of the tile before, the list may be rewritten)
        const int n_tile = wave_tot[0] + wave_tot[1];
        int at = incl - cnt + (wave == 1 ? wave_tot[0] : 0);
        while (sel) {
            const int b = __ffs(static_cast<int>(sel)) - 1;
            sel &= sel - 1;
            list[at++] = static_cast<uint16_t>(tid * 32 + b);   // at < n_tile <= kScTileCols
        }
        __syncthreads();
        n_sel += n_tile;
        if (n_tile == 0) continue;   // (uniform)
        // ---- chain and reduce: this wave's blocks against the listed partners
        const int planes = sc_counter_planes((n_tile + kScLanes - 1) / kScLanes);   // a lane takes entries lane, lane + 64, ...
        for (int rb = wave; rb < kScChunkBlocks; rb += kScWaves) {
            const int b = b0 + rb;
            if (b >= a.nblk) break;
            uint32_t lo[NW], hi[NW];   // (hi, cle: unused and gone without WITH_EQ)
            band_load_edges<BIG, WITH_EQ>(a.AL, a.AH, band_edge_row<BIG>(a.Gp, b, row), lo, hi);
            uint32_t clt[kScMaxPlanes] = {0, 0, 0, 0, 0, 0, 0}, cle[kScMaxPlanes] = {0, 0, 0, 0, 0, 0, 0};
            const uint4 *pb = a.P + static_cast<size_t>(b) * BandLayout<BIG>::NQ * a.Gp;
            for (int e = lane; e < n_tile; e += kScLanes) {
                const int j = t0 + list[e];
                uint32_t p[NW];
#pragma unroll
                for (int q = 0; q < BandLayout<BIG>::NQ; ++q) band_unpack(pb[static_cast<size_t>(q) * a.Gp + j], p, q);
                uint32_t lt = 0, le = 0;
#pragma unroll
                for (int k = 0; k < NW; ++k) {
                    if (k >= a.nbits) break;
                    const int ew = BandLayout<BIG>::edge_word(k);
                    lt = band_borrow(p[k], lo[ew], lt);
                    if constexpr (WITH_EQ) le = band_borrow(p[k], hi[ew], le);
                }
#pragma unroll
                for (int k = 0; k < kScMaxPlanes; ++k) {   // sc_counter_add, unrolled over registers
                    if (k >= planes) break;
                    const uint32_t carry = clt[k] & lt;
                    clt[k] ^= lt;
                    lt = carry;
                    if constexpr (WITH_EQ) {
                        const uint32_t ce = cle[k] & le;
                        cle[k] ^= le;
                        le = ce;
                    }
                }
            }
            const uint32_t n_lt = wave_counts(clt, planes, lane);
            if (lane < 32) acc_lt[rb * 32 + lane] += static_cast<int32_t>(n_lt);
            if constexpr (WITH_EQ) {
                const uint32_t n_le = wave_counts(cle, planes, lane);
                if (lane < 32) acc_le[rb * 32 + lane] += static_cast<int32_t>(n_le);
            }
        }
    }
    __syncthreads();
    if (chunk == 0 && tid == 0) a.sel[query] = n_sel;
    const int slot = b0 * 32 + tid;
    if (slot < a.nblk * 32) {
        const int col = a.slot2col[slot];
        if (col >= 0 && col < a.S) {
            const size_t o = static_cast<size_t>(query) * a.S + col;
            a.gt[o] = acc_lt[tid];
            if constexpr (WITH_EQ) a.eq[o] = acc_le[tid] - acc_lt[tid];
        }
    }
}

}  // namespace

int32_t launch_sample_counts(reo_ctx *c, const int32_t *d_genes, int64_t n_queries, const uint32_t *d_maskbits, uint32_t class_mask,
                             const int32_t *d_slot2col, int32_t *d_sel, int32_t *d_gt, int32_t *d_eq)
{
    if (c->Wp <= 0 || !c->table.p || !c->pos.p || !c->lo.p || !c->hi.p || c->goff32.empty()) {
        set_error("reo_sample_counts: no class table or no bit planes");
        return REO_EINVAL;
    }
    if (const int32_t rp = ensure_planes(c)) return rp;
    ScArgs a;
    a.table = c->table.p; a.maskbits = d_maskbits; a.genes = d_genes; a.slot2col = d_slot2col;
    a.P = c->pos.p; a.AL = c->lo.p; a.AH = c->hi.p;
    a.sel = d_sel; a.gt = d_gt; a.eq = d_eq;
    a.G = static_cast<int>(c->G); a.Gp = c->Gp; a.Wp = c->Wp; a.S = static_cast<int>(c->S); a.nbits = plane_bits(c->G);
    a.nblk = c->goff32.back() / 32;
    a.nchunks = (a.nblk + kScChunkBlocks - 1) / kScChunkBlocks;
    a.class_mask = class_mask;
    const int64_t grid = n_queries * a.nchunks;
    if (n_queries < 1 || a.nblk < 1 || grid > 0x7FFFFFFF) {
        set_error("reo_sample_counts: a batch of %lld queries x %d chunks of sample blocks cannot be launched", (long long)n_queries, a.nchunks);
        return REO_EINVAL;
    }
    a.n_queries = static_cast<int>(n_queries);
    const bool big = c->G > 65535;
    const dim3 g(static_cast<unsigned>(grid));
    if (big) {
        if (d_eq) k_sample_counts<true, true><<<g, kScThreads, 0, c->stream>>>(a);
        else k_sample_counts<true, false><<<g, kScThreads, 0, c->stream>>>(a);
    } else {
        if (d_eq) k_sample_counts<false, true><<<g, kScThreads, 0, c->stream>>>(a);
        else k_sample_counts<false, false><<<g, kScThreads, 0, c->stream>>>(a);
    }
    REO_HIP_CHECK(hipGetLastError());
    return REO_OK;
}

}  // namespace reo
