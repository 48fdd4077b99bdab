// reo_pair_list: the partner genes behind a gene's contingency tallies, read from the 4-bit class table that reo_build_pairs leaves in HBM
// ([G][4 planes][Wp], bit j of row i = the ordered pair (i, j) seen from gene i) and delivered as a CSR.  Two kernels in K2's shape (one
// wave per query row, four rows per workgroup of 256 threads, 16-byte loads of the four planes and of the partner mask as bits):
//   k_pair_count  selected-pair word (pair_list.h) -> popcount -> wave sum -> one int32 per query; the host makes the 64-bit prefix sums;
//   k_pair_fill   the same pass; per loop step a wave-wide exclusive scan of the lanes' popcounts on top of a wave-uniform running base gives
//                 every lane the place of its first entry, and it expands its set bits to (partner, code) from there.  Columns grow with the
//                 lane and with the loop step, so a row's partners come out ascending.
// The fill stores are a lane's own run of consecutive entries (4 + 1 bytes each): neighbouring lanes write neighbouring runs, not neighbouring
// addresses.  Staging a row through LDS would coalesce them; whether that pays is for tools/pair_list_ab.py to show, it
// is not assumed here.  No store goes past the row's own end or past `capacity`: a row whose fill disagrees with its count raises a flag
// (REO_EHIP) instead of writing.
#include "pair_list.h"
#include "reo_internal.h"

namespace reo {

namespace {

constexpr int kPlThreads = 256;
constexpr int kPlRows = kPlThreads / 64;   // query rows per workgroup

struct PairWords { uint32_t cl[4], ch[4], tl[4], th[4], sel[4]; };

// uint4 q of row `row` (table columns 128 q .. 128 q + 127): the four planes and the selected-pair words under the partner mask
__device__ __forceinline__ void pair_words(const uint4 *__restrict__ r, const uint4 *__restrict__ maskbits, int row, int q, int G, int Wq,
                                           uint32_t class_mask, PairWords &p)
{
    const uint4 m = maskbits[q];
    const uint4 cl = r[q], ch = r[Wq + q], tl = r[2 * Wq + q], th = r[3 * Wq + q];
    p.cl[0] = cl.x; p.cl[1] = cl.y; p.cl[2] = cl.z; p.cl[3] = cl.w;
    p.ch[0] = ch.x; p.ch[1] = ch.y; p.ch[2] = ch.z; p.ch[3] = ch.w;
    p.tl[0] = tl.x; p.tl[1] = tl.y; p.tl[2] = tl.z; p.tl[3] = tl.w;
    p.th[0] = th.x; p.th[1] = th.y; p.th[2] = th.z; p.th[3] = th.w;
    const uint32_t mk[4] = {m.x, m.y, m.z, m.w};
#pragma unroll
    for (int k = 0; k < 4; ++k)
        p.sel[k] = pair_select_word(p.cl[k], p.ch[k], p.tl[k], p.th[k], pair_valid_word(row, 4 * q + k, G) & mk[k], class_mask);
}

__global__ __launch_bounds__(kPlThreads) void k_pair_count(const uint32_t *__restrict__ table, const uint4 *__restrict__ maskbits,
                                                           const int32_t *__restrict__ genes, int n_genes, int G, int Wq, uint32_t class_mask,
                                                           int32_t *__restrict__ count)
{
    const int lane = threadIdx.x & 63;
    const int query = blockIdx.x * kPlRows + (threadIdx.x >> 6);   // (wave-uniform)
    if (query >= n_genes) return;
    const int row = genes[query];
    const uint4 *r = reinterpret_cast<const uint4 *>(table) + static_cast<size_t>(row) * kPlanes * Wq;
    uint32_t n = 0;
    for (int q = lane; q < Wq; q += 64) {
        PairWords p;
        pair_words(r, maskbits, row, q, G, Wq, class_mask, p);
        n += __popc(p.sel[0]) + __popc(p.sel[1]) + __popc(p.sel[2]) + __popc(p.sel[3]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if (lane == 0) count[query] = static_cast<int32_t>(n);
}

__global__ __launch_bounds__(kPlThreads) void k_pair_fill(const uint32_t *__restrict__ table, const uint4 *__restrict__ maskbits,
                                                          const int32_t *__restrict__ genes, int n_genes, int G, int Wq, uint32_t class_mask,
                                                          const int64_t *__restrict__ rowptr, int32_t *__restrict__ partner,
                                                          uint8_t *__restrict__ code, int64_t capacity, int32_t *__restrict__ flag)
{
    const int lane = threadIdx.x & 63;
    const int query = blockIdx.x * kPlRows + (threadIdx.x >> 6);   // (wave-uniform: every shuffle below has its 64 lanes)
    if (query >= n_genes) return;
    const int row = genes[query];
    const uint4 *r = reinterpret_cast<const uint4 *>(table) + static_cast<size_t>(row) * kPlanes * Wq;
    const int64_t begin = rowptr[query];
    const int64_t rowend = rowptr[query + 1];
    const int64_t end = rowend < capacity ? rowend : capacity;   // no store at or past this entry
    int64_t base = begin;   // wave-uniform: the first entry of this loop step
    bool bad = false;
    for (int q0 = 0; q0 < Wq; q0 += 64) {
        const int q = q0 + lane;
        PairWords p = {};
        if (q < Wq) pair_words(r, maskbits, row, q, G, Wq, class_mask, p);
        const int cnt = __popc(p.sel[0]) + __popc(p.sel[1]) + __popc(p.sel[2]) + __popc(p.sel[3]);
        int incl = cnt;   // inclusive scan over the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        int64_t at = base + (incl - cnt);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            uint32_t w = p.sel[k];
            while (w) {
                const int b = __ffs(static_cast<int>(w)) - 1;
                w &= w - 1;
                if (at >= begin && at < end) {
                    partner[at] = (4 * q + k) * 32 + b;
                    code[at] = static_cast<uint8_t>(pair_code_at(p.cl[k], p.ch[k], p.tl[k], p.th[k], b));
                } else {
                    bad = true;
                }
                ++at;
            }
        }
        base += __shfl(incl, 63, 64);
    }
    if (base != rowend) bad = true;   // the count pass saw another number of pairs
    if (__ballot(bad) && lane == 0) atomicOr(flag, 1);
}

int32_t check_launch(const reo_ctx *c, int64_t n_genes)
{
    if (c->Wp <= 0 || (c->Wp & 3) || !c->table.p) { set_error("reo_pair_list: no class table"); return REO_EINVAL; }
    if (n_genes < 1 || n_genes > (int64_t(1) << 30)) { set_error("reo_pair_list: %lld query genes (at most 2^30 per call)", (long long)n_genes); return REO_EINVAL; }
    return REO_OK;
}

}  // namespace

int32_t launch_pair_count(reo_ctx *c, const int32_t *d_genes, int64_t n_genes, const uint32_t *d_maskbits, uint32_t class_mask, int32_t *d_count)
{
    const int32_t rc = check_launch(c, n_genes);
    if (rc) return rc;
    const unsigned grid = static_cast<unsigned>((n_genes + kPlRows - 1) / kPlRows);
    k_pair_count<<<grid, kPlThreads, 0, c->stream>>>(c->table.p, reinterpret_cast<const uint4 *>(d_maskbits), d_genes, static_cast<int>(n_genes),
                                                     static_cast<int>(c->G), c->Wp / 4, class_mask, d_count);
    REO_HIP_CHECK(hipGetLastError());
    return REO_OK;
}

int32_t launch_pair_fill(reo_ctx *c, const int32_t *d_genes, int64_t n_genes, const uint32_t *d_maskbits, uint32_t class_mask, const int64_t *d_rowptr,
                         int32_t *d_partner, uint8_t *d_code, int64_t capacity, int32_t *d_flag)
{
    const int32_t rc = check_launch(c, n_genes);
    if (rc) return rc;
    const unsigned grid = static_cast<unsigned>((n_genes + kPlRows - 1) / kPlRows);
    k_pair_fill<<<grid, kPlThreads, 0, c->stream>>>(c->table.p, reinterpret_cast<const uint4 *>(d_maskbits), d_genes, static_cast<int>(n_genes),
                                                    static_cast<int>(c->G), c->Wp / 4, class_mask, d_rowptr, d_partner, d_code, capacity, d_flag);
    REO_HIP_CHECK(hipGetLastError());
    return REO_OK;
}

}  // namespace reo
