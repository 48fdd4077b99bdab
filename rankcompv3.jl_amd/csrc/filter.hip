// reo_filter_matrix: the reference's two low-expression filters on the RESIDENT matrix -- src/RankCompV3.jl:618 (a profile stays iff
// more than min_profiles of its genes are > 0) then :626 (a gene stays iff more than min_features of the KEPT profiles have it > 0) --
// and the compaction of what stays.  Three HBM streams over the matrix (two that count, one that gathers), the G + S counts go to the
// host once in between (the caller wants the masks anyway; csrc/filter_maps.h turns them into the source lists of the gather).
// Not measured, not tuned beyond coalescing: 256 threads are gx lanes along g (consecutive addresses) by 256 / gx rows along s, gx the
// power of two that covers min(G, 256), so that a matrix of two genes by a million profiles reads whole cache lines too.
#include <algorithm>
#include <utility>

#include "filter_maps.h"
#include "reo_internal.h"

namespace reo {

namespace {

constexpr int kFThreads = 256;
constexpr int kFGenesPer = 8;   // f_count_cols: genes per lane and block (a column of 262 143 genes is 128 blocks)
constexpr int kFColsPer = 16;   // f_count_genes: columns per lane and block

int lanes_log2(int64_t G)
{
    int l = 1;
    while (l < 8 && (int64_t(1) << l) < G) ++l;
    return l;
}

// positives per column.  Block b: columns (b / gsplit) * sy .. + sy (one per row of lanes), genes part * gchunk .. + gchunk.
template <class W>
__global__ __launch_bounds__(kFThreads) void f_count_cols(const W *__restrict__ X, int64_t ld, int G, int S, int gxl, int gsplit, W limit,
                                                         int32_t *__restrict__ colcnt)
{
    __shared__ int32_t sh[kFThreads / 2];
    const int gx = 1 << gxl, sy = kFThreads >> gxl;
    const int lane = threadIdx.x & (gx - 1), row = threadIdx.x >> gxl;
    const int part = blockIdx.x % gsplit;
    const int64_t s = static_cast<int64_t>(blockIdx.x / gsplit) * sy + row;
    if (static_cast<int>(threadIdx.x) < sy) sh[threadIdx.x] = 0;
    __syncthreads();
    int cnt = 0;
    if (s < S) {
        const int gchunk = gx * kFGenesPer;
        const int g0 = part * gchunk, g1 = min(G, g0 + gchunk);
        const W *col = X + s * ld;
        for (int g = g0 + lane; g < g1; g += gx) cnt += positive_bits(col[g], limit) ? 1 : 0;
    }
    if (cnt) atomicAdd(&sh[row], cnt);
    __syncthreads();
    if (lane == 0 && s < S && sh[row]) atomicAdd(&colcnt[s], sh[row]);
}

// positives per gene over the columns that :618 keeps (colcnt[s] > min_profiles, the comparison filter_maps.h makes on the host).
// Block b: gene tile b % gtiles (gx genes), columns (b / gtiles) * cpb .. + cpb, dealt to the rows of lanes.
template <class W>
__global__ __launch_bounds__(kFThreads) void f_count_genes(const W *__restrict__ X, int64_t ld, int G, int S, int gxl, int gtiles, W limit,
                                                          const int32_t *__restrict__ colcnt, int64_t min_profiles,
                                                          int32_t *__restrict__ genecnt)
{
    __shared__ int32_t sh[kFThreads];
    const int gx = 1 << gxl, sy = kFThreads >> gxl;
    const int lane = threadIdx.x & (gx - 1), row = threadIdx.x >> gxl;
    const int g = static_cast<int>(blockIdx.x % gtiles) * gx + lane;
    const int64_t cpb = static_cast<int64_t>(sy) * kFColsPer;
    const int64_t s0 = static_cast<int64_t>(blockIdx.x / gtiles) * cpb, s1 = s0 + cpb < S ? s0 + cpb : static_cast<int64_t>(S);
    sh[threadIdx.x] = 0;
    __syncthreads();
    int cnt = 0;
    if (g < G)
        for (int64_t s = s0 + row; s < s1; s += sy)
            if (static_cast<int64_t>(colcnt[s]) > min_profiles) cnt += positive_bits(X[s * ld + g], limit) ? 1 : 0;
    if (cnt) atomicAdd(&sh[lane], cnt);
    __syncthreads();
    if (row == 0 && g < G && sh[lane]) atomicAdd(&genecnt[g], sh[lane]);
}

// out[s' * Gk + g'] = X[src_col[s'] * ld + src_gene[g']]; W is the element's width only
template <class W>
__global__ __launch_bounds__(kFThreads) void f_gather(const W *__restrict__ X, int64_t ld, const int32_t *__restrict__ src_col,
                                                     const int32_t *__restrict__ src_gene, int Gk, int Sk, int gxl, int gtiles,
                                                     W *__restrict__ out)
{
    const int gx = 1 << gxl, sy = kFThreads >> gxl;
    const int lane = threadIdx.x & (gx - 1), row = threadIdx.x >> gxl;
    const int g = static_cast<int>(blockIdx.x % gtiles) * gx + lane;
    const int64_t s = static_cast<int64_t>(blockIdx.x / gtiles) * sy + row;
    if (g < Gk && s < Sk) out[s * Gk + g] = X[static_cast<int64_t>(src_col[s]) * ld + src_gene[g]];
}

template <class W>
void launch_filter_counts(reo_ctx *c, W limit, int64_t min_profiles, int32_t *colcnt, int32_t *genecnt)
{
    const int G = static_cast<int>(c->G), S = static_cast<int>(c->S);
    const int gxl = lanes_log2(G), gx = 1 << gxl, sy = kFThreads >> gxl;
    const W *X = static_cast<const W *>(c->dX);
    const int gsplit = (G + gx * kFGenesPer - 1) / (gx * kFGenesPer);
    const int64_t colgroups = (static_cast<int64_t>(S) + sy - 1) / sy;
    f_count_cols<W><<<static_cast<unsigned>(colgroups * gsplit), kFThreads, 0, c->stream>>>(X, c->ld, G, S, gxl, gsplit, limit, colcnt);
    const int gtiles = (G + gx - 1) / gx;
    const int64_t cpb = static_cast<int64_t>(sy) * kFColsPer, csplit = (S + cpb - 1) / cpb;
    f_count_genes<W><<<static_cast<unsigned>(csplit * gtiles), kFThreads, 0, c->stream>>>(X, c->ld, G, S, gxl, gtiles, limit, colcnt, min_profiles, genecnt);
}

template <class W>
void launch_gather(reo_ctx *c, const int32_t *src_col, const int32_t *src_gene, int64_t Gk, int64_t Sk, void *out)
{
    const int gxl = lanes_log2(Gk), gx = 1 << gxl, sy = kFThreads >> gxl;
    const int gtiles = static_cast<int>((Gk + gx - 1) / gx);
    const int64_t colgroups = (Sk + sy - 1) / sy;
    f_gather<W><<<static_cast<unsigned>(colgroups * gtiles), kFThreads, 0, c->stream>>>(static_cast<const W *>(c->dX), c->ld, src_col, src_gene,
                                                                                     static_cast<int>(Gk), static_cast<int>(Sk), gxl, gtiles,
                                                                                     static_cast<W *>(out));
}

}  // namespace

// The caller (api.hip) has checked the context and invalidated it.  On a refusal or a failure the context holds no matrix.
int32_t filter_matrix(reo_ctx *c, int64_t min_profiles, int64_t min_features, uint8_t *profile_kept, uint8_t *gene_kept,
                      int64_t *S_kept, int64_t *G_kept)
{
    const int64_t G = c->G, S = c->S;
    const size_t eb = c->dtype == 3 ? 4 : 8;
    auto drop = [&](int32_t rc) { c->dtype = 0; c->dX = nullptr; return rc; };
    DevBuf<int32_t> cnt, lists;
    int32_t rc;
    if ((rc = cnt.ensure(static_cast<size_t>(S + G)))) return drop(rc);
    std::vector<int32_t> hcnt(static_cast<size_t>(S + G));
    hipError_t e = hipMemsetAsync(cnt.p, 0, static_cast<size_t>(S + G) * sizeof(int32_t), c->stream);
    if (e == hipSuccess) {
        tic(c, 7);
        switch (c->dtype) {
        case 1: launch_filter_counts<long long>(c, kPosLimitF64, min_profiles, cnt.p, cnt.p + S); break;
        case 2: launch_filter_counts<long long>(c, kPosLimitI64, min_profiles, cnt.p, cnt.p + S); break;
        default: launch_filter_counts<int32_t>(c, kPosLimitF32, min_profiles, cnt.p, cnt.p + S); break;
        }
        toc(c);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(hcnt.data(), cnt.p, hcnt.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);   // nothing queued writes hcnt after return
        set_error("filter_matrix: counting failed: %s", hipGetErrorString(e));
        return drop(e == hipErrorOutOfMemory ? REO_ENOMEM : REO_EHIP);
    }
    const FilterMaps m = filter_maps(hcnt.data(), S, G, min_profiles, min_features, profile_kept, gene_kept);
    if (S_kept) *S_kept = m.S_kept;
    if (G_kept) *G_kept = m.G_kept;
    if (m.too_small) {
        set_error("filter_matrix: %lld of %lld genes and %lld of %lld profiles are left (min_profiles = %lld, min_features = %lld); "
                  "at least 2 of each are needed", (long long)m.G_kept, (long long)G, (long long)m.S_kept, (long long)S,
                  (long long)min_profiles, (long long)min_features);
        collect_timings(c);
        return drop(REO_EINVAL);
    }
    if (m.identity) { collect_timings(c); return REO_OK; }   // nothing dropped: no copy, a caller's buffer stays the matrix
    // compaction into a buffer of the context's own (a caller's _dev buffer is never written), which then replaces dX_owned
    DevBuf<unsigned char> fresh;
    if ((rc = fresh.ensure(static_cast<size_t>(m.G_kept) * m.S_kept * eb)) || (rc = lists.ensure(static_cast<size_t>(m.S_kept + m.G_kept))))
        return drop(rc);
    e = hipMemcpyAsync(lists.p, m.src_col.data(), m.src_col.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(lists.p + m.S_kept, m.src_gene.data(), m.src_gene.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        tic(c, 7);
        if (eb == 8) launch_gather<long long>(c, lists.p, lists.p + m.S_kept, m.G_kept, m.S_kept, fresh.p);
        else launch_gather<int32_t>(c, lists.p, lists.p + m.S_kept, m.G_kept, m.S_kept, fresh.p);
        toc(c);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);   // the source lists are locals
        set_error("filter_matrix: compaction failed: %s", hipGetErrorString(e));
        return drop(e == hipErrorOutOfMemory ? REO_ENOMEM : REO_EHIP);
    }
    std::swap(fresh.p, c->dX_owned.p);   // (fresh now holds the old matrix of the context, if it owned one, and releases it)
    std::swap(fresh.n, c->dX_owned.n);
    c->dX = c->dX_owned.p;
    c->G = m.G_kept; c->S = m.S_kept; c->ld = m.G_kept;
    collect_timings(c);
    return REO_OK;
}

}  // namespace reo
