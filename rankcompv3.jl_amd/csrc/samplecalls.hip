// reo_sample_calls: the calls (+1 / -1 / 0) per query gene and sample, formed on the device from the tails that k_sample_fisher
// (sampletests.hip) leaves there.  Shared arithmetic and host checks: sample_calls.h.
//   k_call_rank   per batch, one thread per cell: the two-sided value, its Benjamini-Hochberg rank m (call_bh_rank), the direction and the
//                 pval_deg bit as one 32-bit word (call_word).  The tails are read along samples ([batch][S]), the words are stored
//                 along queries into the resident buffer laid out by sample, w[s * n_pad + q], through a 32 x 32 LDS tile (one padding
//                 column: no bank conflict either way); loads and stores are coalesced.
//   k_call_cut    one workgroup per sample column: the histogram of the column's ranks in LDS, kCallBins ranks per tile, a scan of the
//                 tile that keeps the largest r with H(r) >= r and carries the running sum into the next tile.  H never exceeds the
//                 number F of rows that have a rank, so no r above F qualifies: the first sweep counts F and the tiles end at
//                 min(n, F).  A last sweep counts the rows within the cut and the calls of either sign.  LDS atomics only.
//   k_call_emit   the reverse transpose: words read along queries, the call of each under its column's cut (call_of), int8 stored along
//                 samples into [n][S].
// Addresses: none is formed from a cell's value.  A rank indexes the LDS histogram only after 1 <= m <= n and 0 <= m - 1 - tile0 <
// kCallBins have been tested; every global index is q * S + s or s * n_pad + q with q < n (<= n_pad) and s < S tested, in 64 bits.
// Padding rows n .. n_pad - 1 of the word buffer are neither stored nor read.
#include "sample_calls.h"
#include "reo_internal.h"

namespace reo {

namespace {

constexpr int kCallThreads = 256;                         // every kernel of this unit
constexpr int kCallRowsPerPass = kCallThreads / kCallTile;   // 8 tile rows per pass, 4 passes per tile
constexpr int kCallBinsPerThread = kCallBins / kCallThreads;
static_assert(kCallBinsPerThread == 32 && kCallTile == 32, "the padded histogram index assumes 32 bins per thread");

struct CallRankArgs {
    const double *p_up, *p_down;   // [nq][S] of the batch
    uint32_t *w;                   // [S][n_pad]
    int64_t n_pad, q0;
    double pval_deg, padj_deg;
    int n, nq, S;                  // n: rows of the whole call (the n of the step-up rule)
};

__global__ __launch_bounds__(kCallThreads) void k_call_rank(CallRankArgs a)
{
    __shared__ uint32_t tile[kCallTile][kCallTile + 1];
    const int tx = threadIdx.x & (kCallTile - 1), ty = threadIdx.x / kCallTile;
    const int qt = blockIdx.x * kCallTile, st = blockIdx.y * kCallTile;
#pragma unroll
    for (int j = 0; j < kCallTile; j += kCallRowsPerPass) {
        const int q = qt + ty + j, s = st + tx;
        uint32_t word = 0;
        if (q < a.nq && s < a.S) {
            const int64_t o = static_cast<int64_t>(q) * a.S + s;
            word = call_word(a.p_up[o], a.p_down[o], a.n, a.pval_deg, a.padj_deg);
        }
        tile[ty + j][tx] = word;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kCallTile; j += kCallRowsPerPass) {
        const int s = st + ty + j, q = qt + tx;
        if (q < a.nq && s < a.S) a.w[static_cast<int64_t>(s) * a.n_pad + a.q0 + q] = tile[tx][ty + j];
    }
}

struct CallCutArgs {
    const uint32_t *w;   // [S][n_pad]
    int32_t *kstar, *cut, *n_up, *n_down;   // [S] each
    int64_t n_pad;
    int n;
};

// bin b of a tile lives at b + b / 32: thread t scans the words 33 t .. 33 t + 31, so the 32 lanes of a half wave read 32 different banks
__device__ __forceinline__ int call_bin_at(int b) { return b + (b >> 5); }

__global__ __launch_bounds__(kCallThreads) void k_call_cut(CallCutArgs a)
{
    __shared__ int hist[kCallBins + kCallBins / 32];
    __shared__ int wsum[kCallThreads / 64];
    __shared__ int sh_best, sh_finite, sh_cnt[3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = a.n;
    const uint32_t *col = a.w + static_cast<int64_t>(blockIdx.x) * a.n_pad;
    for (int b = tid; b < kCallBins + kCallBins / 32; b += kCallThreads) hist[b] = 0;
    if (tid == 0) { sh_best = 0; sh_finite = 0; sh_cnt[0] = sh_cnt[1] = sh_cnt[2] = 0; }
    __syncthreads();
    int carry = 0, lim = n;   // workgroup-uniform
    for (int tile0 = 0; tile0 < lim; tile0 += kCallBins) {
        int finite = 0;
        for (int i = tid; i < n; i += kCallThreads) {
            const int m = call_word_rank(col[i]);
            if (m >= 1 && m <= n) {
                ++finite;
                const int b = m - 1 - tile0;
                if (b >= 0 && b < kCallBins) atomicAdd(&hist[call_bin_at(b)], 1);
            }
        }
        if (tile0 == 0 && finite) atomicAdd(&sh_finite, finite);
        __syncthreads();
        // this thread's 32 bins, then the exclusive prefix of the threads in front of it
        const int b0 = tid * kCallBinsPerThread;
        int s = 0;
#pragma unroll
        for (int u = 0; u < kCallBinsPerThread; ++u) s += hist[call_bin_at(b0 + u)];
        int inc = s;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(inc, o, 64); if (lane >= o) inc += v; }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        int before = carry + inc - s, total = 0;
#pragma unroll
        for (int v = 0; v < kCallThreads / 64; ++v) { if (v < wave) before += wsum[v]; total += wsum[v]; }
        int run = before, best = 0;
#pragma unroll
        for (int u = 0; u < kCallBinsPerThread; ++u) {
            const int at = call_bin_at(b0 + u), r = tile0 + b0 + u + 1;
            run += hist[at];
            hist[at] = 0;   // for the next tile
            if (r <= n && run >= r) best = r;
        }
        if (best) atomicMax(&sh_best, best);
        carry += total;
        if (tile0 == 0) lim = min(n, sh_finite);   // (written before the first barrier of this round, read by everyone behind it)
        __syncthreads();   // wsum and the histogram are free again
    }
    const int kstar = sh_best;   // behind the last barrier of the loop (or the one in front of it: 0)
    int cnt = 0, up = 0, down = 0;
    for (int i = tid; i < n; i += kCallThreads) {
        const uint32_t word = col[i];
        const int m = call_word_rank(word);
        if (m >= 1 && m <= kstar) {
            ++cnt;
            const int8_t call = call_of(word, kstar);
            up += call > 0;
            down += call < 0;
        }
    }
    if (cnt) { atomicAdd(&sh_cnt[0], cnt); atomicAdd(&sh_cnt[1], up); atomicAdd(&sh_cnt[2], down); }
    __syncthreads();
    if (tid == 0) {
        a.kstar[blockIdx.x] = kstar;
        a.cut[blockIdx.x] = sh_cnt[0];
        a.n_up[blockIdx.x] = sh_cnt[1];
        a.n_down[blockIdx.x] = sh_cnt[2];
    }
}

struct CallEmitArgs {
    const uint32_t *w;      // [S][n_pad]
    const int32_t *kstar;   // [S]
    int8_t *calls;          // [n][S]
    int64_t n_pad;
    int n, S;
};

__global__ __launch_bounds__(kCallThreads) void k_call_emit(CallEmitArgs a)
{
    __shared__ int8_t tile[kCallTile][kCallTile + 4];
    const int tx = threadIdx.x & (kCallTile - 1), ty = threadIdx.x / kCallTile;
    const int qt = blockIdx.x * kCallTile, st = blockIdx.y * kCallTile;
#pragma unroll
    for (int j = 0; j < kCallTile; j += kCallRowsPerPass) {
        const int s = st + ty + j, q = qt + tx;
        int8_t call = 0;
        if (q < a.n && s < a.S) call = call_of(a.w[static_cast<int64_t>(s) * a.n_pad + q], a.kstar[s]);
        tile[ty + j][tx] = call;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kCallTile; j += kCallRowsPerPass) {
        const int q = qt + ty + j, s = st + tx;
        if (q < a.n && s < a.S) a.calls[static_cast<int64_t>(q) * a.S + s] = tile[tx][ty + j];
    }
}

bool call_grid(int64_t rows, int64_t S, dim3 *grid)
{
    const int64_t gx = (rows + kCallTile - 1) / kCallTile, gy = (S + kCallTile - 1) / kCallTile;
    if (rows < 1 || S < 1 || gx > 0x7FFFFFFF || gy > 65535) return false;
    *grid = dim3(static_cast<unsigned>(gx), static_cast<unsigned>(gy));
    return true;
}

}  // namespace

int32_t launch_call_rank(reo_ctx *c, int64_t n_genes, int64_t q0, int64_t nq, const double *d_p_up, const double *d_p_down, double pval_deg,
                         double padj_deg, uint32_t *d_words)
{
    CallRankArgs a;
    dim3 grid;
    if (n_genes < 1 || n_genes > kCallMaxQueries || q0 < 0 || nq < 1 || q0 + nq > n_genes || !call_grid(nq, c->S, &grid)) {
        set_error("reo_sample_calls: a batch of %lld queries x %lld samples cannot be launched", (long long)nq, (long long)c->S);
        return REO_EINVAL;
    }
    a.p_up = d_p_up; a.p_down = d_p_down; a.w = d_words;
    a.n_pad = call_padded_rows(n_genes); a.q0 = q0;
    a.pval_deg = pval_deg; a.padj_deg = padj_deg;
    a.n = static_cast<int>(n_genes); a.nq = static_cast<int>(nq); a.S = static_cast<int>(c->S);
    k_call_rank<<<grid, kCallThreads, 0, c->stream>>>(a);
    REO_HIP_CHECK(hipGetLastError());
    return REO_OK;
}

int32_t launch_call_cut(reo_ctx *c, int64_t n_genes, const uint32_t *d_words, int32_t *d_kstar, int32_t *d_cut, int32_t *d_n_up, int32_t *d_n_down)
{
    if (n_genes < 1 || n_genes > kCallMaxQueries || c->S < 1 || c->S > 0x7FFFFFFF) {
        set_error("reo_sample_calls: %lld sample columns of %lld rows cannot be launched", (long long)c->S, (long long)n_genes);
        return REO_EINVAL;
    }
    CallCutArgs a;
    a.w = d_words; a.kstar = d_kstar; a.cut = d_cut; a.n_up = d_n_up; a.n_down = d_n_down;
    a.n_pad = call_padded_rows(n_genes); a.n = static_cast<int>(n_genes);
    k_call_cut<<<dim3(static_cast<unsigned>(c->S)), kCallThreads, 0, c->stream>>>(a);
    REO_HIP_CHECK(hipGetLastError());
    return REO_OK;
}

int32_t launch_call_emit(reo_ctx *c, int64_t n_genes, const uint32_t *d_words, const int32_t *d_kstar, int8_t *d_calls)
{
    CallEmitArgs a;
    dim3 grid;
    if (n_genes > kCallMaxQueries || !call_grid(n_genes, c->S, &grid)) {
        set_error("reo_sample_calls: %lld queries x %lld samples cannot be launched", (long long)n_genes, (long long)c->S);
        return REO_EINVAL;
    }
    a.w = d_words; a.kstar = d_kstar; a.calls = d_calls;
    a.n_pad = call_padded_rows(n_genes); a.n = static_cast<int>(n_genes); a.S = static_cast<int>(c->S);
    k_call_emit<<<grid, kCallThreads, 0, c->stream>>>(a);
    REO_HIP_CHECK(hipGetLastError());
    return REO_OK;
}

}  // namespace reo
