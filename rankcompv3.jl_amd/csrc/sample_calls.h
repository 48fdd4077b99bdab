// Sample calls (reo_sample_calls): up (+1), down (-1) or nothing (0) per query gene and sample, formed on the device from the two Fisher
// tails of reo_sample_tests: the two-sided value, Benjamini-Hochberg down each sample column over the rows of the call, and the two
// thresholds.  What the kernels of samplecalls.hip and a host driver share, so that the driver can evaluate the very same functions under
// the sanitizers (tests/sample_calls_driver.cpp): the two-sided value, the sort-free form of the step-up rule (rank, histogram, cut), the
// 32-bit cell word, the batch and memory arithmetic and the argument checks that need no GPU.  No HIP header in here: plain C++17 (the
// kernels' unit defines the function attributes through pair_list.h).
//
// The step-up rule without a sort: with m_i = min{r in 1..n : p_i (n / r) <= al} (n + 1: none) and H(r) = #{i : m_i <= r},
// the cut is k* = max{r : H(r) >= r} (0: none) and padj_i <= al  <=>  m_i <= k*.  p (n / r) is the expression that bh_columns (_ffi.py)
// evaluates, with the same two roundings, so the calls are those of SampleTests.calls bit for bit.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "sample_tests.h"

namespace reo {

constexpr int kCallBins = 8192;                 // histogram bins (ranks) per tile of k_call_cut: 32 KB of LDS besides the scan's scratch
constexpr int kCallTile = 32;                   // edge of the square tiles that the two transposes move
constexpr uint32_t kCallRankBits = 29;          // the cell word: rank in bits 0 .. 28, pval <= pval_deg in bit 29, the direction in bits 30 .. 31
constexpr uint32_t kCallRankMask = (1u << kCallRankBits) - 1u;
constexpr uint32_t kCallPvalBit = 1u << kCallRankBits;
constexpr uint32_t kCallDirShift = kCallRankBits + 1;
constexpr uint32_t kCallUp = 1u, kCallDown = 2u;   // the direction pair: p_up < p_down, p_down < p_up, 0 for equal tails
constexpr int64_t kCallMaxQueries = static_cast<int64_t>(kCallRankMask) - 1;   // the rank n + 1 ("none") must fit the 29 bits

// The two-sided value min(1, 2 min(p_up, p_down)): SampleTests.pval.
REO_PL_FN double call_pval(double p_up, double p_down)
{
    const double t = 2.0 * (p_up < p_down ? p_up : p_down);
    return t < 1.0 ? t : 1.0;
}

REO_PL_FN uint32_t call_direction(double p_up, double p_down) { return p_up < p_down ? kCallUp : (p_down < p_up ? kCallDown : 0u); }

REO_PL_FN bool call_within(double p, double nd, int32_t r, double al) { return p * (nd / static_cast<double>(r)) <= al; }

// m = the smallest rank r in 1 .. n at which p (n / r) <= al; n + 1: none.  The rule of bh_rank in kernels.hip ("Light passes"), restated
// here and not shared: its twin there keeps its registers.  p in [0, 1] (a NaN has no rank), n >= 1, al in [0, 1].  al = 0 has a rank
// only for p = 0 (p (n / r) >= p for r <= n), and no quotient by al is formed then; the estimate is compared as a double before it
// becomes an integer.  p (n / r) does not grow with r (one rounding each in the quotient and the product, both monotone), so the two
// walks from the estimate end at the smallest r.
REO_PL_FN int32_t call_bh_rank(double p, int32_t n, double al)
{
    const double nd = static_cast<double>(n);
    if (!(al > 0.0)) return p == 0.0 ? 1 : n + 1;
    if (!call_within(p, nd, n, al)) return n + 1;
    const double est = ceil(p * nd / al);
    int32_t m = !(est >= 1.0) ? 1 : (est >= nd ? n : static_cast<int32_t>(est));
    while (m > 1 && call_within(p, nd, m - 1, al)) --m;
    while (!call_within(p, nd, m, al)) ++m;   // (within(n) holds)
    return m;
}

// The cell word.  rank in 1 .. n + 1 <= kCallRankMask.
REO_PL_FN uint32_t call_pack(int32_t rank, uint32_t dir, bool pval_ok)
{
    return (static_cast<uint32_t>(rank) & kCallRankMask) | (pval_ok ? kCallPvalBit : 0u) | (dir << kCallDirShift);
}
REO_PL_FN int32_t call_word_rank(uint32_t w) { return static_cast<int32_t>(w & kCallRankMask); }
REO_PL_FN uint32_t call_word_dir(uint32_t w) { return w >> kCallDirShift; }
REO_PL_FN bool call_word_pval_ok(uint32_t w) { return (w & kCallPvalBit) != 0; }

// One cell: the word from the two tails.
REO_PL_FN uint32_t call_word(double p_up, double p_down, int32_t n, double pval_deg, double padj_deg)
{
    const double p = call_pval(p_up, p_down);
    return call_pack(call_bh_rank(p, n, padj_deg), call_direction(p_up, p_down), p <= pval_deg);
}

// The call of a word under the column's cut k*.
REO_PL_FN int8_t call_of(uint32_t w, int32_t kstar)
{
    if (call_word_rank(w) > kstar || !call_word_pval_ok(w)) return 0;
    const uint32_t d = call_word_dir(w);
    return d == kCallUp ? int8_t(1) : (d == kCallDown ? int8_t(-1) : int8_t(0));
}

// k* = max{r in 1 .. n : H(r) >= r} over a whole histogram, hist[b] = the rows of rank b + 1 (0: no r qualifies).  The driver's form; the
// kernel walks the same running sum tile by tile.
inline int32_t call_cut(const int32_t *hist, int32_t n)
{
    int64_t run = 0;
    int32_t best = 0;
    for (int32_t r = 1; r <= n; ++r) {
        run += hist[r - 1];
        if (run >= r) best = r;
    }
    return best;
}

// Rows of the resident word buffer per sample column: n padded to whole tiles.
REO_PL_FN int64_t call_padded_rows(int64_t n_genes) { return (n_genes + kCallTile - 1) / kCallTile * kCallTile; }

// Batch of queries of phase 1: reo_sample_tests' own (st_batch_rows); `env` = REO_SAMPLE_CALLS_BATCH, which can only lower it.
inline int64_t call_batch_rows(int64_t n_genes, int64_t padded_slots, int64_t env) { return st_batch_rows(n_genes, padded_slots, env); }

// Device bytes of a call besides the context's own: the resident words (4 n_pad S), the calls (n S), the query genes (4 n), the four
// per-sample results (16 S), and the buffers of one batch (two selections, four count buffers of padded slots, two of doubles).
inline int64_t call_device_bytes(int64_t n_genes, int64_t S, int64_t padded_slots, int64_t batch)
{
    return 4 * call_padded_rows(n_genes) * S + n_genes * S + 4 * n_genes + 16 * S + batch * (8 + 16 * padded_slots + 16 * S) + 4;
}

// Argument checks of reo_sample_calls that need neither the context's state nor the GPU.  0 when everything is in order; otherwise the
// number of the failed check (1 ..) and its message in msg.  genes is a HOST array.
inline int sample_calls_check_args(int64_t G, const int32_t *genes, int64_t n_genes, double pval_deg, double padj_deg, const int8_t *calls,
                                   char *msg, size_t msg_n)
{
    if (!genes || !calls) { snprintf(msg, msg_n, "reo_sample_calls: genes and calls must not be null"); return 1; }
    if (n_genes < 1 || n_genes > kCallMaxQueries) {
        snprintf(msg, msg_n, "reo_sample_calls: n_genes = %lld, between 1 and 2^29 - 2 query genes per call", (long long)n_genes);
        return 2;
    }
    if (!(pval_deg >= 0.0 && pval_deg <= 1.0)) { snprintf(msg, msg_n, "reo_sample_calls: pval_deg = %g is not a number in [0, 1]", pval_deg); return 3; }
    if (!(padj_deg >= 0.0 && padj_deg <= 1.0)) { snprintf(msg, msg_n, "reo_sample_calls: padj_deg = %g is not a number in [0, 1]", padj_deg); return 4; }
    return query_genes_in_range("reo_sample_calls", G, genes, n_genes, msg, msg_n) ? 0 : 5;
}

}  // namespace reo
