// Sample tests (reo_sample_tests): is gene i up or down in ONE sample?  The pairs that are stable in the control group are the background,
// the sample's orderings are tested against it with Fisher's exact test.  What the kernel of sampletests.hip and a host driver share, so
// that the driver can evaluate the very same functions under the sanitizers (tests/sample_tests_driver.cpp): the 2 x 2 table from the six
// device counts, the two hypergeometric tails, the log-factorial table they read, the batch sizing and the argument checks that need no
// GPU.  No HIP header in here: plain C++17 (the kernel's unit defines the function attributes through pair_list.h).
//
// The table is [[a, b], [u, d]]: a = n_above_ctrl, b = n_below_ctrl, u = partners below gene i in the sample, d = partners above it.
// N = a + b + u + d, K = a + u, n = u + d, X ~ Hypergeometric(N, K, n); p_up = P(X >= u), p_down = P(X <= u).  The support of X is
// max(0, u - b) .. min(n, K): u always lies inside it.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "sample_counts.h"

// Every read of the log-factorial table goes through this; the host driver replaces it with a read that checks i <= N < entries.
#ifndef REO_ST_LF_AT
#define REO_ST_LF_AT(lf, i, N, entries) ((lf)[(i)])
#endif

namespace reo {

constexpr uint32_t kStMaskAbove = 0x1C0;   // ic = 3: gene i stably above j in the control group (n31 | n32 | n33)
constexpr uint32_t kStMaskBelow = 0x007;   // ic = 1 (n11 | n12 | n13)
constexpr double kStCut = 0x1p-60;         // the recurrence ends when a term falls below this share of the sum so far

struct StTable {
    int64_t a, b, u, d;              // the 2 x 2 table
    int32_t rev_up, rev_down, tied;  // what the call reports besides the tails
};

// Entries of the log-factorial table of a problem with G genes: lf[0 .. 2 (G - 1)] (N <= 2 |J| <= 2 (G - 1)).
REO_PL_FN int64_t st_lf_entries(int64_t G) { return G < 1 ? 1 : 2 * (G - 1) + 1; }

// lf[k] = log k!: a running sum of logl(k) in long double, rounded once per entry.
inline void st_build_lf(int64_t G, std::vector<double> &lf)
{
    const int64_t n = st_lf_entries(G);
    lf.assign(static_cast<size_t>(n), 0.0);
    long double acc = 0.0L;
    for (int64_t k = 1; k < n; ++k) {
        acc += logl(static_cast<long double>(k));
        lf[static_cast<size_t>(k)] = static_cast<double>(acc);
    }
}

// The table from the six counts of the two launch_sample_counts calls (A: class mask 0x1C0, B: 0x007): sel = selected partners of the
// query, gt / eq = of those, in how many the gene lies above its partner / is tied with it in this sample.  false (t untouched) when
// the counts cannot come from G genes -- nothing may be indexed with them then.
REO_PL_FN bool st_table(int64_t G, int32_t sel_a, int32_t sel_b, int32_t gt_a, int32_t eq_a, int32_t gt_b, int32_t eq_b, StTable *t)
{
    if (sel_a < 0 || sel_b < 0 || gt_a < 0 || eq_a < 0 || gt_b < 0 || eq_b < 0) return false;
    if (static_cast<int64_t>(sel_a) + sel_b > G - 1) return false;
    if (static_cast<int64_t>(gt_a) + eq_a > sel_a || static_cast<int64_t>(gt_b) + eq_b > sel_b) return false;
    t->a = sel_a;
    t->b = sel_b;
    t->u = static_cast<int64_t>(gt_a) + gt_b;
    t->tied = eq_a + eq_b;
    t->d = t->a + t->b - t->u - t->tied;
    t->rev_up = gt_b;
    t->rev_down = sel_a - gt_a - eq_a;
    return true;
}

// p_up = P(X >= u), p_down = P(X <= u) of the table above.  lf has `entries` entries and N = a + b + u + d must be < entries (st_table
// with the G that sized lf guarantees it; otherwise both tails are NaN and nothing is read).  pmf(u) comes from the table, the tail that
// points away from the mode from the ratio recurrence (integer products formed exactly, then divided), the other tail is
// 1 - small + pmf(u); both are clamped to [0, 1].
REO_PL_FN void st_tails(const double *lf, int64_t entries, int64_t a, int64_t b, int64_t u, int64_t d, double *p_up, double *p_down)
{
    const int64_t N = a + b + u + d, K = a + u, n = u + d, M = b + d;   // M = N - K
    if (a < 0 || b < 0 || u < 0 || d < 0 || N >= entries) {
        *p_up = *p_down = NAN;
        return;
    }
    if (n == 0) {   // an empty background, or every pair tied: nothing to test
        *p_up = *p_down = 1.0;
        return;
    }
    // log pmf(u) = log C(K, u) + log C(M, d) - log C(N, n)
    const double lk = REO_ST_LF_AT(lf, K, N, entries) - REO_ST_LF_AT(lf, u, N, entries) - REO_ST_LF_AT(lf, a, N, entries);
    const double lm = REO_ST_LF_AT(lf, M, N, entries) - REO_ST_LF_AT(lf, d, N, entries) - REO_ST_LF_AT(lf, b, N, entries);
    const double ln = REO_ST_LF_AT(lf, N, N, entries) - REO_ST_LF_AT(lf, n, N, entries) - REO_ST_LF_AT(lf, N - n, N, entries);
    const double pm = exp((lk + lm) - ln);
    const int64_t mode = ((n + 1) * (K + 1)) / (N + 2);
    const int64_t lo = u > b ? u - b : 0, hi = n < K ? n : K;
    const bool upper = u > mode;   // the upper tail is the small one
    double s = pm, t = pm;
    if (pm > 0.0) {
        if (upper) {
            for (int64_t x = u; x < hi; ++x) {   // pmf(x + 1) / pmf(x)
                t = t * static_cast<double>((K - x) * (n - x)) / static_cast<double>((x + 1) * (M - n + x + 1));
                s += t;
                if (t < s * kStCut) break;
            }
        } else {
            for (int64_t x = u; x > lo; --x) {   // pmf(x - 1) / pmf(x)
                t = t * static_cast<double>(x * (M - n + x)) / static_cast<double>((K - x + 1) * (n - x + 1));
                s += t;
                if (t < s * kStCut) break;
            }
        }
    }
    double large = 1.0 - s + pm;
    if (s > 1.0) s = 1.0;
    if (large > 1.0) large = 1.0;
    if (large < 0.0) large = 0.0;
    *p_up = upper ? s : large;
    *p_down = upper ? large : s;
}

// Batch of queries: the count buffers take padded slots x 4 bytes a row, the two buffers of doubles S x 8 <= padded slots x 8; sized as
// sc_batch_rows sizes its own with rows of twice the length, so that every device buffer stays under kScBudgetBytes.  `env` =
// REO_SAMPLE_TESTS_BATCH in queries (tests), which can only lower it.
inline int64_t st_batch_rows(int64_t n_genes, int64_t padded_slots, int64_t env) { return sc_batch_rows(n_genes, 2 * padded_slots, env); }

// Argument checks of reo_sample_tests that need neither the context's state nor the GPU.  0 when everything is in order; otherwise the
// number of the failed check (1 ..) and its message in msg.  genes is a HOST array.
inline int sample_tests_check_args(int64_t G, const int32_t *genes, int64_t n_genes, const double *p_up, const double *p_down, char *msg,
                                   size_t msg_n)
{
    if (!genes || !p_up || !p_down) { snprintf(msg, msg_n, "reo_sample_tests: genes, p_up and p_down must not be null"); return 1; }
    if (n_genes < 1 || n_genes > kScMaxQueries) {
        snprintf(msg, msg_n, "reo_sample_tests: n_genes = %lld, between 1 and 2^30 query genes per call", (long long)n_genes);
        return 2;
    }
    return query_genes_in_range("reo_sample_tests", G, genes, n_genes, msg, msg_n) ? 0 : 3;
}

}  // namespace reo
