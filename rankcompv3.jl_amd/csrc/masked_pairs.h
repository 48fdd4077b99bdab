// Missing values (reo_set_valid_mask, reo_build_pairs_masked, reo_pair_counts_masked): a pair (i, j) is compared in the samples where BOTH
// genes were observed, and each side of its class is judged against the threshold of that many samples.  What the kernels of
// maskedpairs.hip, the entry points of api.hip and a host driver share, so that the driver can evaluate the very same functions under the
// sanitizers (tests/masked_pairs_driver.cpp): the side-class rule, the packing of a validity word, the counts of one block of 32 sample
// slots, the threshold function and its table, and the argument checks -- all of which run on the host before anything is uploaded.
// No HIP header in here: plain C++17 (the kernels' unit defines the function attributes through pair_list.h).
//
// The comparison itself is the borrow chain of k1_counts over the pos / lo / hi planes (band_chain.h); it yields, for one pair and one block of
// 32 sample slots, a word `lt` (bit s: x_i > x_j and not tied in slot s) and a word `le` (bit s: greater or tied).  The planes are those of
// the whole matrix: the cell under an invalid byte takes part in its sample's ranking (the caller writes a filler there), and the validity
// words take its comparisons out again.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "pair_list.h"

namespace reo {

constexpr int64_t kMpMaxGenes = 65535;      // the 16-plane layout only
constexpr int64_t kMpMaxSamples = 65535;
constexpr int kMpRows = 8;                  // table rows that one wave of k_pairs_masked walks with a column's planes in registers
constexpr int64_t kMpMaxRect = int64_t(1) << 28;   // counts per array of one reo_pair_counts_masked call (rows x columns x groups)

// get_major_reo_lower_count, src/RankCompV3.jl:81-92, with
// pvalue(Binomial(n, 1/2), x; tail = :both) = min(1, 2 min(ccdf(x-1), cdf(x)))
// (HypothesisTests, call sites :83,85).  The cdf is accumulated term by term in
// long double, pmf(t) = exp(log C(n,t) - n ln 2), so the scan over x is O(n).
inline int32_t reo_lower_count(int32_t n, double thr)
{
    const long double ln2 = 0.693147180559945309417232121458L;
    long double logc = 0.0L, cdf_prev = 0.0L;  // cdf(x-1)
    int32_t first_above = -1;
    double pmin = 1.0;
    for (int x = 0; x <= n / 2; ++x) {
        if (x > 0) logc += std::log(static_cast<long double>(n - x + 1)) - std::log(static_cast<long double>(x));
        long double cdf = x >= n ? 1.0L : cdf_prev + std::exp(logc - static_cast<long double>(n) * ln2);
        if (cdf > 1.0L) cdf = 1.0L;
        const long double hi = 1.0L - cdf_prev;
        long double p = 2.0L * (cdf < hi ? cdf : hi);
        if (p > 1.0L) p = 1.0L;
        if (x == 0) {
            pmin = static_cast<double>(p);
            if (!(pmin < thr)) return n;  // the WARN branch (:87-90)
        }
        if (static_cast<double>(p) > thr) { first_above = x; break; }
        cdf_prev = cdf;
    }
    return first_above < 0 ? -1 : n - first_above + 1;  // -idx + 2 + n with idx = x + 1
}

// m(0 .. n_side): the threshold of every number of jointly observed samples that a side of n_side samples can have.  false when some n has
// none (reo_lower_count answers -1: pval_reo = 1).  O(n_side^2) host arithmetic, made once per (side sizes, pval_reo) and kept.
inline bool mp_threshold_table(int32_t n_side, double pval_reo, std::vector<int32_t> &m)
{
    m.assign(static_cast<size_t>(n_side < 0 ? 0 : n_side) + 1, 0);
    for (int32_t n = 0; n <= n_side; ++n) {
        m[static_cast<size_t>(n)] = reo_lower_count(n, pval_reo);
        if (m[static_cast<size_t>(n)] < 0) return false;
    }
    return true;
}

// The smallest n with min(1, 2 * 0.5^n) < pval_reo: the first n at which reo_lower_count leaves its fallback branch (8 at 0.01), what
// min_complete defaults to per side (capped by the side's size).  pval_reo in (0, 1].
inline int32_t mp_first_informative_n(double pval_reo)
{
    int32_t n = 1;
    double p = 1.0;   // 2 * 0.5^n
    while (n < 2000 && !((p < 1.0 ? p : 1.0) < pval_reo)) { ++n; p *= 0.5; }
    return n;
}

// The class of one side: a of its n jointly observed samples show x_i > x_j (coins included), m = m(n).  1: stably below, 3: stably above,
// 2: unstable -- and always 2 with fewer than min_complete samples, never "stable by unanimity of three samples".
REO_PL_FN int mp_side_class(int32_t a, int32_t n, int32_t m, int32_t min_complete)
{
    if (n < min_complete) return 2;
    if (a >= m) return 3;
    if (n - a >= m) return 1;
    return 2;
}

// The class code 3 (ic - 1) + (it - 1) of the ordered pair, and the sides of the mirrored pair (its code is 8 minus this one).
REO_PL_FN uint32_t mp_pair_code(int ic, int it) { return static_cast<uint32_t>(3 * (ic - 1) + (it - 1)); }
REO_PL_FN int mp_mirror_side(int side) { return 4 - side; }

// The validity word of gene `gene` in one block of 32 sample slots: bit s = the byte of the slot's column (slot2col: the caller's column of
// every slot of the block, -1 for padding).  valid is [S][G] bytes, column-major.  Padding slots and genes >= G give 0.
REO_PL_FN uint32_t mp_valid_word(const uint8_t *valid, int64_t G, int64_t S, int64_t gene, const int32_t *slot2col /* 32 */)
{
    if (gene < 0 || gene >= G) return 0u;
    uint32_t w = 0;
    for (int s = 0; s < 32; ++s) {
        const int64_t col = slot2col[s];
        if (col >= 0 && col < S && valid[col * G + gene] != 0) w |= 1u << s;
    }
    return w;
}

// One block's share of the three counts of a pair: v = V_i & V_j.
REO_PL_FN void mp_count_block(uint32_t lt, uint32_t le, uint32_t v, uint32_t &n_gt, uint32_t &n_eq, uint32_t &n_avail)
{
    n_gt += static_cast<uint32_t>(__builtin_popcount(lt & v));
    n_eq += static_cast<uint32_t>(__builtin_popcount(le & ~lt & v));
    n_avail += static_cast<uint32_t>(__builtin_popcount(v));
}

// What the checks need to know of the context.
struct MpState {
    bool multi;           // a reo_create_multi context (leader or peer)
    int32_t world;        // reo_set_shard
    int64_t G, S;         // the resident matrix (0 x 0: none)
    int32_t ngroups;
    bool has_mask;        // a mask is set and has the matrix's shape
};

// reo_set_valid_mask (valid != NULL).  0 when everything is in order; otherwise the number of the failed check (1 ..) and its message.
inline int mp_check_mask_args(const MpState &st, int64_t G, int64_t S, int64_t ld, char *msg, size_t msg_n)
{
    if (st.G < 1 || st.S < 1) { snprintf(msg, msg_n, "reo_set_valid_mask: no expression matrix set (the mask belongs to a resident matrix)"); return 1; }
    if (G != st.G || S != st.S) {
        snprintf(msg, msg_n, "reo_set_valid_mask: the mask is %lld x %lld, the matrix %lld x %lld", (long long)G, (long long)S, (long long)st.G,
                 (long long)st.S);
        return 2;
    }
    if (ld < G) { snprintf(msg, msg_n, "reo_set_valid_mask: leading dimension %lld < G = %lld", (long long)ld, (long long)G); return 3; }
    return 0;
}

// What reo_build_pairs_masked and reo_pair_counts_masked share (what = the call's name).
inline int mp_check_context(const char *what, const MpState &st, char *msg, size_t msg_n)
{
    if (st.multi) {
        snprintf(msg, msg_n, "%s is not available on a reo_create_multi context (the validity mask lives on one device)", what);
        return 1;
    }
    if (st.world > 1) {
        snprintf(msg, msg_n, "%s is not available on a sharded context (reo_set_shard: %d shards; the masked build has no exchange)", what, st.world);
        return 2;
    }
    if (!st.has_mask) {
        snprintf(msg, msg_n, "%s: no validity mask of the matrix's shape (%lld x %lld) is set (reo_set_valid_mask; a matrix of another shape drops it)",
                 what, (long long)st.G, (long long)st.S);
        return 3;
    }
    if (st.S > kMpMaxSamples) { snprintf(msg, msg_n, "%s: S = %lld, at most 65535 samples", what, (long long)st.S); return 4; }
    if (st.G > kMpMaxGenes) { snprintf(msg, msg_n, "%s: G = %lld, at most 65535 genes (the 16-plane layout only)", what, (long long)st.G); return 5; }
    return 0;
}

inline int mp_check_build_args(const MpState &st, int32_t k, double pval_reo, const int32_t *min_complete, char *msg, size_t msg_n)
{
    const int rc = mp_check_context("reo_build_pairs_masked", st, msg, msg_n);
    if (rc) return rc;
    if (!min_complete) { snprintf(msg, msg_n, "reo_build_pairs_masked: min_complete must not be null (two integers, one per side)"); return 6; }
    if (min_complete[0] < 1 || min_complete[1] < 1) {
        snprintf(msg, msg_n, "reo_build_pairs_masked: min_complete = (%d, %d), each side needs at least 1 jointly observed sample", min_complete[0],
                 min_complete[1]);
        return 7;
    }
    if (!(pval_reo > 0.0 && pval_reo <= 1.0)) { snprintf(msg, msg_n, "reo_build_pairs_masked: pval_reo = %g is outside (0, 1]", pval_reo); return 8; }
    if (k < 0 || k >= st.ngroups) { snprintf(msg, msg_n, "reo_build_pairs_masked: comparison %d outside [0,%d)", k, st.ngroups); return 9; }
    return 0;
}

inline int mp_check_counts_args(const MpState &st, int64_t i0, int64_t i1, int64_t j0, int64_t j1, const int32_t *n_gt, const int32_t *n_eq,
                                const int32_t *n_avail, char *msg, size_t msg_n)
{
    const int rc = mp_check_context("reo_pair_counts_masked", st, msg, msg_n);
    if (rc) return rc;
    if (!n_gt || !n_eq || !n_avail) { snprintf(msg, msg_n, "reo_pair_counts_masked: n_gt, n_eq and n_avail must not be null"); return 6; }
    if (i0 < 0 || j0 < 0 || i1 > st.G || j1 > st.G || i0 >= i1 || j0 >= j1) {
        snprintf(msg, msg_n, "reo_pair_counts_masked: bad pair block [%lld,%lld) x [%lld,%lld)", (long long)i0, (long long)i1, (long long)j0,
                 (long long)j1);
        return 7;
    }
    if ((i1 - i0) * (j1 - j0) > kMpMaxRect / (st.ngroups < 1 ? 1 : st.ngroups)) {
        snprintf(msg, msg_n, "reo_pair_counts_masked: %lld x %lld pairs x %d groups, at most 2^28 counts per call: ask in row strips",
                 (long long)(i1 - i0), (long long)(j1 - j0), st.ngroups);
        return 8;
    }
    return 0;
}

// The refusal of a call that compares on the bit planes while a mask is set.
inline void mp_query_refusal(const char *what, char *msg, size_t msg_n)
{
    snprintf(msg, msg_n, "%s compares on the bit planes of the whole matrix and would count the fillers under the validity mask: not available "
                         "while a mask is set (reo_set_valid_mask(NULL) clears it)", what);
}

}  // namespace reo
