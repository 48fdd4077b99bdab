// Label-permutation null of a gene's best partner score (reo_top_partners_null): is the best partner that reo_top_partners lists for a query
// gene better than the best partner that meaningless labels produce for the same gene?  Per label row b and query row r (gene q), the max
// over the eligible partners p of |N_b(q, p)|, the smallest p that attains it, and how many partners reach the row's cut -- the single-step
// maxT null over a gene's partners.  The product of two earlier pieces: the lt / le words of (query, partner, block of 32 sample slots) do
// not depend on the labels, so one borrow chain serves kPermQ permutations (top_pairs_null.h); and the rows are query genes that meet every
// column (top_partners.h).  What the kernel of toppartnersnull.hip, the entry point of queries.hip and a host driver of the tests share, so
// that the driver can evaluate the very same functions under the sanitizers (tests/top_partners_null_driver.cpp): the reduction key and its
// unpacking, the eligibility rule, the limits, the batch rule and every argument check with its message.  No HIP header in here: plain
// C++17 (the kernels' unit defines the function attributes through pair_list.h).
//
// A label row is top_pairs_null.h's (tn_check_row): the side sizes, and with them 2 S_A S_B, hold under every row.
//
// The reduction key of partner p in a (label row, query row) cell puts "larger |N| first, then the smaller p" into one unsigned number of 63
// bits, larger = better:
//     |N| (31 bits, bits 32 .. 62)   2^32 - 1 - p (32 bits, bits 0 .. 31)
// |N| < 2^31 and p <= 65534: no partner has the key 0, which therefore stands for "no partner".  The rank shift Gamma of top_partners.h is
// NOT a tie-break here: it depends on the labels and would need a D per permutation.
#pragma once

#include <cstdint>
#include <cstdio>
#include <vector>

#include "top_pairs_null.h"
#include "top_partners.h"

namespace reo {

constexpr int64_t kTprnMaxPerms = int64_t(1) << 20;   // label rows per call
constexpr int64_t kTprnMaxGenes = int64_t(1) << 20;   // query genes per call
constexpr int64_t kTprnMaxCells = int64_t(1) << 26;   // n_perm * n_genes: the caller's arrays
constexpr int64_t kTprnBatchCap = 64;                 // most permutations of one launch (a multiple of kPermQ)
constexpr int64_t kTprnCellBytes = 12;                // device bytes per (permutation, padded query row): a 64-bit key and a 32-bit counter
static_assert(kTprnBatchCap % kPermQ == 0, "a full batch is whole launch groups");

// The key of partner p < G <= 65535 from |N| < 2^31; never 0.
REO_PL_FN uint64_t tprn_key(uint64_t abs_n, int p) { return (abs_n << 32) | (0xFFFFFFFFu - static_cast<uint32_t>(p)); }

// The outputs of one cell from its reduced key: key 0 (no eligible partner) gives -1, -1.
REO_PL_FN void tprn_unpack(uint64_t key, int64_t *max_n, int32_t *p)
{
    if (key == 0) { *max_n = -1; *p = -1; return; }
    *max_n = static_cast<int64_t>(key >> 32);
    *p = static_cast<int32_t>(0xFFFFFFFFu - static_cast<uint32_t>(key));
}

// The eligibility of column p in the row of q is top_partners.h's.
REO_PL_FN bool tprn_eligible(int32_t p, int32_t q, int G, const uint32_t *maskbits) { return tpr_eligible(p, q, G, maskbits); }

// The cut of a row as the kernel compares it: |N| < 2^31, so a cut of 2^31 or more is 0xFFFFFFFF, which no partner reaches.
REO_PL_FN uint32_t tprn_cut_word(int64_t cut) { return cut < (int64_t(1) << 31) ? static_cast<uint32_t>(cut) : 0xFFFFFFFFu; }

// Query rows of the device arrays: the queries padded with gene 0 up to a multiple of kTnRows.
REO_PL_FN int64_t tprn_padded_rows(int64_t n) { return (n + kTnRows - 1) / kTnRows * kTnRows; }

// Permutations per launch: at most kTprnBatchCap, n_perm and `env_cap` (REO_TOP_PARTNERS_NULL_BATCH; <= 0: none), few enough that the keys
// and counters of a batch stay within kTprBudget and the free memory, a multiple of kPermQ when above it, never below 1.
inline int64_t tprn_batch(int64_t n_perm, int64_t n_genes, uint64_t free_bytes, int64_t env_cap)
{
    int64_t p = kTprnBatchCap;
    if (env_cap > 0 && p > env_cap) p = env_cap;
    if (p > n_perm) p = n_perm;
    const uint64_t budget = free_bytes < static_cast<uint64_t>(kTprBudget) ? free_bytes : static_cast<uint64_t>(kTprBudget);
    const int64_t fit = static_cast<int64_t>(budget / static_cast<uint64_t>(kTprnCellBytes * tprn_padded_rows(n_genes)));
    if (p > fit) p = fit;
    if (p > kPermQ) p = p / kPermQ * kPermQ;
    return p < 1 ? 1 : p;
}

// Every argument check of reo_top_partners_null, on HOST arrays, before anything is uploaded.  group_id: the S labels of the context (read
// only behind tp_check_context).  0 when in order -- *s_a, *s_b then hold the sides' sizes --, otherwise the number of the failed check
// (1 .. 8: tp_check_context's).
inline int tprn_check_args(const TpState &st, const int32_t *group_id, int32_t a, int32_t b, const uint8_t *sides, int64_t n_perm,
                           const int32_t *genes, int64_t n_genes, const uint8_t *partner_mask, const int64_t *cuts, const int64_t *max_n,
                           const int32_t *arg_p, const int32_t *n_reach, int64_t *s_a, int64_t *s_b, char *msg, size_t msg_n)
{
    const char *what = "reo_top_partners_null";
    const int rc = tp_check_context(what, st, a, b, msg, msg_n);
    if (rc) return rc;
    if (n_perm < 1 || n_perm > kTprnMaxPerms) {
        snprintf(msg, msg_n, "%s: n_perm = %lld, between 1 and 2^20 permutations per call", what, (long long)n_perm);
        return 9;
    }
    if (n_genes < 1 || n_genes > kTprnMaxGenes) {
        snprintf(msg, msg_n, "%s: n_genes = %lld, between 1 and 2^20 query genes per call", what, (long long)n_genes);
        return 10;
    }
    if (n_perm * n_genes > kTprnMaxCells) {
        snprintf(msg, msg_n, "%s: n_perm * n_genes = %lld x %lld, at most 2^26 cells per call", what, (long long)n_perm, (long long)n_genes);
        return 11;
    }
    if (!sides || !genes || !max_n || !arg_p) {
        snprintf(msg, msg_n, "%s: sides, genes, max_n and arg_p must not be null", what);
        return 12;
    }
    if ((cuts == nullptr) != (n_reach == nullptr)) {
        snprintf(msg, msg_n, "%s: %s is null and %s is not: n_reach is null exactly when cuts is", what, cuts ? "n_reach" : "cuts",
                 cuts ? "cuts" : "n_reach");
        return 13;
    }
    for (int64_t q = 0; q < n_genes; ++q)
        if (genes[q] < 0 || genes[q] >= st.G) {
            snprintf(msg, msg_n, "%s: genes[%lld] = %d is outside the genes [0, %lld) (column %lld of the answer)", what, (long long)q, genes[q],
                     (long long)st.G, (long long)q);
            return 14;
        }
    for (int64_t q = 0; cuts && q < n_genes; ++q)
        if (cuts[q] < 0) { snprintf(msg, msg_n, "%s: cuts[%lld] = %lld, a cut of |N| is not negative", what, (long long)q, (long long)cuts[q]); return 15; }
    if (!group_id) { snprintf(msg, msg_n, "%s: no group labels", what); return 16; }
    std::vector<uint8_t> obs(static_cast<size_t>(st.S));
    int64_t na = 0, nb = 0;
    for (int64_t s = 0; s < st.S; ++s) {
        const uint8_t v = tn_column_byte(group_id[s], a, b, st.ngroups);
        obs[static_cast<size_t>(s)] = v;
        na += v == 1;
        nb += v == 0;
    }
    if (na < 1 || nb < 1) {
        snprintf(msg, msg_n, "%s: side A has %lld samples and side B %lld, both sides need at least one", what, (long long)na, (long long)nb);
        return 17;
    }
    for (int64_t p = 0; p < n_perm; ++p) {
        int64_t at = 0, got = 0;
        const int rr = tn_check_row(sides + p * st.S, obs.data(), st.S, na, &at, &got);
        if (rr == 1) {
            snprintf(msg, msg_n, "%s: row %lld of sides holds the byte %lld in column %lld (1 = side A, 0 = side B, 2 = takes no part)", what,
                     (long long)p, (long long)got, (long long)at);
            return 18;
        }
        if (rr == 2) {
            snprintf(msg, msg_n, "%s: row %lld of sides holds the byte %lld in column %lld, whose sample is on %s (a 2 marks exactly the samples of "
                                 "groups on neither side)", what, (long long)p, (long long)got, (long long)at,
                     obs[static_cast<size_t>(at)] == 2 ? "neither side" : "one of the sides");
            return 19;
        }
        if (rr == 3) {
            snprintf(msg, msg_n, "%s: row %lld of sides has %lld ones and %lld zeros, side A has %lld samples and side B %lld (a permutation keeps "
                                 "the sizes)", what, (long long)p, (long long)got, (long long)(na + nb - got), (long long)na, (long long)nb);
            return 20;
        }
    }
    for (int64_t g = 0; partner_mask && g < st.G; ++g)
        if (partner_mask[g] > 1) {
            snprintf(msg, msg_n, "%s: partner_mask[%lld] = %d, a byte of the mask is 0 or 1", what, (long long)g, (int)partner_mask[g]);
            return 21;
        }
    *s_a = na; *s_b = nb;
    return 0;
}

}  // namespace reo
