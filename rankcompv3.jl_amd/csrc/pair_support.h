// Pair support (reo_pair_support): HOW STRONGLY a listed pair supports a call -- per group, in how many samples gene i lies above its partner
// j (and in how many the two are tied), and optionally the outcome of every single sample.  What the kernel of pairsupport.hip and a host
// driver share, so that the driver can evaluate the very same functions under the sanitizers (tests/pair_support_driver.cpp): the work items
// that a CSR of pairs is cut into, the batch of entries whose device buffers stay under the budget, the byte that an (lt, le) bit pair
// stands for, and the argument checks -- all of which run on the host before anything is uploaded.  No HIP header in here: plain C++17 (the
// kernel's unit defines the function attributes through pair_list.h).
//
// The comparison itself is the borrow chain of k1_counts over the pos / lo / hi planes (band_chain.h); it yields, for one pair and one block of
// 32 sample slots, a word `lt` (bit s: x_i > x_j and not tied in slot s) and a word `le` (bit s: greater or tied).
#pragma once

#include <cstdint>
#include <cstdio>
#include <vector>

#include "pair_list.h"

namespace reo {

constexpr int kPsLanes = 64;                        // entries per work item: one lane each
constexpr int64_t kPsMaxGenes = int64_t(1) << 30;   // rows per call
// The budget: bytes of EACH of the two device count buffers (batch x ngroups x 4) and of the outcome buffer (batch x S)
constexpr int64_t kPsBudgetBytes = int64_t(32) << 20;

// One wave's work: `count` (1 .. kPsLanes) consecutive entries of CSR row `row`, the first one at `first` counted from the batch's first
// entry; `gene` = genes[row], so that the kernel needs no second lookup.  16 bytes: one load.
struct PsItem {
    int32_t row, first, count, gene;
};

// Entries per batch: as many as keep every device buffer under the budget (at least one: 2^25 samples are a 32 MiB outcome row); `env` =
// REO_PAIR_SUPPORT_BATCH in entries (tests), which can only lower it; <= 0: none.  The count buffers alone hold it to budget / 4 = 2^23
// entries, so every offset inside a batch is far from the end of int32.
inline int64_t ps_batch_entries(int64_t total, int64_t ngroups, int64_t S, bool with_outcome, int64_t env)
{
    int64_t b = kPsBudgetBytes / ((ngroups < 1 ? 1 : ngroups) * 4);
    if (with_outcome && S > 0 && kPsBudgetBytes / S < b) b = kPsBudgetBytes / S;
    if (b < 1) b = 1;
    if (env > 0 && env < b) b = env;
    return b < total ? b : total;
}

// The work items of entries [e0, e1) of the CSR: every row's share of the range in pieces of at most kPsLanes consecutive entries, rows in
// order, empty rows give nothing.  *row_io: a row at or before the one that holds e0 on entry (0 for the first batch), the row that holds e1
// on return -- the batches of a call walk the rows once.  rowptr has passed pair_support_check_args (starts at 0, never decreases).
inline void ps_build_items(const int32_t *genes, const int64_t *rowptr, int64_t n_genes, int64_t e0, int64_t e1, int64_t *row_io,
                           std::vector<PsItem> &items)
{
    items.clear();
    int64_t q = *row_io;
    while (q < n_genes && rowptr[q + 1] <= e0) ++q;
    int64_t at = e0;
    while (at < e1 && q < n_genes) {
        const int64_t end = rowptr[q + 1] < e1 ? rowptr[q + 1] : e1;
        while (at < end) {
            const int64_t n = end - at < kPsLanes ? end - at : kPsLanes;
            items.push_back(PsItem{static_cast<int32_t>(q), static_cast<int32_t>(at - e0), static_cast<int32_t>(n), genes[q]});
            at += n;
        }
        if (at < e1) ++q;   // (the row is used up; at == e1 inside a row: the next batch goes on in it)
    }
    *row_io = q;
}

// The outcome byte of sample bit s: 0 (x_i < x_j), 1 (tied), 2 (x_i > x_j).  lt implies le, so the byte is the sum of the two bits.
REO_PL_FN uint8_t ps_outcome_byte(uint32_t lt, uint32_t le, int s)
{
    return static_cast<uint8_t>(((lt >> s) & 1u) + ((le >> s) & 1u));
}

// The 32 outcome bytes of a block.
REO_PL_FN void ps_outcome_expand(uint32_t lt, uint32_t le, uint8_t *out /* 32 */)
{
    for (int s = 0; s < 32; ++s) out[s] = ps_outcome_byte(lt, le, s);
}

// Argument checks of reo_pair_support: all of them, on HOST arrays, before anything is uploaded -- no address on the device is formed from
// an unchecked value.  0 when everything is in order; otherwise the number of the failed check (1 ..) and its message in msg.
inline int pair_support_check_args(int64_t G, const int32_t *genes, int64_t n_genes, const int64_t *rowptr, const int32_t *partner,
                                   const int32_t *n_gt, char *msg, size_t msg_n)
{
    if (!genes || !rowptr || !n_gt) { snprintf(msg, msg_n, "reo_pair_support: genes, rowptr and n_gt must not be null"); return 1; }
    if (n_genes < 1 || n_genes > kPsMaxGenes) {
        snprintf(msg, msg_n, "reo_pair_support: n_genes = %lld, between 1 and 2^30 rows per call", (long long)n_genes);
        return 2;
    }
    if (!query_genes_in_range("reo_pair_support", G, genes, n_genes, msg, msg_n)) return 3;
    if (rowptr[0] != 0) { snprintf(msg, msg_n, "reo_pair_support: rowptr[0] = %lld, a CSR starts at 0", (long long)rowptr[0]); return 4; }
    for (int64_t q = 0; q < n_genes; ++q)
        if (rowptr[q + 1] < rowptr[q]) {
            snprintf(msg, msg_n, "reo_pair_support: rowptr decreases at row %lld (%lld after %lld)", (long long)q, (long long)rowptr[q + 1],
                     (long long)rowptr[q]);
            return 4;
        }
    if (!partner && rowptr[n_genes] > 0) {
        snprintf(msg, msg_n, "reo_pair_support: partner is null and rowptr lists %lld entries", (long long)rowptr[n_genes]);
        return 5;
    }
    for (int64_t q = 0; q < n_genes; ++q)
        for (int64_t e = rowptr[q]; e < rowptr[q + 1]; ++e) {
            if (partner[e] < 0 || partner[e] >= G) {
                snprintf(msg, msg_n, "reo_pair_support: partner[%lld] = %d (row %lld) is outside [0, %lld)", (long long)e, partner[e], (long long)q,
                         (long long)G);
                return 6;
            }
            if (partner[e] == genes[q]) {
                snprintf(msg, msg_n, "reo_pair_support: partner[%lld] = %d is the gene of its own row %lld (the diagonal is no pair)", (long long)e,
                         partner[e], (long long)q);
                return 7;
            }
        }
    return 0;
}

}  // namespace reo
