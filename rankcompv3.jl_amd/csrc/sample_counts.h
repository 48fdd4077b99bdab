// Sample counts (reo_sample_counts): in WHICH samples a gene's selected pairs show "gene i above its partner".  What the kernel of
// samplecounts.hip and a host driver share, so that the driver can evaluate the very same functions under the sanitizers
// (tests/sample_counts_driver.cpp): the lane-local vertical counters (bit planes c_0, c_1, ... over 32 sample bits), their expansion to
// per-sample counts, the number of planes that n additions need, the slot -> column map of the sample slots, and the argument checks that
// need no GPU.  No HIP header in here: plain C++17 (the kernel's unit defines the function attributes through pair_list.h).
//
// The comparison itself is the borrow chain of k1_counts over the pos / lo / hi planes (band_chain.h); it yields, for one partner and one
// block of 32 sample slots, a word `lt` (bit s: x_i > x_j and not tied in slot s) and a word `le` (bit s: greater or tied).  A lane adds the
// words of its partners into vertical counters: plane k holds bit k of the 32 running counts.
#pragma once

#include <cstdint>
#include <cstdio>
#include <vector>

#include "pair_list.h"

namespace reo {

constexpr int kScTileCols = 4096;                   // table columns per tile: the partner list of a tile lives in LDS (2 bytes per entry)
constexpr int kScTileWords = kScTileCols / 32;
constexpr int kScLanes = 64;
constexpr int kScMaxPlanes = 7;                     // a lane takes at most kScTileCols / kScLanes = 64 partners per tile: counts 0 .. 64
constexpr int kScChunkBlocks = 8;                   // sample blocks (of 32 slots) per workgroup: two for each of its four waves
constexpr int64_t kScMaxQueries = int64_t(1) << 30;
// The budget: bytes of EACH of the two device count buffers (batch x padded slots x 4); the queries of a call go in batches of
// as many rows as fit (at least one: 2^20 samples in 33 groups are 4.2 MB a row)
constexpr int64_t kScBudgetBytes = int64_t(32) << 20;

// Planes that a vertical counter needs after n additions of one-bit words: the bits of n (0 for n = 0).
REO_PL_FN int sc_counter_planes(int n)
{
    int p = 0;
    while (n > 0) { ++p; n >>= 1; }
    return p;
}

// c += w, per sample bit: a ripple of half adders over planes 0 .. planes - 1.  The caller sizes `planes` with sc_counter_planes for the
// number of additions it makes, so no carry leaves the last plane.
REO_PL_FN void sc_counter_add(uint32_t *c, int planes, uint32_t w)
{
    for (int k = 0; k < planes; ++k) {
        const uint32_t carry = c[k] & w;
        c[k] ^= w;
        w = carry;
    }
}

// The count of sample bit s held by the planes.
REO_PL_FN uint32_t sc_counter_at(const uint32_t *c, int planes, int s)
{
    uint32_t n = 0;
    for (int k = 0; k < planes; ++k) n += ((c[k] >> s) & 1u) << k;
    return n;
}

// The planes expanded to 32 counts.
REO_PL_FN void sc_counter_expand(const uint32_t *c, int planes, uint32_t *count /* 32 */)
{
    for (int s = 0; s < 32; ++s) count[s] = sc_counter_at(c, planes, s);
}

// Batch of queries whose count rows (padded slots x 4 bytes each) fit the budget; `env` = REO_SAMPLE_COUNTS_BATCH in queries (tests), which
// can only lower it; <= 0: none.
inline int64_t sc_batch_rows(int64_t n_genes, int64_t padded_slots, int64_t env)
{
    int64_t b = kScBudgetBytes / (padded_slots * 4);
    if (b < 1) b = 1;
    if (env > 0 && env < b) b = env;
    return b < n_genes ? b : n_genes;
}

// The sample slots of the bit planes (transform.hip): the groups in order, each padded to whole blocks of 32 slots, the samples of a group in
// column order.  map[slot] = the caller's column of that slot, -1 for a padding slot; returns false (map untouched) on a label outside
// [0, ngroups).  map.size() / 32 = the sample blocks.
inline bool sc_slot_map(const int32_t *group_id, int64_t S, int ngroups, std::vector<int32_t> &map)
{
    if (ngroups < 1 || S < 0) return false;
    std::vector<int64_t> off(static_cast<size_t>(ngroups) + 1, 0);
    for (int64_t s = 0; s < S; ++s) {
        if (group_id[s] < 0 || group_id[s] >= ngroups) return false;
        ++off[group_id[s] + 1];
    }
    for (int g = 0; g < ngroups; ++g) off[g + 1] = off[g] + (off[g + 1] + 31) / 32 * 32;
    map.assign(static_cast<size_t>(off[ngroups]), -1);
    std::vector<int64_t> at(off.begin(), off.end() - 1);
    for (int64_t s = 0; s < S; ++s) map[static_cast<size_t>(at[group_id[s]]++)] = static_cast<int32_t>(s);
    return true;
}

// Argument checks of reo_sample_counts that need neither the context's state nor the GPU.  0 when everything is in order; otherwise the
// number of the failed check (1 ..) and its message in msg.  genes is a HOST array.
inline int sample_counts_check_args(int64_t G, const int32_t *genes, int64_t n_genes, uint32_t class_mask, const int32_t *n_gt, char *msg,
                                    size_t msg_n)
{
    if (!genes || !n_gt) { snprintf(msg, msg_n, "reo_sample_counts: genes and n_gt must not be null"); return 1; }
    if (n_genes < 1 || n_genes > kScMaxQueries) {
        snprintf(msg, msg_n, "reo_sample_counts: n_genes = %lld, between 1 and 2^30 query genes per call", (long long)n_genes);
        return 2;
    }
    if (!query_class_mask_ok("reo_sample_counts", class_mask, msg, msg_n)) return 3;
    return query_genes_in_range("reo_sample_counts", G, genes, n_genes, msg, msg_n) ? 0 : 4;
}

}  // namespace reo
