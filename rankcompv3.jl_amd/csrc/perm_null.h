// Label-permutation null (reo_perm_null, reo_perm_codes): the class table of comparison k under shuffled sample labels, and what a pass over
// it says of every gene.  A permutation is a row of S bytes in the caller's column order, 1 = side A, with exactly n1 ones (n1 = the size
// of group k); side B is every other sample.  The sample ranks do not depend on the labels, so the bit planes stay where they are and the
// lt / le words of a pair and a block of 32 sample slots are the same under every permutation: a permutation only says which of their bits
// count for which side, as one A-word per block.  What the kernels of permpairs.hip, the entry points of api.hip and a host driver
// share, so that the driver can evaluate the very same functions under the sanitizers (tests/perm_null_driver.cpp): the packing of an
// A-word and of a live word, the check of a label row, the exceed rule, the batch width and the argument checks -- all of which run on
// the host before anything is touched.  No HIP header in here: plain C++17 (the kernels' unit defines the function attributes through
// pair_list.h).
//
// Semantics, for permutation p and the unordered pair i < j:  a = n_gt_A + tie_wins(seed, i, j, 0, n_eq_A),
// b = n_gt_B + tie_wins(seed, i, j, 1, n_eq_B) -- the coin of tie_coin.h keyed by side 0 and side 1, never by the context's group ids --,
// ic = mp_side_class(a, n1, m1, 0), it = mp_side_class(b, n2, m2, 0) with the context's thresholds m1 = thr[0, k], m2 = thr[1, k] (the
// sizes are kept, so they hold unchanged), code 3 (ic - 1) + (it - 1), and 8 minus it for (j, i).  The table of permutation p therefore
// equals, byte for byte and ties included, the reo_build_pairs(0) table of a two-group context with the same seed and group ids 1 - row.
// With a context of more than two groups the permuted tables are still two-group tables, one coin stream per side.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "masked_pairs.h"

namespace reo {

constexpr int kPermQ = 16;             // permutations that one launch group of k_pairs_permuted classifies from one borrow chain
constexpr int kPermRows = 4;           // table rows that one wave of k_pairs_permuted walks with a column's planes in registers
constexpr int64_t kPermBatchCap = 64;  // most tables of one batch (a multiple of kPermQ); REO_PERM_BATCH in the environment asks for fewer
constexpr int64_t kPermMaxPerms = int64_t(1) << 24;
static_assert(kPermBatchCap % kPermQ == 0, "a full batch is whole launch groups");

// A label row: S bytes, each 0 or 1, exactly n1 ones.  0 in order; 1 a byte other than 0 / 1 (*at: its column, *got: the byte); 2 another
// number of ones (*got: the count).
REO_PL_FN int pn_check_row(const uint8_t *row, int64_t S, int64_t n1, int64_t *at, int64_t *got)
{
    int64_t ones = 0;
    for (int64_t s = 0; s < S; ++s) {
        if (row[s] > 1) { *at = s; *got = row[s]; return 1; }
        ones += row[s];
    }
    if (ones != n1) { *at = -1; *got = ones; return 2; }
    return 0;
}

// The live word of one block of 32 sample slots: bit s = the slot has a column (slot2col: the caller's column of every slot of the block,
// -1 for padding).
REO_PL_FN uint32_t pn_live_word(int64_t S, const int32_t *slot2col /* 32 */)
{
    uint32_t w = 0;
    for (int s = 0; s < 32; ++s)
        if (slot2col[s] >= 0 && slot2col[s] < S) w |= 1u << s;
    return w;
}

// The A-word of one permutation and block: bit s = the slot's column is on side A.  Padding slots give 0: A is a subset of live.
REO_PL_FN uint32_t pn_side_word(const uint8_t *row /* S */, int64_t S, const int32_t *slot2col /* 32 */)
{
    uint32_t w = 0;
    for (int s = 0; s < 32; ++s) {
        const int64_t col = slot2col[s];
        if (col >= 0 && col < S && row[col] == 1) w |= 1u << s;
    }
    return w;
}

// Where the A-word of permutation p and block b lies: [launch group p / kPermQ][block][p % kPermQ], so that the kPermQ words a wave needs
// per block are one run of memory.  Rows past n_perm inside the last group stay 0 (the caller clears the buffer).
REO_PL_FN size_t pn_word_index(int64_t p, int64_t b, int64_t nblk)
{
    return (static_cast<size_t>(p / kPermQ) * static_cast<size_t>(nblk) + static_cast<size_t>(b)) * kPermQ + static_cast<size_t>(p % kPermQ);
}
REO_PL_FN size_t pn_word_count(int64_t n_perm, int64_t nblk)
{
    return static_cast<size_t>((n_perm + kPermQ - 1) / kPermQ) * static_cast<size_t>(nblk) * kPermQ;
}

// The exceed rule of n_ge: the permutation's |delta1| reaches the observed one, compared as doubles.  Equality counts (so does 0 against 0:
// a gene that never moves has p_perm = 1); a NaN on either side does not.
REO_PL_FN bool pn_exceeds(double d_perm, double d_obs) { return std::fabs(d_perm) >= std::fabs(d_obs); }

// Tables per batch: as many as fit half of the free device memory, at most kPermBatchCap, n_perm and `env_cap` (REO_PERM_BATCH; <= 0:
// none); 0 when not even one fits.
inline int64_t pn_batch_tables(uint64_t free_bytes, uint64_t table_bytes, int64_t n_perm, int64_t env_cap)
{
    if (table_bytes == 0 || table_bytes > free_bytes) return 0;
    int64_t p = static_cast<int64_t>(free_bytes / 2 / table_bytes);
    if (p < 1) p = 1;
    if (p > kPermBatchCap) p = kPermBatchCap;
    if (env_cap > 0 && p > env_cap) p = env_cap;
    if (p > n_perm) p = n_perm;
    return p;
}

// What the checks need to know of the context.
struct PnState {
    bool multi;           // a reo_create_multi context (leader or peer)
    int32_t world;        // reo_set_shard
    int64_t G, S;         // the resident matrix (0 x 0: none)
    int32_t ngroups;      // 0: no groups
    int64_t n_labels;     // labels of reo_set_groups
    bool has_mask;        // a validity mask is set
    bool thr_set;         // thresholds set
    int32_t built_k;      // comparison of the resident class table (-1: none)
    bool plain_table;     // ... built by reo_build_pairs (no contrast, no mask) and complete
};

// What reo_perm_null and reo_perm_codes share (what = the call's name; need_table: the resident table of k is read).  0 when everything is
// in order; otherwise the number of the failed check (1 ..) and its message.
inline int pn_check_context(const char *what, const PnState &st, int32_t k, bool need_table, char *msg, size_t msg_n)
{
    if (st.multi) { snprintf(msg, msg_n, "%s is not available on a reo_create_multi context (the permuted tables live on one device)", what); return 1; }
    if (st.world > 1) {
        snprintf(msg, msg_n, "%s is not available on a sharded context (reo_set_shard: %d shards; the permuted build has no exchange)", what, st.world);
        return 2;
    }
    if (st.G < 1 || st.S < 1 || st.ngroups < 2 || st.n_labels != st.S) {
        snprintf(msg, msg_n, "%s: no expression matrix with group labels of its width is set", what);
        return 3;
    }
    if (st.has_mask) {
        snprintf(msg, msg_n, "%s compares on the bit planes of the whole matrix and would count the fillers under the validity mask: not available "
                             "while a mask is set (reo_set_valid_mask(NULL) clears it)", what);
        return 4;
    }
    if (st.S > kMpMaxSamples) { snprintf(msg, msg_n, "%s: S = %lld, at most 65535 samples", what, (long long)st.S); return 5; }
    if (st.G > kMpMaxGenes) { snprintf(msg, msg_n, "%s: G = %lld, at most 65535 genes (the 16-plane layout only)", what, (long long)st.G); return 6; }
    if (k < 0 || k >= st.ngroups) { snprintf(msg, msg_n, "%s: comparison %d outside [0,%d)", what, k, st.ngroups); return 7; }
    if (!st.thr_set) { snprintf(msg, msg_n, "%s: thresholds not set (reo_compute_thresholds)", what); return 8; }
    if (need_table && (st.built_k != k || !st.plain_table)) {
        snprintf(msg, msg_n, "%s: no class table of comparison %d is resident (call reo_build_pairs(%d) first; a contrast or masked table does not count)",
                 what, k, k);
        return 9;
    }
    return 0;
}

// The label rows of a call: n_perm rows of S bytes, every one checked before anything is touched.
inline int pn_check_rows(const char *what, const uint8_t *side_a, int64_t n_perm, int64_t S, int64_t n1, char *msg, size_t msg_n)
{
    if (!side_a) { snprintf(msg, msg_n, "%s: side_a must not be null", what); return 10; }
    if (n_perm < 1 || n_perm > kPermMaxPerms) { snprintf(msg, msg_n, "%s: n_perm = %lld, between 1 and 2^24 permutations per call", what, (long long)n_perm); return 11; }
    for (int64_t p = 0; p < n_perm; ++p) {
        int64_t at = 0, got = 0;
        const int rc = pn_check_row(side_a + p * S, S, n1, &at, &got);
        if (rc == 1) {
            snprintf(msg, msg_n, "%s: row %lld of side_a holds the byte %lld in column %lld (1 = side A, 0 = side B)", what, (long long)p, (long long)got,
                     (long long)at);
            return 12;
        }
        if (rc == 2) {
            snprintf(msg, msg_n, "%s: row %lld of side_a has %lld ones, side A of the comparison has %lld samples (a permutation keeps the sizes)", what,
                     (long long)p, (long long)got, (long long)n1);
            return 13;
        }
    }
    return 0;
}

inline int pn_check_null_args(const PnState &st, int32_t k, const uint8_t *side_a, int64_t n_perm, int64_t n1, const uint8_t *ref_mask,
                              double pval_deg, double padj_deg, const double *delta1_obs, const int32_t *n_ge, const int32_t *n_up,
                              const int32_t *n_down, const double *se_null, char *msg, size_t msg_n)
{
    const char *what = "reo_perm_null";
    if (!ref_mask || !delta1_obs || !n_ge || !n_up || !n_down || !se_null || !side_a) {
        snprintf(msg, msg_n, "%s: side_a, ref_mask, delta1_obs, n_ge, n_up, n_down and se_null must not be null (delta1_null may be)", what);
        return 10;
    }
    int rc = pn_check_context(what, st, k, true, msg, msg_n);
    if (rc) return rc;
    if ((rc = pn_check_rows(what, side_a, n_perm, st.S, n1, msg, msg_n))) return rc;
    if (!(pval_deg >= 0.0) || !(padj_deg >= 0.0)) { snprintf(msg, msg_n, "%s: pval_deg = %g, padj_deg = %g: neither may be negative or NaN", what, pval_deg, padj_deg); return 14; }
    return 0;
}

inline int pn_check_codes_args(const PnState &st, int32_t k, const uint8_t *side_a, int64_t n1, int64_t i0, int64_t i1, int64_t j0, int64_t j1,
                               const uint8_t *code, char *msg, size_t msg_n)
{
    const char *what = "reo_perm_codes";
    if (!code || !side_a) { snprintf(msg, msg_n, "%s: side_a and code must not be null", what); return 10; }
    int rc = pn_check_context(what, st, k, false, msg, msg_n);
    if (rc) return rc;
    if ((rc = pn_check_rows(what, side_a, 1, st.S, n1, msg, msg_n))) return rc;
    if (i0 < 0 || j0 < 0 || i1 > st.G || j1 > st.G || i0 >= i1 || j0 >= j1) {
        snprintf(msg, msg_n, "%s: bad pair block [%lld,%lld) x [%lld,%lld)", what, (long long)i0, (long long)i1, (long long)j0, (long long)j1);
        return 15;
    }
    return 0;
}

}  // namespace reo
