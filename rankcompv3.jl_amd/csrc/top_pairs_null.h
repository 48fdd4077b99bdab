// Label-permutation null of the best pair score (reo_top_pairs_null): is the winning score of reo_top_pairs larger than the best score that
// meaningless labels produce?  Per permutation p, max over the eligible pairs i < j of |N_p(i, j)|, the pair that attains it, and how many
// pairs reach each of a few cuts -- the single-step maxT null of Geman's top-scoring pair.  The lt / le words of a pair and a block of 32
// sample slots do not depend on the labels (perm_null.h), so one borrow chain serves kPermQ permutations; N is that of top_pairs.h.  What the
// kernels of toppairsnull.hip, the entry point of queries.hip and a host driver of the tests share, so that the driver can evaluate the very
// same functions under the sanitizers (tests/top_pairs_null_driver.cpp): the check of a label row, the packing of the A-word (perm_null.h's)
// and of the live word that leaves out the samples of neither side, the reduction key and its unpacking, the batch rule and every argument
// check with its message.  No HIP header in here: plain C++17 (the kernels' unit defines the function attributes through pair_list.h).
//
// A label row: S bytes in the caller's column order, 1 = side A, 0 = side B, 2 = takes no part; exactly S_A ones and S_B zeros, and a 2
// exactly on the samples of the groups on neither side of (a, b) -- the same columns in every row, so the live word of a block is shared by
// all permutations, and the sizes, and with them 2 S_A S_B, hold under every permutation.
//
// The reduction key of a pair puts "larger |N| first, then the smaller (i, j)" into one unsigned number of 63 bits, larger = better:
//     |N| (31 bits, bits 32 .. 62)   2^32 - 1 - (i G + j) (32 bits, bits 0 .. 31)
// |N| < 2^31 and i G + j < 2^32 - 1 at G <= 65535: no pair has the key 0, which therefore stands for "no pair".  The rank shift Gamma of
// top_pairs.h is NOT a tie-break here: it depends on the labels and would need a D per permutation.
#pragma once

#include <cstdint>
#include <cstdio>
#include <vector>

#include "perm_null.h"
#include "top_pairs.h"

namespace reo {

constexpr int64_t kTnMaxPerms = int64_t(1) << 20;   // permutations per call
constexpr int kTnMaxCuts = 8;                       // cuts of |N| per call
constexpr int64_t kTnBatchCap = 64;                 // most permutations of one launch (a multiple of kPermQ); REO_TOP_NULL_BATCH asks for fewer
constexpr int kTnRows = 4;                          // rows that one wave of k_top_pairs_null walks with a column's planes in registers
static_assert(kTnBatchCap % kPermQ == 0, "a full batch is whole launch groups");

// The byte that every label row holds in the column of a sample of group g: 1 side A, 0 side B, 2 neither (b = -1: every other sample is B).
REO_PL_FN uint8_t tn_column_byte(int32_t g, int32_t a, int32_t b, int32_t ngroups)
{
    if (g < 0 || g >= ngroups) return 2;
    if (g == a) return 1;
    return (b < 0 || g == b) ? 0 : 2;
}

// A label row against the observed labels `obs` (S bytes of tn_column_byte).  0 in order; 1 a byte above 2 (*at: its column, *got: the
// byte); 2 a 2 where the sample is on a side, or none where it is on neither (*at: the column, *got: the byte); 3 another number of ones
// than side A has samples (*got: the count).  Behind 2 the ones and zeros together are S_A + S_B: the zeros are right when the ones are.
REO_PL_FN int tn_check_row(const uint8_t *row, const uint8_t *obs, int64_t S, int64_t s_a, int64_t *at, int64_t *got)
{
    int64_t ones = 0;
    for (int64_t s = 0; s < S; ++s) {
        if (row[s] > 2) { *at = s; *got = row[s]; return 1; }
        ones += row[s] == 1;
    }
    for (int64_t s = 0; s < S; ++s)
        if ((row[s] == 2) != (obs[s] == 2)) { *at = s; *got = row[s]; return 2; }
    if (ones != s_a) { *at = -1; *got = ones; return 3; }
    return 0;
}

// The live word of one block of 32 sample slots: bit s = the slot has a column and the row's byte there is not 2 (pn_live_word without the
// samples of neither side).  Every row of a call gives the same word.
REO_PL_FN uint32_t tn_live_word(const uint8_t *row /* S */, int64_t S, const int32_t *slot2col /* 32 */)
{
    uint32_t w = 0;
    for (int s = 0; s < 32; ++s) {
        const int64_t col = slot2col[s];
        if (col >= 0 && col < S && row[col] != 2) w |= 1u << s;
    }
    return w;
}

// The key of the pair (i, j), i < j < G <= 65535, from |N| < 2^31; never 0.
REO_PL_FN uint64_t tn_key(uint64_t abs_n, int i, int j, int G)
{
    return (abs_n << 32) | (0xFFFFFFFFu - (static_cast<uint32_t>(i) * static_cast<uint32_t>(G) + static_cast<uint32_t>(j)));
}

// The outputs of one permutation from its reduced key: key 0 (no eligible pair) gives -1, -1, -1.
REO_PL_FN void tn_unpack(uint64_t key, int G, int64_t *max_n, int32_t *i, int32_t *j)
{
    if (key == 0) { *max_n = -1; *i = -1; *j = -1; return; }
    const uint32_t idx = 0xFFFFFFFFu - static_cast<uint32_t>(key);
    *max_n = static_cast<int64_t>(key >> 32);
    *i = static_cast<int32_t>(idx / static_cast<uint32_t>(G));
    *j = static_cast<int32_t>(idx % static_cast<uint32_t>(G));
}

// Permutations per launch: at most kTnBatchCap, n_perm and `env_cap` (REO_TOP_NULL_BATCH; <= 0: none).
inline int64_t tn_batch(int64_t n_perm, int64_t env_cap)
{
    int64_t p = kTnBatchCap;
    if (env_cap > 0 && p > env_cap) p = env_cap;
    if (p > n_perm) p = n_perm;
    return p;
}

// Every argument check of reo_top_pairs_null, on HOST arrays, before anything is uploaded.  group_id: the S labels of the context (read
// only behind tp_check_context).  0 when in order -- *s_a, *s_b then hold the sides' sizes --, otherwise the number of the failed check.
inline int tn_check_args(const TpState &st, const int32_t *group_id, int32_t a, int32_t b, const uint8_t *sides, int64_t n_perm,
                         const uint8_t *gene_mask, const int64_t *cuts, int32_t n_cuts, const int64_t *max_n, const int32_t *arg_i,
                         const int32_t *arg_j, const int64_t *n_reach, int64_t *s_a, int64_t *s_b, char *msg, size_t msg_n)
{
    const char *what = "reo_top_pairs_null";
    const int rc = tp_check_context(what, st, a, b, msg, msg_n);
    if (rc) return rc;
    if (n_perm < 1 || n_perm > kTnMaxPerms) {
        snprintf(msg, msg_n, "%s: n_perm = %lld, between 1 and 2^20 permutations per call", what, (long long)n_perm);
        return 9;
    }
    if (n_cuts < 0 || n_cuts > kTnMaxCuts) { snprintf(msg, msg_n, "%s: n_cuts = %d, between 0 and 8 cuts per call", what, n_cuts); return 10; }
    if (!sides || !max_n || !arg_i || !arg_j || (n_cuts > 0 && (!cuts || !n_reach))) {
        snprintf(msg, msg_n, "%s: sides, max_n, arg_i and arg_j must not be null, nor cuts and n_reach with n_cuts = %d", what, n_cuts);
        return 11;
    }
    for (int t = 0; t < n_cuts; ++t)
        if (cuts[t] < 0) { snprintf(msg, msg_n, "%s: cuts[%d] = %lld, a cut of |N| is not negative", what, t, (long long)cuts[t]); return 12; }
    if (!group_id) { snprintf(msg, msg_n, "%s: no group labels", what); return 13; }
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
        return 14;
    }
    for (int64_t p = 0; p < n_perm; ++p) {
        int64_t at = 0, got = 0;
        const int rr = tn_check_row(sides + p * st.S, obs.data(), st.S, na, &at, &got);
        if (rr == 1) {
            snprintf(msg, msg_n, "%s: row %lld of sides holds the byte %lld in column %lld (1 = side A, 0 = side B, 2 = takes no part)", what,
                     (long long)p, (long long)got, (long long)at);
            return 15;
        }
        if (rr == 2) {
            snprintf(msg, msg_n, "%s: row %lld of sides holds the byte %lld in column %lld, whose sample is on %s (a 2 marks exactly the samples of "
                                 "groups on neither side)", what, (long long)p, (long long)got, (long long)at,
                     obs[static_cast<size_t>(at)] == 2 ? "neither side" : "one of the sides");
            return 16;
        }
        if (rr == 3) {
            snprintf(msg, msg_n, "%s: row %lld of sides has %lld ones and %lld zeros, side A has %lld samples and side B %lld (a permutation keeps "
                                 "the sizes)", what, (long long)p, (long long)got, (long long)(na + nb - got), (long long)na, (long long)nb);
            return 17;
        }
    }
    for (int64_t g = 0; gene_mask && g < st.G; ++g)
        if (gene_mask[g] > 1) {
            snprintf(msg, msg_n, "%s: gene_mask[%lld] = %d, a byte of the mask is 0 or 1", what, (long long)g, (int)gene_mask[g]);
            return 18;
        }
    *s_a = na; *s_b = nb;
    return 0;
}

}  // namespace reo
