// Leave-one-out cross-validation of the k-TSP classifier (reo_top_pairs_loo): for every sample s of the two sides of a search, the greedy
// disjoint selection of top_pairs.h's order on the training set "both sides without s", and what the held-out sample shows on every pick.
// What the kernels of toppairsloo.hip, the entry point of queries.hip and a host driver of the tests share, so that the driver can evaluate
// the very same functions under the sanitizers (tests/top_pairs_loo_driver.cpp): the fold's counts, N and D, the held-out outcome, the
// comparison of two candidates inside a fold, the cut rule, the capacity rule and every argument check with its message.  No HIP header in
// here: plain C++17 (the kernels' unit defines the function attributes through pair_list.h).
//
// A fold: one sample s of side A or of side B.  Its sizes are (S_A - 1, S_B) or (S_A, S_B - 1); the counts of a pair in the fold are the
// full counts minus the sample's own bit (gt: gene_i above gene_j and not tied, eq: tied) on the sample's side; N(s) = tp_num of those;
// D(s)_g = tp_shift of the sums of lo + hi over the sides without the sample; Gamma(s) = |D(s)_i - D(s)_j|.  Inside the fold the pairs are
// ordered as top_pairs.h orders them: |N(s)| descending, Gamma(s) descending, i ascending, j ascending -- a total order, so the greedy
// walk "take a pair when neither gene is used, up to kmax pairs" does not depend on how the pairs are stored.
//
// Why a band of candidates holds every pick of every fold (the cut rule, loo_cut).  Let S_max = max(S_A, S_B).
//   (1) Removing one sample moves |N| of a pair by at most 2 S_max.  With w = gt - lt per side, N = w_A S_B - w_B S_A.  A sample of side A
//       changes w_A by at most 1 and S_A by 1: N(s) - N = -(+-1) S_B + w_B, and |w_B| <= S_B, so |N(s) - N| <= 2 S_B; a sample of side B
//       likewise moves N by at most 2 S_A.
//   (2) Let the greedy disjoint walk of the FULL-data order yield 2 kmax pairs, the last of them with |N| = v.  All of them have
//       |N| >= v, so in any fold they still have |N(s)| >= v - 2 S_max, and they are pairwise disjoint.
//   (3) A greedy pick uses two genes and therefore blocks at most two of those 2 kmax disjoint pairs.  In front of pick r <= kmax at most
//       2 (kmax - 1) of them are blocked: at least two are still free, so the pick -- the best free pair of the fold -- has
//       |N(s)| >= v - 2 S_max.
//   (4) A pair with full |N| < T = v - 4 S_max has |N(s)| <= T - 1 + 2 S_max = v - 2 S_max - 1: strictly less than any pick of (3).
//   So every pick of every fold has full |N| >= T, whatever Gamma says: it is a candidate.  When 2 kmax disjoint pairs do not exist within
//   the deepest list (2^20 pairs), T = 0 and every eligible pair is a candidate.
#pragma once

#include <cstdint>
#include <cstdio>
#include <vector>

#include "top_pairs.h"

namespace reo {

constexpr int kLooMaxK = 64;                               // picks per fold
constexpr int64_t kLooFirstWant = 1024;                    // step 1: the full-data list grows from here, doubling, up to kTpMaxWant
constexpr int64_t kLooMaxRecords = int64_t(1) << 26;       // candidates per call; REO_TOP_PAIRS_LOO_CAP can only lower it
constexpr int64_t kLooFirstRecords = int64_t(1) << 18;     // records of the first emit; the counter says how many a second one needs
constexpr int kLooThreads = 256;                           // threads of one fold's workgroup
constexpr int kLooUsedWords = 2048;                        // the used-gene bitmap of a fold: 65 536 bits

// The held-out sample's outcome of a pair from its two bits: +1 gene_i above gene_j, 0 tied, -1 below.
REO_PL_FN int loo_outcome(uint32_t gt_bit, uint32_t eq_bit) { return gt_bit ? 1 : (eq_bit ? 0 : -1); }

// N of a pair in the fold of a sample of side `side` (0 = A, 1 = B) that shows (gt_bit, eq_bit) on the pair; s_a, s_b: the FULL sizes.
REO_PL_FN int64_t loo_num(const TpRec &r, int side, uint32_t gt_bit, uint32_t eq_bit, int64_t s_a, int64_t s_b)
{
    const int32_t g = static_cast<int32_t>(gt_bit), e = static_cast<int32_t>(eq_bit);
    if (side == 0) return tp_num(r.gt_a - g, r.eq_a - e, r.gt_b, r.eq_b, s_a - 1, s_b);
    return tp_num(r.gt_a, r.eq_a, r.gt_b - g, r.eq_b - e, s_a, s_b - 1);
}

// D of a gene in that fold: sum_a, sum_b = the gene's sums of lo + hi over the full sides, v = its lo + hi in the held-out sample.
REO_PL_FN int64_t loo_shift(int64_t sum_a, int64_t sum_b, int side, int64_t v, int64_t s_a, int64_t s_b)
{
    if (side == 0) return tp_shift(sum_a - v, sum_b, s_a - 1, s_b);
    return tp_shift(sum_a, sum_b - v, s_a, s_b - 1);
}

// 2^32 - 1 - (i G + j): larger = the earlier pair; never 0 at G <= 65535.
REO_PL_FN uint32_t loo_index_key(int i, int j, int G)
{
    return 0xFFFFFFFFu - (static_cast<uint32_t>(i) * static_cast<uint32_t>(G) + static_cast<uint32_t>(j));
}

// Does the candidate (|N(s)| = nx, Gamma(s) = gx, index key kx) come before (ny, gy, ky) in the fold's order?
REO_PL_FN bool loo_before(uint64_t nx, uint64_t gx, uint32_t kx, uint64_t ny, uint64_t gy, uint32_t ky)
{
    if (nx != ny) return nx > ny;
    if (gx != gy) return gx > gy;
    return kx > ky;
}

// Where the words of candidate c and sample block b lie: [block][candidate], a fold reads consecutive candidates contiguously.
REO_PL_FN size_t loo_word_index(int b, uint32_t c, uint32_t n_cand) { return static_cast<size_t>(b) * n_cand + c; }

// The cut of the band (the argument in front): v = |N| of the last of the 2 kmax full-data disjoint pairs.
inline int64_t loo_cut(int64_t v, int64_t s_a, int64_t s_b)
{
    const int64_t t = v - 4 * (s_a > s_b ? s_a : s_b);
    return t > 0 ? t : 0;
}

// The greedy disjoint walk over a list in order: how many pairs it takes (at most `want`); *last = the list index of the last one taken.
inline int64_t loo_disjoint(const int32_t *gene_i, const int32_t *gene_j, int64_t n, int64_t G, int64_t want, int64_t *last)
{
    std::vector<uint8_t> used(static_cast<size_t>(G > 0 ? G : 0), 0);
    int64_t taken = 0;
    *last = -1;
    for (int64_t e = 0; e < n && taken < want; ++e) {
        const int32_t i = gene_i[e], j = gene_j[e];
        if (i < 0 || j < 0 || i >= G || j >= G || used[static_cast<size_t>(i)] || used[static_cast<size_t>(j)]) continue;
        used[static_cast<size_t>(i)] = used[static_cast<size_t>(j)] = 1;
        ++taken; *last = e;
    }
    return taken;
}

// Most candidate records of a call: 2^26; `env` = REO_TOP_PAIRS_LOO_CAP (tests) can only lower it; <= 0: none.
inline int64_t loo_capacity(int64_t env) { return env > 0 && env < kLooMaxRecords ? env : kLooMaxRecords; }
// Records of the first emit: 2^18, never above the cap; `env` = REO_TOP_PAIRS_LOO_FIRST (tests of the resize) can only lower it.
inline int64_t loo_first_records(int64_t cap, int64_t env)
{
    int64_t n = env > 0 && env < kLooFirstRecords ? env : kLooFirstRecords;
    return n < cap ? n : cap;
}
// Device bytes that n candidates need over `blocks` blocks of 32 sample slots: the records and two words per block.
inline int64_t loo_bytes(int64_t n, int64_t blocks) { return n * (static_cast<int64_t>(sizeof(TpRec)) + 8 * blocks); }

// 0 when n candidates can be held; otherwise the number of the check, with the count and the cut in the message.
inline int loo_check_count(int64_t n, int64_t cut, int64_t cap, int64_t blocks, uint64_t free_bytes, char *msg, size_t msg_n)
{
    if (n > cap) {
        snprintf(msg, msg_n, "reo_top_pairs_loo: %lld pairs reach the cut |N| >= %lld, at most %lld candidate records per call (small sides move every "
                 "score by a large step: search fewer genes through gene_mask)", (long long)n, (long long)cut, (long long)cap);
        return 1;
    }
    if (static_cast<uint64_t>(loo_bytes(n, blocks)) > free_bytes) {
        snprintf(msg, msg_n, "reo_top_pairs_loo: %lld pairs reach the cut |N| >= %lld and need %lld bytes of device memory, %llu are free", (long long)n,
                 (long long)cut, (long long)loo_bytes(n, blocks), (unsigned long long)free_bytes);
        return 2;
    }
    return 0;
}

// Every argument check of reo_top_pairs_loo, on HOST arrays, before anything is uploaded.  0 when in order, otherwise the number of the
// failed check (1 .. 8: tp_check_context's).
inline int loo_check_args(const TpState &st, int32_t a, int32_t b, const uint8_t *gene_mask, int32_t kmax, const int32_t *gene_i,
                          const int32_t *gene_j, const int64_t *num, const int64_t *rank_num, const int8_t *outcome, const int8_t *side,
                          const int64_t *stats, char *msg, size_t msg_n)
{
    const int rc = tp_check_context("reo_top_pairs_loo", st, a, b, msg, msg_n);
    if (rc) return rc;
    if (kmax < 1 || kmax > kLooMaxK) {
        snprintf(msg, msg_n, "reo_top_pairs_loo: kmax = %d, between 1 and %d picks per fold", kmax, kLooMaxK);
        return 9;
    }
    if (!gene_i || !gene_j || !num || !rank_num || !outcome || !side || !stats) {
        snprintf(msg, msg_n, "reo_top_pairs_loo: gene_i, gene_j, num, rank_num, outcome, side and stats must not be null");
        return 10;
    }
    for (int64_t g = 0; gene_mask && g < st.G; ++g)
        if (gene_mask[g] > 1) {
            snprintf(msg, msg_n, "reo_top_pairs_loo: gene_mask[%lld] = %d, a byte of the mask is 0 or 1", (long long)g, (int)gene_mask[g]);
            return 11;
        }
    return 0;
}

// A fold leaves one sample out: each side needs two.
inline int loo_check_sides(int64_t s_a, int64_t s_b, char *msg, size_t msg_n)
{
    if (s_a < 2) { snprintf(msg, msg_n, "reo_top_pairs_loo: side A has %lld samples, a fold leaves one out: each side needs at least two", (long long)s_a); return 12; }
    if (s_b < 2) { snprintf(msg, msg_n, "reo_top_pairs_loo: side B has %lld samples, a fold leaves one out: each side needs at least two", (long long)s_b); return 13; }
    return 0;
}

}  // namespace reo
