// Top-scoring pairs (reo_top_pairs, reo_rank_shift): WHICH few gene pairs, out of all G (G - 1) / 2, separate two sides best -- the search of
// Geman's top-scoring pair and Tan's k-TSP.  What the kernels of toppairs.hip, the host driver of queries.hip and a host driver of the tests
// share, so that the test driver can evaluate the very same functions under the sanitizers (tests/top_pairs_driver.cpp): the key of a pair and
// its digits, the digit that holds the n-th key of a histogram, the tile-skip rule, N and Gamma from the counts and the rank shift, the final
// comparison, the pass loop of the selection and every argument check with its message.  No HIP header in here: plain C++17 (the kernels'
// unit defines the function attributes through pair_list.h).
//
// The score (include/reo_hip.h): per side, gt = samples with x_i above x_j and not tied, eq = tied samples, lt = S_side - gt - eq,
// w = gt - lt;  N = w(A) S_B - w(B) S_A (antisymmetric in (i, j)), score = |N| / (2 S_A S_B).  The rank shift of a gene is
// D_i = W_i(A) S_B - W_i(B) S_A with W_i(side) the sum over the side's samples of (genes below i) - (genes above i), and
// Gamma_ij = |D_i - D_j| breaks equal |N|.  The order over i < j: |N| descending, Gamma descending, i ascending, j ascending.
//
// The key of a pair puts that order into one unsigned number of 111 bits, larger = earlier:
//     |N| (31 bits, bits 80 .. 110)   Gamma (48 bits, bits 32 .. 79)   2^32 - 1 - (i G + j) (32 bits, bits 0 .. 31)
// No two pairs share a key.  The selection is a radix select over its ten 12-bit digits, most significant first, that RECOUNTS the pairs in
// every pass instead of storing a score per pair: a pass histograms the digit below the prefix chosen so far, the host picks the bin that
// holds the n-th key and extends the prefix; as soon as the keys above the prefix and the keys that share it fit the candidate buffer, one
// more pass emits them and the host sorts.
#pragma once

#include <cstdint>
#include <cstdio>

#include "masked_pairs.h"
#include "pair_list.h"

namespace reo {

constexpr int64_t kTpMaxGenes = 65535;               // the 16-plane layout only
constexpr int64_t kTpMaxSamples = 65535;
constexpr int64_t kTpMaxWant = int64_t(1) << 20;     // pairs per call
constexpr int64_t kTpMinCapacity = int64_t(1) << 18; // candidate records: max(4 n_want, this)
constexpr int kTpRows = 8;                           // rows that one wave of k_top_pairs walks with a column's planes in registers
constexpr int kTpWaves = 4;                          // waves per workgroup: four neighbouring column tiles of the same rows
constexpr int kTpDigitBits = 12;
constexpr int kTpBins = 1 << kTpDigitBits;           // bins of one pass
constexpr int kTpAbove = kTpBins, kTpBelow = kTpBins + 1;   // the two extra counters of a pass: keys above / below the prefix
constexpr int kTpHistWords = kTpBins + 2;
constexpr int kTpKeyBits = 120;                      // ten digits; the key itself has 111 bits
constexpr int kTpGammaBits = 48;

struct TpKey {
    uint64_t hi, lo;   // bits 64 .. 127, bits 0 .. 63
};

// One candidate as the emit pass stores it: the pair and its four counts (gt and eq of "gene_i above gene_j" per side).
struct TpRec {
    int32_t i, j, gt_a, eq_a, gt_b, eq_b;
};

REO_PL_FN int tp_cmp(const TpKey &x, const TpKey &y)
{
    if (x.hi != y.hi) return x.hi < y.hi ? -1 : 1;
    if (x.lo != y.lo) return x.lo < y.lo ? -1 : 1;
    return 0;
}

// key >> s, s in [0, 127]
REO_PL_FN TpKey tp_shr(const TpKey &k, int s)
{
    TpKey r;
    if (s == 0) { r = k; }
    else if (s < 64) { r.lo = (k.lo >> s) | (k.hi << (64 - s)); r.hi = k.hi >> s; }
    else if (s == 64) { r.lo = k.hi; r.hi = 0; }
    else { r.lo = k.hi >> (s - 64); r.hi = 0; }
    return r;
}

// (key << 12) | digit: the prefix one digit longer
REO_PL_FN TpKey tp_extend(const TpKey &k, uint32_t digit)
{
    TpKey r;
    r.hi = (k.hi << kTpDigitBits) | (k.lo >> (64 - kTpDigitBits));
    r.lo = (k.lo << kTpDigitBits) | digit;
    return r;
}

// The digit whose lowest bit is bit s of the key, and everything above that digit.
REO_PL_FN uint32_t tp_digit(const TpKey &k, int s) { return static_cast<uint32_t>(tp_shr(k, s).lo) & (kTpBins - 1); }
REO_PL_FN TpKey tp_top(const TpKey &k, int s) { return tp_shr(k, s + kTpDigitBits); }

// The key of the pair (i, j), i < j < G <= 65535, from |N| < 2^31 and Gamma < 2^48.
REO_PL_FN TpKey tp_pack(uint64_t abs_n, uint64_t gamma, int i, int j, int G)
{
    const uint32_t idx = 0xFFFFFFFFu - (static_cast<uint32_t>(i) * static_cast<uint32_t>(G) + static_cast<uint32_t>(j));
    TpKey k;
    k.hi = (abs_n << (kTpGammaBits - 32)) | (gamma >> 32);
    k.lo = (gamma << 32) | idx;
    return k;
}

// N of a pair from its four counts and the sides' sizes: w = gt - lt = 2 gt + eq - S per side.  |N| <= 2 S_A S_B.
REO_PL_FN int64_t tp_num(int32_t gt_a, int32_t eq_a, int32_t gt_b, int32_t eq_b, int64_t s_a, int64_t s_b)
{
    const int64_t wa = 2 * static_cast<int64_t>(gt_a) + eq_a - s_a, wb = 2 * static_cast<int64_t>(gt_b) + eq_b - s_b;
    return wa * s_b - wb * s_a;
}

REO_PL_FN uint64_t tp_abs(int64_t v) { return v < 0 ? static_cast<uint64_t>(-v) : static_cast<uint64_t>(v); }
REO_PL_FN uint64_t tp_gamma(int64_t d_i, int64_t d_j) { return tp_abs(d_i - d_j); }

// The rank shift of a gene from its sums of lo + hi over the live sample slots of the two sides (above = lo, below = G - hi per slot, so
// W = sum - G S_side; the G S_A S_B terms cancel).
REO_PL_FN int64_t tp_shift(int64_t sum_a, int64_t sum_b, int64_t s_a, int64_t s_b) { return sum_a * s_b - sum_b * s_a; }

REO_PL_FN TpKey tp_rec_key(const TpRec &r, const int64_t *D, int G, int64_t s_a, int64_t s_b)
{
    return tp_pack(tp_abs(tp_num(r.gt_a, r.eq_a, r.gt_b, r.eq_b, s_a, s_b)), tp_gamma(D[r.i], D[r.j]), r.i, r.j, G);
}

// The final comparison: does the pair of key x come before that of key y?
REO_PL_FN bool tp_before(const TpKey &x, const TpKey &y) { return tp_cmp(x, y) > 0; }

// The tile-skip rule.  A wave owns column tile `ctile` (columns 64 ctile .. 64 ctile + 63) and the rows i0 .. i0 + kTpRows - 1; only pairs
// i < j are walked: a wave whose last column is <= its first row has none, and inside a tile that touches the diagonal the lanes with
// j <= i are dead.
REO_PL_FN bool tp_tile_live(int ctile, int i0, int G) { return ctile * 64 + 63 > i0 && ctile * 64 < G && i0 < G; }
// A workgroup (column tiles kTpWaves bx .. kTpWaves bx + kTpWaves - 1): its last tile reaches furthest right, so when that one has no
// pair none of them has.
REO_PL_FN bool tp_group_live(int bx, int i0) { return (bx * kTpWaves + kTpWaves - 1) * 64 + 63 > i0; }
REO_PL_FN bool tp_lane_live(int i, int j, int G) { return i < j && j < G; }
REO_PL_FN bool tp_mask_bit(const uint32_t *bits, int g) { return !bits || ((bits[g >> 5] >> (g & 31)) & 1u) != 0; }

// Which bits a key can have at all: per field all ones below the highest bit of its bound (|N| <= n_max, Gamma <= g_max; the index field
// is always full).  A digit of this mask that reads 0 is 0 in every key: its pass is skipped and the prefix extended with 0.
REO_PL_FN uint64_t tp_ones_below(uint64_t bound)
{
    uint64_t m = 0;
    while (m < bound) m = (m << 1) | 1u;
    return m;
}
REO_PL_FN TpKey tp_bound_mask(uint64_t n_max, uint64_t g_max)
{
    TpKey k;
    const uint64_t n = tp_ones_below(n_max), g = tp_ones_below(g_max);
    k.hi = (n << (kTpGammaBits - 32)) | (g >> 32);
    k.lo = (g << 32) | 0xFFFFFFFFu;
    return k;
}

// The bin that holds the want-th key (counted from the largest, want >= 1) of a pass: `above` keys lie above the prefix, bins[d] share the
// prefix and have digit d.  Returns the digit, *above_out = keys above (prefix, digit), *share_out = keys that share it; -1 when there are
// fewer than `want` keys at or above the prefix in all (an empty histogram included), with *above_out = their number and *share_out = 0.
inline int tp_pick_digit(const uint64_t *bins /* kTpBins */, uint64_t above, uint64_t want, uint64_t *above_out, uint64_t *share_out)
{
    uint64_t cum = above;
    for (int d = kTpBins - 1; d >= 0; --d) {
        if (cum + bins[d] >= want) { *above_out = cum; *share_out = bins[d]; return d; }
        cum += bins[d];
    }
    *above_out = cum; *share_out = 0;
    return -1;
}

// Candidate records of a call: max(4 n_want, 2^18); `env` = REO_TOP_PAIRS_CAP (tests of deep refinement), which can only lower it and
// never below n_want; <= 0: none.
inline int64_t tp_capacity(int64_t n_want, int64_t env)
{
    int64_t cap = 4 * n_want > kTpMinCapacity ? 4 * n_want : kTpMinCapacity;
    if (env > 0 && env < cap) cap = env < n_want ? n_want : env;
    return cap;
}

// What the selection hands to the emit pass: a pair is a candidate when key >> shift >= cut.
struct TpSelect {
    TpKey cut{0, 0};
    int shift = 0;
    int passes = 0;         // histogram passes run
    uint64_t n_cand = 0;    // candidates the emit pass will find
};

// The pass loop.  hist(prefix, shift, bins) fills bins[kTpHistWords] with the histogram of one pass -- for every eligible pair, with
// t = key >> (shift + 12): t > prefix counts in bins[kTpAbove], t < prefix in bins[kTpBelow], t == prefix in bins[digit at shift] -- and
// returns 0, or an error of its own that the loop passes on.  The library's hist launches k_top_pairs<HIST>; the test driver's walks a
// list of keys.  Returns 0, the error of hist, or -1 when a pass contradicts the passes before it (the counts above the prefix differ).
template <class Hist>
int tp_select(Hist &&hist, const TpKey &bound_mask, uint64_t want, uint64_t capacity, TpSelect *out)
{
    TpKey prefix{0, 0};
    uint64_t above = 0;
    uint64_t bins[kTpHistWords];
    *out = TpSelect();
    for (int s = kTpKeyBits - kTpDigitBits; s >= 0; s -= kTpDigitBits) {
        if (tp_digit(bound_mask, s) == 0) { prefix = tp_extend(prefix, 0); continue; }
        for (int b = 0; b < kTpHistWords; ++b) bins[b] = 0;
        const int rc = hist(prefix, s, bins);
        if (rc) return rc;
        ++out->passes;
        if (bins[kTpAbove] != above) return -1;
        uint64_t share = 0;
        const int d = tp_pick_digit(bins, above, want, &above, &share);
        if (d < 0) {   // fewer than `want` eligible pairs: all of them
            out->cut = TpKey{0, 0}; out->shift = 0; out->n_cand = above;
            return 0;
        }
        prefix = tp_extend(prefix, static_cast<uint32_t>(d));
        out->cut = prefix; out->shift = s; out->n_cand = above + share;
        if (above + share <= capacity) return 0;
    }
    return 0;   // (the key is exhausted: one key shares the prefix, and above < want <= capacity)
}

// What the checks need to know of the context.
struct TpState {
    bool multi;           // a reo_create_multi context (leader or peer)
    int32_t world;        // reo_set_shard
    bool has_mask;        // a validity mask is in force
    int64_t G, S;         // the resident matrix
    int32_t ngroups;
};

// reo_rank_shift and reo_top_pairs share these (what = the call's name).  0 when in order, otherwise the number of the failed check.
inline int tp_check_context(const char *what, const TpState &st, int32_t a, int32_t b, char *msg, size_t msg_n)
{
    if (st.multi) {
        snprintf(msg, msg_n, "%s is not available on a reo_create_multi context (the search runs on one device: use a context of reo_create)", what);
        return 1;
    }
    if (st.world > 1) {
        snprintf(msg, msg_n, "%s is not available on a sharded context (reo_set_shard: %d shards; the search has no exchange)", what, st.world);
        return 2;
    }
    if (st.has_mask) { mp_query_refusal(what, msg, msg_n); return 3; }
    if (st.G > kTpMaxGenes) { snprintf(msg, msg_n, "%s: G = %lld, at most 65535 genes (the 16-plane layout only)", what, (long long)st.G); return 4; }
    if (st.S > kTpMaxSamples) { snprintf(msg, msg_n, "%s: S = %lld, at most 65535 samples", what, (long long)st.S); return 5; }
    if (a < 0 || a >= st.ngroups) { snprintf(msg, msg_n, "%s: a = %d is outside the groups [0, %d)", what, a, st.ngroups); return 6; }
    if (b < -1 || b >= st.ngroups) {
        snprintf(msg, msg_n, "%s: b = %d is outside the groups [0, %d) and not -1 (every other sample)", what, b, st.ngroups);
        return 7;
    }
    if (b == a) { snprintf(msg, msg_n, "%s: b == a == %d, the two sides must differ", what, a); return 8; }
    return 0;
}

inline int tp_check_shift_args(const TpState &st, int32_t a, int32_t b, const int64_t *D, char *msg, size_t msg_n)
{
    const int rc = tp_check_context("reo_rank_shift", st, a, b, msg, msg_n);
    if (rc) return rc;
    if (!D) { snprintf(msg, msg_n, "reo_rank_shift: D must not be null"); return 9; }
    return 0;
}

// Every argument check of reo_top_pairs, on HOST arrays, before anything is uploaded.
inline int tp_check_args(const TpState &st, int32_t a, int32_t b, const uint8_t *gene_mask, int64_t n_want, const int32_t *gene_i,
                         const int32_t *gene_j, const int32_t *counts, const int64_t *key, const int64_t *n_found, char *msg, size_t msg_n)
{
    const int rc = tp_check_context("reo_top_pairs", st, a, b, msg, msg_n);
    if (rc) return rc;
    if (n_want < 1 || n_want > kTpMaxWant) {
        snprintf(msg, msg_n, "reo_top_pairs: n_want = %lld, between 1 and 2^20 pairs per call", (long long)n_want);
        return 9;
    }
    if (!gene_i || !gene_j || !counts || !key || !n_found) {
        snprintf(msg, msg_n, "reo_top_pairs: gene_i, gene_j, counts, key and n_found must not be null");
        return 10;
    }
    for (int64_t g = 0; gene_mask && g < st.G; ++g)
        if (gene_mask[g] > 1) {
            snprintf(msg, msg_n, "reo_top_pairs: gene_mask[%lld] = %d, a byte of the mask is 0 or 1", (long long)g, (int)gene_mask[g]);
            return 11;
        }
    return 0;
}

}  // namespace reo
