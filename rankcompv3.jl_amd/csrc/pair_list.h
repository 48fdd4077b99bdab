// The pair list (reo_pair_list): which partner genes make up a gene's contingency tallies.  What both kernels of pairlist.hip and a host
// driver share: the selected-pair word of 32 table columns, the per-bit class it stands for, the validity word of a table word, and the
// argument checks that need no GPU -- so that a host driver can evaluate the very same functions under the sanitizers
// (tests/pair_list_driver.cpp).  No HIP header in here: plain C++17 (the kernels' unit defines the function attributes).
//
// The class table is [G][4 planes][Wp] 32-bit words, planes cL cH tL tH; bit j of row i holds the ordered pair (i, j) seen from gene i.
// A pair is in at most one of L / H on each side; neither bit set is the middle class.  The class code is 3 * ic + it with
// ic = 0 (cL), 1 (neither), 2 (cH) and it likewise from tL / tH: the column of the reference's R[(i-1)*r+j, :] minus one
// (src/RankCompV3.jl:383-386), what reo_get_codes returns, and the position of the pair's tally among n11 .. n33 (:403).
#pragma once

#include <cstdint>
#include <cstdio>

#if defined(__HIPCC__)
#define REO_PL_FN __host__ __device__ inline
#else
#define REO_PL_FN inline
#endif

namespace reo {

constexpr uint32_t kPairClassAll = 0x1FFu;   // class codes 0 .. 8

// Columns 32 w .. 32 w + 31 of row `row`: the bits that are gene columns (< G) and not the diagonal.
REO_PL_FN uint32_t pair_valid_word(int row, int w, int G)
{
    const int c0 = w * 32;
    uint32_t valid = 0xFFFFFFFFu;
    if (c0 + 32 > G) valid = c0 >= G ? 0u : (0xFFFFFFFFu >> (c0 + 32 - G));
    if ((row >> 5) == w) valid &= ~(1u << (row & 31));
    return valid;
}

// The pairs of one table word whose class is selected: the OR over the selected codes c of C[c / 3] & T[c % 3], with
// C = {cl, ~(cl | ch), ch} and T likewise -- per C the three T terms are gathered first, nine ANDs become three.  `valid` clears the
// columns >= G and the diagonal bit (pair_valid_word), and whatever partner mask the caller has ANDed into it.
REO_PL_FN uint32_t pair_select_word(uint32_t cl, uint32_t ch, uint32_t tl, uint32_t th, uint32_t valid, uint32_t class_mask)
{
    const uint32_t C[3] = {cl, ~(cl | ch), ch}, T[3] = {tl, ~(tl | th), th};
    uint32_t sel = 0;
    for (int ic = 0; ic < 3; ++ic) {
        const uint32_t m = (class_mask >> (3 * ic)) & 7u;
        const uint32_t t = ((m & 1u) ? T[0] : 0u) | ((m & 2u) ? T[1] : 0u) | ((m & 4u) ? T[2] : 0u);
        sel |= C[ic] & t;
    }
    return sel & valid;
}

// The class code of bit `b` of a table word.
REO_PL_FN uint32_t pair_code_at(uint32_t cl, uint32_t ch, uint32_t tl, uint32_t th, int b)
{
    const uint32_t ic = ((cl >> b) & 1u) ? 0u : (((ch >> b) & 1u) ? 2u : 1u);
    const uint32_t it = ((tl >> b) & 1u) ? 0u : (((th >> b) & 1u) ? 2u : 1u);
    return 3u * ic + it;
}

// Two checks that every query entry point makes (reo_pair_list, reo_sample_counts, reo_sample_tests, reo_pair_support) with its own name
// `what` in front: true when in order, otherwise false and the message in msg.  genes is a HOST array (null or n_genes < 1: nothing to check).
inline bool query_genes_in_range(const char *what, int64_t G, const int32_t *genes, int64_t n_genes, char *msg, size_t msg_n)
{
    for (int64_t q = 0; genes && q < n_genes; ++q)
        if (genes[q] < 0 || genes[q] >= G) {
            snprintf(msg, msg_n, "%s: genes[%lld] = %d is outside [0, %lld)", what, (long long)q, genes[q], (long long)G);
            return false;
        }
    return true;
}

inline bool query_class_mask_ok(const char *what, uint32_t class_mask, char *msg, size_t msg_n)
{
    if (class_mask != 0 && !(class_mask & ~kPairClassAll)) return true;
    snprintf(msg, msg_n, "%s: class_mask 0x%X selects %s (bit c selects class code c = 3*(ic-1)+(it-1), c in 0..8: 0x1 .. 0x1FF)", what, class_mask,
             class_mask == 0 ? "no class" : "bits above 8");
    return false;
}

// Argument checks of reo_pair_list that need neither the context's state nor the GPU.  0 when everything is in order; otherwise the number
// of the failed check (1 ..) and its message in msg.  genes is a HOST array.
inline int pair_list_check_args(int64_t G, const int32_t *genes, int64_t n_genes, uint32_t class_mask, const int64_t *rowptr,
                                const int32_t *partner, const uint8_t *code, int64_t capacity, char *msg, size_t msg_n)
{
    if (!genes || !rowptr) { snprintf(msg, msg_n, "reo_pair_list: genes and rowptr must not be null"); return 1; }
    if (n_genes < 1) { snprintf(msg, msg_n, "reo_pair_list: n_genes = %lld, at least one query gene is needed", (long long)n_genes); return 2; }
    if (!query_class_mask_ok("reo_pair_list", class_mask, msg, msg_n)) return 3;
    if ((partner == nullptr) != (code == nullptr)) {
        snprintf(msg, msg_n, "reo_pair_list: partner and code are both given, or both null (count only)");
        return 4;
    }
    if (capacity < 0 || (!partner && capacity != 0)) {
        snprintf(msg, msg_n, "reo_pair_list: capacity %lld (it counts the entries of partner and code; 0 when they are null)", (long long)capacity);
        return 5;
    }
    return query_genes_in_range("reo_pair_list", G, genes, n_genes, msg, msg_n) ? 0 : 6;
}

// rowptr from the per-query counts (64-bit prefix sums); returns the total.
inline int64_t pair_list_rowptr(const int32_t *count, int64_t n_genes, int64_t *rowptr)
{
    int64_t at = 0;
    for (int64_t q = 0; q < n_genes; ++q) { rowptr[q] = at; at += count[q]; }
    rowptr[n_genes] = at;
    return at;
}

}  // namespace reo
