// Top partners (reo_top_partners): for every query gene q the best m partner genes p, the row-shaped answer to the question that
// reo_top_pairs answers for all pairs at once.  What the kernels of toppartners.hip, the entry point of queries.hip and a host driver of the
// tests share, so that the driver can evaluate the very same functions under the sanitizers (tests/top_partners_driver.cpp): the cell that
// the count kernel stores per (query, column), the key of a row and its comparison, the orientation rule, the batch rule and every argument
// check with its message.  No HIP header in here: plain C++17 (the kernels' unit defines the function attributes through pair_list.h).
//
// The row of q (include/reo_hip.h): every p != q inside partner_mask, with the four counts of "q above p", N_qp = tp_num of those (signed,
// N_pq = -N_qp) and Gamma_qp = |D_q - D_p| (D over all genes, whatever the mask); ordered |N| descending, Gamma descending, p ascending.
// The identity with top_pairs.h: that order over i < j is |N| descending, Gamma descending, (i, j) ascending.  |N| and Gamma do not depend on
// the orientation of a pair, and among the pairs that contain q, (i, j) = (min(q, p), max(q, p)) ascends exactly when p ascends (p < q: the
// pairs (p, q), first and ordered by p; p > q: the pairs (q, p), behind them and ordered by p).  So the row of q is the subsequence of
// reo_top_pairs' total order over all pairs that contain q, re-oriented to "q above p" (tests/test_top_partners_cpu.py pins it).
#pragma once

#include <cstdint>
#include <cstdio>

#include "top_pairs.h"

namespace reo {

constexpr int64_t kTprMaxGenes = int64_t(1) << 20;      // query genes per call
constexpr int32_t kTprMaxWant = 1024;                   // partners per row
constexpr int64_t kTprMaxCells = int64_t(1) << 26;      // n_genes * m_want: the caller's arrays
constexpr int64_t kTprBudget = int64_t(256) << 20;      // device bytes of one batch: its cells and its rows of the outputs
constexpr int kTprThreads = 256;                        // threads of one row's workgroup in k_top_partners_select

// What the count kernel stores per (query row, column p): the counts of "q above p".  Unsigned 16 bits each: a side has at most 65 535
// samples (kTpMaxSamples), and S_A = 32 768 sets bit 15.
struct TprCell {
    uint16_t gt_a, eq_a, gt_b, eq_b;
};
static_assert(sizeof(TprCell) == 8, "one 64-bit store per lane");
static_assert(kTpMaxSamples <= 0xFFFF, "a count fits the cell");

REO_PL_FN uint64_t tpr_pack(uint32_t gt_a, uint32_t eq_a, uint32_t gt_b, uint32_t eq_b)
{
    return static_cast<uint64_t>(gt_a & 0xFFFFu) | (static_cast<uint64_t>(eq_a & 0xFFFFu) << 16) | (static_cast<uint64_t>(gt_b & 0xFFFFu) << 32) |
           (static_cast<uint64_t>(eq_b & 0xFFFFu) << 48);
}
REO_PL_FN TprCell tpr_unpack(uint64_t w)
{
    return TprCell{static_cast<uint16_t>(w), static_cast<uint16_t>(w >> 16), static_cast<uint16_t>(w >> 32), static_cast<uint16_t>(w >> 48)};
}
REO_PL_FN int64_t tpr_num(const TprCell &c, int64_t s_a, int64_t s_b) { return tp_num(c.gt_a, c.eq_a, c.gt_b, c.eq_b, s_a, s_b); }

// The key of partner p in the row of q; p < 0: no partner.
struct TprKey {
    uint64_t abs_n, gamma;
    int32_t p;
};
REO_PL_FN TprKey tpr_key(const TprCell &c, int64_t d_q, int64_t d_p, int32_t p, int64_t s_a, int64_t s_b)
{
    return TprKey{tp_abs(tpr_num(c, s_a, s_b)), tp_gamma(d_q, d_p), p};
}
// Does partner x come before partner y in the row's order?  |N| descending, Gamma descending, p ascending; no two partners of a row share p.
REO_PL_FN bool tpr_before(const TprKey &x, const TprKey &y)
{
    if (x.abs_n != y.abs_n) return x.abs_n > y.abs_n;
    if (x.gamma != y.gamma) return x.gamma > y.gamma;
    return x.p < y.p;
}
// One step of a round of the selection: `cand` replaces `best` when it lies strictly behind the previous round's winner `prev` (prev.p < 0:
// the first round, nothing to lie behind) and before `best` (best.p < 0: none yet).
REO_PL_FN bool tpr_takes(const TprKey &cand, const TprKey &prev, const TprKey &best)
{
    if (prev.p >= 0 && !tpr_before(prev, cand)) return false;
    return best.p < 0 || tpr_before(cand, best);
}
REO_PL_FN bool tpr_eligible(int32_t p, int32_t q, int G, const uint32_t *maskbits) { return p != q && p < G && tp_mask_bit(maskbits, p); }

// The orientation rule: the counts of "p above q" on a side of `s` samples from those of "q above p" (lt = s - gt - eq changes places with gt,
// the tied samples stay); with both sides flipped N changes its sign and Gamma stays.
REO_PL_FN int32_t tpr_flip_gt(int32_t gt, int32_t eq, int64_t s) { return static_cast<int32_t>(s - gt - eq); }
REO_PL_FN TpRec tpr_orient(int32_t q, int32_t p, int32_t gt_a, int32_t eq_a, int32_t gt_b, int32_t eq_b, int64_t s_a, int64_t s_b)
{
    if (q < p) return TpRec{q, p, gt_a, eq_a, gt_b, eq_b};
    return TpRec{p, q, tpr_flip_gt(gt_a, eq_a, s_a), eq_a, tpr_flip_gt(gt_b, eq_b, s_b), eq_b};
}

// The batch rule.  A query row costs 8 Gp bytes of cells and 36 m_want bytes of outputs on the device; a batch stays within kTprBudget and
// within the free memory, is a multiple of kTpRows, at least kTpRows and no more than the padded number of queries.  `env` =
// REO_TOP_PARTNERS_BATCH (tests of the seam) can only lower it; <= 0: none.
REO_PL_FN int64_t tpr_padded_rows(int64_t n) { return (n + kTpRows - 1) / kTpRows * kTpRows; }
REO_PL_FN int64_t tpr_row_bytes(int64_t Gp, int64_t m_want) { return 8 * Gp + 36 * m_want; }
inline int64_t tpr_batch_rows(int64_t n_genes, int64_t Gp, int64_t m_want, uint64_t free_bytes, int64_t env)
{
    const uint64_t budget = free_bytes < static_cast<uint64_t>(kTprBudget) ? free_bytes : static_cast<uint64_t>(kTprBudget);
    int64_t rows = static_cast<int64_t>(budget / static_cast<uint64_t>(tpr_row_bytes(Gp, m_want))) / kTpRows * kTpRows;
    if (env > 0 && tpr_padded_rows(env) < rows) rows = tpr_padded_rows(env);
    if (rows > tpr_padded_rows(n_genes)) rows = tpr_padded_rows(n_genes);
    return rows < kTpRows ? kTpRows : rows;
}

// Every argument check of reo_top_partners, on HOST arrays, before anything is uploaded.  0 when in order, otherwise the number of the
// failed check (1 .. 8: tp_check_context's).
inline int tpr_check_args(const TpState &st, int32_t a, int32_t b, const int32_t *genes, int64_t n_genes, const uint8_t *partner_mask, int32_t m_want,
                          const int32_t *partner, const int32_t *counts, const int64_t *key, const int32_t *n_found, char *msg, size_t msg_n)
{
    const int rc = tp_check_context("reo_top_partners", st, a, b, msg, msg_n);
    if (rc) return rc;
    if (n_genes < 1 || n_genes > kTprMaxGenes) {
        snprintf(msg, msg_n, "reo_top_partners: n_genes = %lld, between 1 and 2^20 query genes per call", (long long)n_genes);
        return 9;
    }
    if (m_want < 1 || m_want > kTprMaxWant) {
        snprintf(msg, msg_n, "reo_top_partners: m_want = %d, between 1 and %d partners per row", m_want, kTprMaxWant);
        return 10;
    }
    if (n_genes * m_want > kTprMaxCells) {
        snprintf(msg, msg_n, "reo_top_partners: n_genes * m_want = %lld x %d, at most 2^26 listed partners per call", (long long)n_genes, m_want);
        return 11;
    }
    if (!genes || !partner || !counts || !key || !n_found) {
        snprintf(msg, msg_n, "reo_top_partners: genes, partner, counts, key and n_found must not be null");
        return 12;
    }
    for (int64_t q = 0; q < n_genes; ++q)
        if (genes[q] < 0 || genes[q] >= st.G) {
            snprintf(msg, msg_n, "reo_top_partners: genes[%lld] = %d is outside the genes [0, %lld) (row %lld of the answer)", (long long)q, genes[q],
                     (long long)st.G, (long long)q);
            return 13;
        }
    for (int64_t g = 0; partner_mask && g < st.G; ++g)
        if (partner_mask[g] > 1) {
            snprintf(msg, msg_n, "reo_top_partners: partner_mask[%lld] = %d, a byte of the mask is 0 or 1", (long long)g, (int)partner_mask[g]);
            return 14;
        }
    return 0;
}

}  // namespace reo
