// Host-only driver for csrc/top_partners.h (tests/test_top_partners_cpu.py builds it with -fsanitize=address,undefined and runs it): the
// functions that reo_top_partners runs on the host and shares with the kernels of csrc/toppartners.hip.
//   - the cell: tpr_pack / tpr_unpack at the limits (65 535, bit 15 set) and on seeded counts, tpr_num against tp_num;
//   - tpr_before against the packed key of top_pairs.h (tp_pack, tp_before) on the pairs that contain a query gene, equal fields included:
//     the row's order is the subsequence of the search's order;
//   - tpr_takes: the rounds of the selection, run by 1, 3, 64 and 256 "threads" that stride over seeded rows with many equal |N| and
//     Gamma, enumerate the sorted row exactly and end after the last eligible partner; tpr_eligible;
//   - the orientation rule against a recount of "p above q" from seeded outcomes: N changes its sign, the tied counts stay;
//   - the batch rule: the budget, the free memory, the environment's batch, multiples of kTpRows;
//   - tpr_check_args: every check with its number and message, the context's refusals under the call's own name.
//   Prints "ok <checks>"; anything on stderr is a failure.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "top_partners.h"

using namespace reo;

namespace {

long g_checks = 0, g_fail = 0;

uint64_t g_state = 0x13198A2E03707344ULL;
uint64_t rnd()   // splitmix64, seeded: the same words on every run
{
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

void expect(bool ok, const char *what, long a = 0, long b = 0)
{
    ++g_checks;
    if (!ok) { fprintf(stderr, "FAIL %s (%ld, %ld)\n", what, a, b); ++g_fail; }
}

void expect_msg(int got, int want, const char *msg, const char *needle)
{
    expect(got == want, "check number", got, want);
    expect(strstr(msg, needle) != nullptr, needle);
    if (!strstr(msg, needle)) fprintf(stderr, "  message was: %s\n", msg);
}

void cell()
{
    TprCell c = tpr_unpack(tpr_pack(65535, 0, 32768, 32767));
    expect(c.gt_a == 65535 && c.eq_a == 0 && c.gt_b == 32768 && c.eq_b == 32767, "the limits: 65 535 and bit 15");
    expect(tpr_pack(1, 2, 3, 4) == 0x0004000300020001ULL, "gt_A in the lowest 16 bits, eq_B in the highest");
    expect(tpr_num(tpr_unpack(tpr_pack(32768, 0, 0, 0)), 32768, 32767) == int64_t(32768) * 32767 * 2, "bit 15 is a count, not a sign");
    for (int round = 0; round < 400; ++round) {
        const int s_a = 1 + static_cast<int>(rnd() % 65535), s_b = 1 + static_cast<int>(rnd() % 65535);
        const uint32_t gt_a = static_cast<uint32_t>(rnd() % (s_a + 1)), eq_a = static_cast<uint32_t>(rnd() % (s_a - gt_a + 1));
        const uint32_t gt_b = static_cast<uint32_t>(rnd() % (s_b + 1)), eq_b = static_cast<uint32_t>(rnd() % (s_b - gt_b + 1));
        c = tpr_unpack(tpr_pack(gt_a, eq_a, gt_b, eq_b));
        expect(c.gt_a == gt_a && c.eq_a == eq_a && c.gt_b == gt_b && c.eq_b == eq_b, "pack / unpack", round);
        expect(tpr_num(c, s_a, s_b) == tp_num(static_cast<int32_t>(gt_a), static_cast<int32_t>(eq_a), static_cast<int32_t>(gt_b), static_cast<int32_t>(eq_b), s_a, s_b),
               "N of a cell", round);
    }
}

void order()
{
    const int G = 65535;
    for (int round = 0; round < 3000; ++round) {
        const int q = static_cast<int>(rnd() % 200);
        uint64_t n[2], g[2];
        int p[2];
        for (int e = 0; e < 2; ++e) {
            n[e] = rnd() % 4; g[e] = round % 3 ? rnd() % 3 : rnd() >> 16;   // (Gamma below 2^48: what the packed key holds)
            do p[e] = static_cast<int>(rnd() % 200); while (p[e] == q);
        }
        if (p[0] == p[1]) continue;   // (a row lists a partner once)
        if (round % 2 == 0) { n[1] = n[0]; g[1] = g[0]; }
        const TprKey x{n[0], g[0], p[0]}, y{n[1], g[1], p[1]};
        const TpKey kx = tp_pack(n[0], g[0], std::min(q, p[0]), std::max(q, p[0]), G), ky = tp_pack(n[1], g[1], std::min(q, p[1]), std::max(q, p[1]), G);
        expect(tpr_before(x, y) == tp_before(kx, ky), "the row's order is the search's order over the pairs that contain q", round, q);
        expect(tpr_before(x, y) != tpr_before(y, x), "total: one of two partners comes first", round);
    }
    expect(!tpr_before(TprKey{3, 9, 17}, TprKey{3, 9, 17}), "a partner is not before itself");
    expect(tpr_before(TprKey{4, 0, 99}, TprKey{3, 99, 1}) && tpr_before(TprKey{3, 5, 99}, TprKey{3, 4, 1}) && tpr_before(TprKey{3, 5, 8}, TprKey{3, 5, 9}),
           "|N|, then Gamma, then p ascending");
    expect(tpr_before(TprKey{uint64_t(1) << 33, 0, 5}, TprKey{(uint64_t(1) << 33) - 1, ~uint64_t(0), 0}), "|N| above 2^32 is compared whole");
    const uint32_t bits[2] = {0x5u, 0x80000000u};
    expect(tpr_eligible(0, 7, 64, bits) && !tpr_eligible(1, 7, 64, bits) && tpr_eligible(2, 7, 64, bits) && tpr_eligible(63, 7, 64, bits), "the mask's bits");
    expect(!tpr_eligible(2, 2, 64, bits) && !tpr_eligible(63, 7, 63, bits) && tpr_eligible(9, 7, 64, nullptr) && !tpr_eligible(7, 7, 64, nullptr),
           "never the query itself, never a column beyond G; no mask: every gene");
}

// the rounds of k_top_partners_select on the host: `threads` strided scans, then the reduction
void rounds()
{
    for (int round = 0; round < 40; ++round) {
        const int G = 1 + static_cast<int>(rnd() % 300), q = static_cast<int>(rnd() % G);
        std::vector<TprKey> keys;
        std::vector<uint32_t> bits(static_cast<size_t>(G + 31) / 32, 0);
        for (int p = 0; p < G; ++p)
            if (round % 4 == 0 || rnd() % 3) bits[static_cast<size_t>(p) >> 5] |= 1u << (p & 31);
        std::vector<TprKey> all(static_cast<size_t>(G));
        for (int p = 0; p < G; ++p) {
            all[static_cast<size_t>(p)] = TprKey{round % 5 == 0 ? 0 : rnd() % 4, round % 5 == 0 ? 0 : rnd() % 3, p};
            if (tpr_eligible(p, q, G, bits.data())) keys.push_back(all[static_cast<size_t>(p)]);
        }
        std::sort(keys.begin(), keys.end(), [](const TprKey &x, const TprKey &y) { return tpr_before(x, y); });
        for (const int threads : {1, 3, 64, 256}) {
            TprKey prev{0, 0, -1};
            size_t found = 0;
            for (;; ++found) {
                TprKey win{0, 0, -1};
                for (int t = 0; t < threads; ++t) {
                    TprKey mine{0, 0, -1};
                    for (int p = t; p < G; p += threads)
                        if (tpr_eligible(p, q, G, bits.data()) && tpr_takes(all[static_cast<size_t>(p)], prev, mine)) mine = all[static_cast<size_t>(p)];
                    if (mine.p >= 0 && (win.p < 0 || tpr_before(mine, win))) win = mine;
                }
                if (win.p < 0) break;
                expect(found < keys.size() && win.p == keys[found].p && win.abs_n == keys[found].abs_n && win.gamma == keys[found].gamma,
                       "round r finds entry r of the sorted row", static_cast<long>(found), threads);
                if (found >= keys.size()) break;
                prev = win;
            }
            expect(found == keys.size(), "the rounds end after the last eligible partner", static_cast<long>(found), static_cast<long>(keys.size()));
        }
    }
}

void orientation()
{
    for (int round = 0; round < 300; ++round) {
        const int s_a = 1 + static_cast<int>(rnd() % 9), s_b = 1 + static_cast<int>(rnd() % 9);
        int32_t c[4] = {0, 0, 0, 0}, back[4] = {0, 0, 0, 0};   // "q above p" and "p above q"
        for (int s = 0; s < s_a + s_b; ++s) {
            const int out = static_cast<int>(rnd() % 3), side = s < s_a ? 0 : 2;   // 2: q above p, 1: tied, 0: below
            c[side] += out == 2; c[side + 1] += out == 1;
            back[side] += out == 0; back[side + 1] += out == 1;
        }
        const int64_t n = tp_num(c[0], c[1], c[2], c[3], s_a, s_b);
        expect(tp_num(back[0], back[1], back[2], back[3], s_a, s_b) == -n, "N is antisymmetric", round);
        const int32_t q = 10, lo = 3, hi = 20;
        const TpRec same = tpr_orient(q, hi, c[0], c[1], c[2], c[3], s_a, s_b), flip = tpr_orient(q, lo, c[0], c[1], c[2], c[3], s_a, s_b);
        expect(same.i == q && same.j == hi && same.gt_a == c[0] && same.eq_a == c[1] && same.gt_b == c[2] && same.eq_b == c[3], "q < p: as it is", round);
        expect(flip.i == lo && flip.j == q && flip.gt_a == back[0] && flip.eq_a == back[1] && flip.gt_b == back[2] && flip.eq_b == back[3],
               "q > p: the counts of p above q", round);
        expect(tp_num(flip.gt_a, flip.eq_a, flip.gt_b, flip.eq_b, s_a, s_b) == -n, "and N with the other sign", round);
    }
    expect(tpr_flip_gt(32768, 0, 32768) == 0 && tpr_flip_gt(0, 0, 65535) == 65535 && tpr_flip_gt(3, 4, 10) == 3, "gt' = S - gt - eq");
}

void batch()
{
    const uint64_t plenty = uint64_t(1) << 40;
    expect(tpr_padded_rows(1) == 8 && tpr_padded_rows(8) == 8 && tpr_padded_rows(9) == 16 && tpr_padded_rows(1 << 20) == 1 << 20, "multiples of kTpRows");
    expect(tpr_row_bytes(1024, 1) == 8 * 1024 + 36 && tpr_row_bytes(65536, 1024) == 8 * 65536 + 36 * 1024, "8 bytes per cell, 36 per listed partner");
    expect(tpr_batch_rows(20, 1024, 3, plenty, 0) == 24 && tpr_batch_rows(1, 1024, 3, plenty, 0) == 8, "no more than the padded queries");
    expect(tpr_batch_rows(20, 1024, 3, plenty, 8) == 8 && tpr_batch_rows(20, 1024, 3, plenty, 9) == 16 && tpr_batch_rows(20, 1024, 3, plenty, 1) == 8,
           "the environment's batch, padded");
    expect(tpr_batch_rows(20, 1024, 3, plenty, 4000) == 24 && tpr_batch_rows(20, 1024, 3, plenty, -5) == 24, "it can only lower");
    const int64_t full = tpr_batch_rows(1 << 20, 20480, 1, plenty, 0);
    expect(full % kTpRows == 0 && full * tpr_row_bytes(20480, 1) <= kTprBudget && (full + kTpRows) * tpr_row_bytes(20480, 1) > kTprBudget, "the budget of 256 MiB", static_cast<long>(full));
    const int64_t tight = tpr_batch_rows(1 << 20, 20480, 1, 10 * 1000 * 1000, 0);
    expect(tight % kTpRows == 0 && tight * tpr_row_bytes(20480, 1) <= 10 * 1000 * 1000 && tight >= kTpRows && tight < full, "within the free memory", static_cast<long>(tight));
    expect(tpr_batch_rows(1 << 20, 65536, 1024, 1000, 0) == kTpRows, "never below one row tile (the allocation then says so)");
    expect(tpr_batch_rows(65536, 65536, 1024, plenty, 0) * tpr_row_bytes(65536, 1024) <= kTprBudget, "the largest rows");
}

void check_args()
{
    char msg[320];
    const TpState ok{false, 1, false, 300, 12, 3};
    uint8_t mask[300];
    memset(mask, 1, sizeof mask);
    int32_t genes[4] = {0, 299, 7, 7}, partner[8], counts[32], found[4];
    int64_t key[16];
    const auto call = [&](const TpState &st, int32_t a, int32_t b, const int32_t *g, int64_t n, const uint8_t *pm, int32_t m) {
        return tpr_check_args(st, a, b, g, n, pm, m, partner, counts, key, found, msg, sizeof msg);
    };
    expect(call(ok, 0, 2, genes, 4, nullptr, 2) == 0 && call(ok, 1, -1, genes, 1, mask, 1024) == 0, "in order");
    TpState st = ok;
    st.multi = true;
    expect_msg(call(st, 0, 2, genes, 4, nullptr, 2), 1, msg, "reo_top_partners is not available on a reo_create_multi context");
    st = ok; st.world = 4;
    expect_msg(call(st, 0, 2, genes, 4, nullptr, 2), 2, msg, "reo_top_partners is not available on a sharded context (reo_set_shard: 4 shards");
    st = ok; st.has_mask = true;
    expect_msg(call(st, 0, 2, genes, 4, nullptr, 2), 3, msg, "reo_top_partners compares on the bit planes of the whole matrix");
    st = ok; st.G = 65536;
    expect_msg(call(st, 0, 2, genes, 4, nullptr, 2), 4, msg, "G = 65536, at most 65535 genes");
    st = ok; st.S = 65536;
    expect_msg(call(st, 0, 2, genes, 4, nullptr, 2), 5, msg, "S = 65536, at most 65535 samples");
    expect_msg(call(ok, 3, 2, genes, 4, nullptr, 2), 6, msg, "reo_top_partners: a = 3 is outside the groups [0, 3)");
    expect_msg(call(ok, 0, 3, genes, 4, nullptr, 2), 7, msg, "b = 3 is outside the groups [0, 3) and not -1");
    expect_msg(call(ok, 1, 1, genes, 4, nullptr, 2), 8, msg, "reo_top_partners: b == a == 1, the two sides must differ");
    expect_msg(call(ok, 0, 2, genes, 0, nullptr, 2), 9, msg, "reo_top_partners: n_genes = 0, between 1 and 2^20 query genes per call");
    expect_msg(call(ok, 0, 2, genes, (int64_t(1) << 20) + 1, nullptr, 2), 9, msg, "n_genes = 1048577");
    expect_msg(call(ok, 0, 2, nullptr, -1, nullptr, 2), 9, msg, "n_genes = -1");
    expect_msg(call(ok, 0, 2, genes, 4, nullptr, 0), 10, msg, "reo_top_partners: m_want = 0, between 1 and 1024 partners per row");
    expect_msg(call(ok, 0, 2, genes, 4, nullptr, 1025), 10, msg, "m_want = 1025");
    expect_msg(call(ok, 0, 2, genes, (int64_t(1) << 16) + 1, nullptr, 1024), 11, msg, "reo_top_partners: n_genes * m_want = 65537 x 1024, at most 2^26 listed partners per call");
    expect_msg(call(ok, 0, 2, nullptr, 4, nullptr, 2), 12, msg, "reo_top_partners: genes, partner, counts, key and n_found must not be null");
    expect_msg(tpr_check_args(ok, 0, 2, genes, 4, nullptr, 2, nullptr, counts, key, found, msg, sizeof msg), 12, msg, "must not be null");
    expect_msg(tpr_check_args(ok, 0, 2, genes, 4, nullptr, 2, partner, nullptr, key, found, msg, sizeof msg), 12, msg, "must not be null");
    expect_msg(tpr_check_args(ok, 0, 2, genes, 4, nullptr, 2, partner, counts, nullptr, found, msg, sizeof msg), 12, msg, "must not be null");
    expect_msg(tpr_check_args(ok, 0, 2, genes, 4, nullptr, 2, partner, counts, key, nullptr, msg, sizeof msg), 12, msg, "must not be null");
    genes[2] = 300;
    expect_msg(call(ok, 0, 2, genes, 4, nullptr, 2), 13, msg, "reo_top_partners: genes[2] = 300 is outside the genes [0, 300) (row 2 of the answer)");
    expect(call(ok, 0, 2, genes, 2, nullptr, 2) == 0, "a gene beyond n_genes is not read");
    genes[2] = 7; genes[0] = -1;
    expect_msg(call(ok, 0, 2, genes, 4, nullptr, 2), 13, msg, "genes[0] = -1 is outside the genes [0, 300) (row 0");
    genes[0] = 0;
    mask[299] = 2;
    expect_msg(call(ok, 0, 2, genes, 4, mask, 2), 14, msg, "reo_top_partners: partner_mask[299] = 2, a byte of the mask is 0 or 1");
    mask[299] = 0;
    expect(call(ok, 0, 2, genes, 4, mask, 2) == 0, "a query gene outside the mask is in order");
}

}  // namespace

int main()
{
    cell();
    order();
    rounds();
    orientation();
    batch();
    check_args();
    if (g_fail) { fprintf(stderr, "%ld of %ld checks failed\n", g_fail, g_checks); return 1; }
    printf("ok %ld\n", g_checks);
    return 0;
}
