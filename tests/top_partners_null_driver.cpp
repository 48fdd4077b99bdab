// Host-only driver for csrc/top_partners_null.h (tests/test_top_partners_null_cpu.py builds it with -fsanitize=address,undefined and runs
// it): the functions that reo_top_partners_null runs on the host and shares with the kernel of csrc/toppartnersnull.hip.
//   - tprn_check_args: every check with its number and message, the context's refusals of tp_check_context under the call's own name;
//   - tprn_key / tprn_unpack: the fields come back, key 0 is "no partner", no partner has key 0 (partner 65 534 at |N| = 0 included), and
//     the order of keys is "|N| descending, then p ascending" on seeded partners;
//   - tprn_eligible against a bit mask, tprn_cut_word, tprn_padded_rows;
//   - tprn_batch: the cap, the environment's cap, fewer permutations than either, the budget and the free memory, whole launch groups
//     above kPermQ, never below 1.
//   Prints "ok <checks>"; anything on stderr is a failure.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "top_partners_null.h"

using namespace reo;

namespace {

long g_checks = 0, g_fail = 0;

uint64_t g_state = 0x243F6A8885A308D3ULL;
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

// Twelve samples of three groups: 0 0 1 1 2 2 0 1 2 0 1 1 -- sizes 4, 5, 3.
const int32_t kGid[12] = {0, 0, 1, 1, 2, 2, 0, 1, 2, 0, 1, 1};

void check_args()
{
    char msg[320];
    const TpState ok{false, 1, false, 300, 12, 3};
    uint8_t rows[3 * 12];
    for (int p = 0; p < 3; ++p)
        for (int s = 0; s < 12; ++s) rows[p * 12 + s] = tn_column_byte(kGid[s], 0, 2, 3);   // group 0 against group 2: 4 ones, 3 zeros, 5 twos
    std::swap(rows[12 + 0], rows[12 + 4]);                                                  // row 1: a shuffle inside A and B
    uint8_t mask[300];
    memset(mask, 1, sizeof mask);
    const int32_t genes[5] = {0, 299, 7, 7, 150};
    int64_t cuts[5] = {0, 1, 24, int64_t(1) << 40, 7}, max_n[15], s_a = -5, s_b = -5;
    int32_t arg[15], reach[15];
    const auto call = [&](const TpState &st, int32_t a, int32_t b, const uint8_t *r, int64_t n_perm, const int32_t *g, int64_t n_genes, const uint8_t *pm,
                          const int64_t *c, int64_t *mx, int32_t *ap, int32_t *nr) {
        return tprn_check_args(st, kGid, a, b, r, n_perm, g, n_genes, pm, c, mx, ap, nr, &s_a, &s_b, msg, sizeof msg);
    };
    expect(call(ok, 0, 2, rows, 3, genes, 5, nullptr, cuts, max_n, arg, reach) == 0 && s_a == 4 && s_b == 3, "in order, with cuts", s_a, s_b);
    expect(call(ok, 0, 2, rows, 3, genes, 5, mask, nullptr, max_n, arg, nullptr) == 0, "in order, a mask, no cuts and no counters");
    uint8_t rest[12];
    for (int s = 0; s < 12; ++s) rest[s] = tn_column_byte(kGid[s], 1, -1, 3);
    expect(call(ok, 1, -1, rest, 1, genes, 1, nullptr, nullptr, max_n, arg, nullptr) == 0 && s_a == 5 && s_b == 7, "group 1 against the rest", s_a, s_b);
    // the context's refusals, under this call's name
    TpState st = ok;
    st.multi = true;
    expect_msg(call(st, 0, 2, rows, 3, genes, 5, nullptr, cuts, max_n, arg, reach), 1, msg, "reo_top_partners_null is not available on a reo_create_multi context");
    st = ok; st.world = 4;
    expect_msg(call(st, 0, 2, rows, 3, genes, 5, nullptr, cuts, max_n, arg, reach), 2, msg,
               "reo_top_partners_null is not available on a sharded context (reo_set_shard: 4 shards");
    st = ok; st.has_mask = true;
    expect_msg(call(st, 0, 2, rows, 3, genes, 5, nullptr, cuts, max_n, arg, reach), 3, msg, "reo_top_partners_null compares on the bit planes of the whole matrix");
    st = ok; st.G = 65536;
    expect_msg(call(st, 0, 2, rows, 3, genes, 5, nullptr, cuts, max_n, arg, reach), 4, msg, "G = 65536, at most 65535 genes");
    st = ok; st.S = 70000;
    expect_msg(call(st, 0, 2, rows, 3, genes, 5, nullptr, cuts, max_n, arg, reach), 5, msg, "S = 70000, at most 65535 samples");
    expect_msg(call(ok, 3, 2, rows, 3, genes, 5, nullptr, cuts, max_n, arg, reach), 6, msg, "a = 3 is outside the groups [0, 3)");
    expect_msg(call(ok, 0, 3, rows, 3, genes, 5, nullptr, cuts, max_n, arg, reach), 7, msg, "b = 3 is outside the groups");
    expect_msg(call(ok, 2, 2, rows, 3, genes, 5, nullptr, cuts, max_n, arg, reach), 8, msg, "reo_top_partners_null: b == a == 2");
    // its own
    expect_msg(call(ok, 0, 2, rows, 0, genes, 5, nullptr, cuts, max_n, arg, reach), 9, msg, "n_perm = 0, between 1 and 2^20");
    expect_msg(call(ok, 0, 2, rows, (1 << 20) + 1, genes, 5, nullptr, cuts, max_n, arg, reach), 9, msg, "n_perm = 1048577");
    expect_msg(call(ok, 0, 2, rows, 3, genes, 0, nullptr, cuts, max_n, arg, reach), 10, msg, "n_genes = 0, between 1 and 2^20 query genes");
    expect_msg(call(ok, 0, 2, rows, 3, genes, (1 << 20) + 1, nullptr, cuts, max_n, arg, reach), 10, msg, "n_genes = 1048577");
    expect_msg(call(ok, 0, 2, rows, 1 << 13, genes, (1 << 13) + 1, nullptr, cuts, max_n, arg, reach), 11, msg,
               "n_perm * n_genes = 8192 x 8193, at most 2^26 cells per call");
    expect_msg(call(ok, 0, 2, nullptr, 3, genes, 5, nullptr, cuts, max_n, arg, reach), 12, msg, "sides, genes, max_n and arg_p must not be null");
    expect_msg(call(ok, 0, 2, rows, 3, nullptr, 5, nullptr, cuts, max_n, arg, reach), 12, msg, "must not be null");
    expect_msg(call(ok, 0, 2, rows, 3, genes, 5, nullptr, cuts, nullptr, arg, reach), 12, msg, "must not be null");
    expect_msg(call(ok, 0, 2, rows, 3, genes, 5, nullptr, cuts, max_n, nullptr, reach), 12, msg, "must not be null");
    expect_msg(call(ok, 0, 2, rows, 3, genes, 5, nullptr, cuts, max_n, arg, nullptr), 13, msg, "n_reach is null and cuts is not: n_reach is null exactly when cuts is");
    expect_msg(call(ok, 0, 2, rows, 3, genes, 5, nullptr, nullptr, max_n, arg, reach), 13, msg, "cuts is null and n_reach is not: n_reach is null exactly when cuts is");
    const int32_t far[3] = {4, 300, -1}, below[3] = {4, 5, -1};
    expect_msg(call(ok, 0, 2, rows, 3, far, 3, nullptr, nullptr, max_n, arg, nullptr), 14, msg, "genes[1] = 300 is outside the genes [0, 300)");
    expect_msg(call(ok, 0, 2, rows, 3, below, 3, nullptr, nullptr, max_n, arg, nullptr), 14, msg, "genes[2] = -1 is outside the genes");
    expect(call(ok, 0, 2, rows, 3, below, 2, nullptr, nullptr, max_n, arg, nullptr) == 0, "the genes in front of the wrong one are in order");
    int64_t neg[5] = {4, 0, 3, -1, 2};
    expect_msg(call(ok, 0, 2, rows, 3, genes, 5, nullptr, neg, max_n, arg, reach), 15, msg, "cuts[3] = -1, a cut of |N| is not negative");
    expect(call(ok, 0, 2, rows, 3, genes, 3, nullptr, neg, max_n, arg, reach) == 0, "the cuts of the rows asked for");
    expect_msg(tprn_check_args(ok, nullptr, 0, 2, rows, 3, genes, 5, nullptr, cuts, max_n, arg, reach, &s_a, &s_b, msg, sizeof msg), 16, msg, "no group labels");
    const int32_t one[12] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};
    expect_msg(tprn_check_args(ok, one, 1, -1, rows, 3, genes, 5, nullptr, cuts, max_n, arg, reach, &s_a, &s_b, msg, sizeof msg), 17, msg,
               "side A has 12 samples and side B 0, both sides need at least one");
    uint8_t bad[3 * 12];
    memcpy(bad, rows, sizeof bad);
    bad[2 * 12 + 7] = 3;
    expect_msg(call(ok, 0, 2, bad, 3, genes, 5, nullptr, cuts, max_n, arg, reach), 18, msg, "row 2 of sides holds the byte 3 in column 7");
    memcpy(bad, rows, sizeof bad);
    bad[12 + 2] = 0;                                                                        // a sample of group 1 takes part
    expect_msg(call(ok, 0, 2, bad, 3, genes, 5, nullptr, cuts, max_n, arg, reach), 19, msg, "row 1 of sides holds the byte 0 in column 2, whose sample is on neither side");
    memcpy(bad, rows, sizeof bad);
    bad[0] = 2;                                                                             // a sample of group 0 takes no part
    expect_msg(call(ok, 0, 2, bad, 3, genes, 5, nullptr, cuts, max_n, arg, reach), 19, msg,
               "row 0 of sides holds the byte 2 in column 0, whose sample is on one of the sides");
    memcpy(bad, rows, sizeof bad);
    bad[2 * 12 + 4] = 1;                                                                    // a zero became a one
    expect_msg(call(ok, 0, 2, bad, 3, genes, 5, nullptr, cuts, max_n, arg, reach), 20, msg,
               "row 2 of sides has 5 ones and 2 zeros, side A has 4 samples and side B 3");
    expect(call(ok, 0, 2, bad, 2, genes, 5, nullptr, cuts, max_n, arg, reach) == 0, "the rows in front of the wrong one are in order");
    mask[299] = 2;
    expect_msg(call(ok, 0, 2, rows, 3, genes, 5, mask, cuts, max_n, arg, reach), 21, msg, "partner_mask[299] = 2");
}

void check_key()
{
    int64_t m = 0;
    int32_t p = 0;
    tprn_unpack(0, &m, &p);
    expect(m == -1 && p == -1, "key 0: no partner");
    expect(tprn_key(0, 65534) != 0 && tprn_key(0, 65534) == 0xFFFFFFFFull - 65534ull, "the last partner of the largest problem at |N| = 0 has a key");
    expect(tprn_key(0x7FFFFFFFull, 0) >> 63 == 0, "63 bits");
    struct Cand { uint64_t n; int p; };
    std::vector<Cand> cs;
    for (int t = 0; t < 2000; ++t) cs.push_back(Cand{rnd() % 5 == 0 ? 0x7FFFFFFFull : rnd() % 7, static_cast<int>(rnd() % 65535)});
    for (const Cand &c : cs) {
        const uint64_t k = tprn_key(c.n, c.p);
        tprn_unpack(k, &m, &p);
        expect(k != 0 && m == static_cast<int64_t>(c.n) && p == c.p, "the fields come back", p, c.p);
    }
    for (size_t x = 0; x + 1 < cs.size(); ++x) {
        const Cand &c = cs[x], &d = cs[x + 1];
        const bool first = c.n != d.n ? c.n > d.n : c.p < d.p, same = c.n == d.n && c.p == d.p;
        const uint64_t kc = tprn_key(c.n, c.p), kd = tprn_key(d.n, d.p);
        expect(same ? kc == kd : (first ? kc > kd : kc < kd), "a larger key is a larger |N| or a smaller partner", static_cast<long>(x));
    }
}

void check_small_rules()
{
    std::vector<uint32_t> bits(4, 0u);   // 128 genes, the even ones inside the mask
    for (int g = 0; g < 128; g += 2) bits[static_cast<size_t>(g) >> 5] |= 1u << (g & 31);
    for (int q = 0; q < 100; q += 7)
        for (int p = 0; p < 128; ++p) {
            expect(tprn_eligible(p, q, 100, nullptr) == (p != q && p < 100), "no mask: every other gene below G", q, p);
            expect(tprn_eligible(p, q, 100, bits.data()) == (p != q && p < 100 && p % 2 == 0), "the mask filters the partners, not the query", q, p);
        }
    expect(tprn_cut_word(0) == 0 && tprn_cut_word(5) == 5 && tprn_cut_word((int64_t(1) << 31) - 1) == 0x7FFFFFFFu, "a cut below 2^31 is itself");
    expect(tprn_cut_word(int64_t(1) << 31) == 0xFFFFFFFFu && tprn_cut_word(int64_t(1) << 40) == 0xFFFFFFFFu, "a cut no |N| reaches");
    expect(tprn_padded_rows(1) == kTnRows && tprn_padded_rows(kTnRows) == kTnRows && tprn_padded_rows(kTnRows + 1) == 2 * kTnRows &&
           tprn_padded_rows(7) == 8, "whole row tiles");
}

void check_batch()
{
    const uint64_t lots = uint64_t(1) << 40;
    expect(tprn_batch(1000, 300, lots, 0) == 64 && tprn_batch(1000, 300, lots, -3) == 64, "the cap");
    expect(tprn_batch(1000, 300, lots, 20) == 16 && tprn_batch(1000, 300, lots, 1) == 1 && tprn_batch(1000, 300, lots, 500) == 64 &&
           tprn_batch(1000, 300, lots, 16) == 16 && tprn_batch(1000, 300, lots, 15) == 15 && tprn_batch(1000, 300, lots, 33) == 32,
           "the environment can only lower it; whole launch groups above kPermQ");
    expect(tprn_batch(17, 300, lots, 0) == 16 && tprn_batch(33, 300, lots, 0) == 32 && tprn_batch(16, 300, lots, 0) == 16 && tprn_batch(5, 300, lots, 0) == 5 &&
           tprn_batch(1, 300, lots, 64) == 1, "never more than the permutations");
    // the budget: 12 bytes per (permutation, padded row) within kTprBudget = 256 MiB -- 2^20 rows: 21 fit, 16 are taken
    expect(tprn_batch(64, 1 << 20, lots, 0) == 16, "2^20 query rows", tprn_batch(64, 1 << 20, lots, 0));
    expect(tprn_batch(64, 1 << 19, lots, 0) == 32 && tprn_batch(64, 1 << 18, lots, 0) == 64, "2^19 and 2^18 query rows");
    expect(tprn_batch(64, 1 << 20, uint64_t(12) << 20, 0) == 1 && tprn_batch(64, 1 << 20, 0, 0) == 1, "little free memory: never below 1");
    expect(tprn_batch(64, 1000, 12 * 1000 * 40, 0) == 32 && tprn_batch(64, 1000, 12 * 1000 * 10, 0) == 10 && tprn_batch(64, 999, 12 * 1000 * 10, 0) == 10,
           "the free memory, in padded rows");
    for (int t = 0; t < 3000; ++t) {
        const int64_t n_perm = 1 + static_cast<int64_t>(rnd() % 200), n_genes = 1 + static_cast<int64_t>(rnd() % (1 << 20));
        const int64_t env = static_cast<int64_t>(rnd() % 80) - 5;
        const uint64_t free_bytes = rnd() % (uint64_t(1) << 30);
        const int64_t p = tprn_batch(n_perm, n_genes, free_bytes, env);
        const uint64_t budget = std::min<uint64_t>(free_bytes, static_cast<uint64_t>(kTprBudget));
        expect(p >= 1 && p <= kTprnBatchCap && p <= n_perm && (env <= 0 || p <= env) && (p <= kPermQ || p % kPermQ == 0), "the rule's bounds", p, n_perm);
        expect(p == 1 || static_cast<uint64_t>(p * kTprnCellBytes * tprn_padded_rows(n_genes)) <= budget, "the batch fits the budget", p, n_genes);
    }
    expect(kTprnBatchCap % kPermQ == 0 && kTprnMaxPerms == 1 << 20 && kTprnMaxGenes == 1 << 20 && kTprnMaxCells == 1 << 26 && kTprnCellBytes == 12,
           "the constants of the header");
}

}  // namespace

int main()
{
    check_args();
    check_key();
    check_small_rules();
    check_batch();
    if (g_fail) { fprintf(stderr, "%ld of %ld checks failed\n", g_fail, g_checks); return 1; }
    printf("ok %ld\n", g_checks);
    return 0;
}
