// Host-only driver for csrc/top_pairs_null.h (tests/test_top_pairs_null_cpu.py builds it with -fsanitize=address,undefined and runs it): the
// functions that reo_top_pairs_null runs on the host and shares with the kernels of csrc/toppairsnull.hip.
//   - tn_check_args: every check with its number and message, the context's refusals of tp_check_context under the call's own name;
//   - tn_column_byte, tn_check_row: the observed bytes of three groups for (a, b) and (a, -1), rows in order and each kind of wrong row;
//   - pn_side_word / pn_word_index / pn_word_count with rows that hold a 2, and tn_live_word: the live word leaves out padding and the
//     columns of neither side, A is a subset of live, live minus A is side B, for every block of a seeded slot map;
//   - tn_key / tn_unpack: the fields come back, key 0 is "no pair", no pair has key 0 (the last pair of 65 535 genes at |N| = 0 included),
//     and the order of keys is "|N| descending, then (i, j) ascending" on seeded pairs;
//   - tn_batch: the cap, the environment's cap, fewer permutations than either.
//   Prints "ok <checks>"; anything on stderr is a failure.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "top_pairs_null.h"

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
    int64_t cuts[8] = {0, 1, 5, 24, 25, 1 << 20, int64_t(1) << 40, 7}, max_n[3], reach[24], s_a = -5, s_b = -5;
    int32_t gi[3], gj[3];
    const auto call = [&](const TpState &st, int32_t a, int32_t b, const uint8_t *r, int64_t n_perm, const uint8_t *gm, const int64_t *c, int32_t nc,
                          int64_t *mx, int32_t *ai, int32_t *aj, int64_t *nr) {
        return tn_check_args(st, kGid, a, b, r, n_perm, gm, c, nc, mx, ai, aj, nr, &s_a, &s_b, msg, sizeof msg);
    };
    expect(call(ok, 0, 2, rows, 3, nullptr, cuts, 8, max_n, gi, gj, reach) == 0 && s_a == 4 && s_b == 3, "in order, eight cuts", s_a, s_b);
    expect(call(ok, 0, 2, rows, 3, mask, nullptr, 0, max_n, gi, gj, nullptr) == 0, "in order, a mask, no cuts and neither array");
    uint8_t rest[12];
    for (int s = 0; s < 12; ++s) rest[s] = tn_column_byte(kGid[s], 1, -1, 3);
    expect(call(ok, 1, -1, rest, 1, nullptr, nullptr, 0, max_n, gi, gj, nullptr) == 0 && s_a == 5 && s_b == 7, "group 1 against the rest", s_a, s_b);
    // the context's refusals, under this call's name
    TpState st = ok;
    st.multi = true;
    expect_msg(call(st, 0, 2, rows, 3, nullptr, cuts, 2, max_n, gi, gj, reach), 1, msg, "reo_top_pairs_null is not available on a reo_create_multi context");
    st = ok; st.world = 4;
    expect_msg(call(st, 0, 2, rows, 3, nullptr, cuts, 2, max_n, gi, gj, reach), 2, msg, "reo_top_pairs_null is not available on a sharded context (reo_set_shard: 4 shards");
    st = ok; st.has_mask = true;
    expect_msg(call(st, 0, 2, rows, 3, nullptr, cuts, 2, max_n, gi, gj, reach), 3, msg, "reo_top_pairs_null compares on the bit planes of the whole matrix");
    st = ok; st.G = 65536;
    expect_msg(call(st, 0, 2, rows, 3, nullptr, cuts, 2, max_n, gi, gj, reach), 4, msg, "G = 65536, at most 65535 genes");
    st = ok; st.S = 70000;
    expect_msg(call(st, 0, 2, rows, 3, nullptr, cuts, 2, max_n, gi, gj, reach), 5, msg, "S = 70000, at most 65535 samples");
    expect_msg(call(ok, 3, 2, rows, 3, nullptr, cuts, 2, max_n, gi, gj, reach), 6, msg, "a = 3 is outside the groups [0, 3)");
    expect_msg(call(ok, 0, 3, rows, 3, nullptr, cuts, 2, max_n, gi, gj, reach), 7, msg, "b = 3 is outside the groups");
    expect_msg(call(ok, 2, 2, rows, 3, nullptr, cuts, 2, max_n, gi, gj, reach), 8, msg, "reo_top_pairs_null: b == a == 2");
    // its own
    expect_msg(call(ok, 0, 2, rows, 0, nullptr, cuts, 2, max_n, gi, gj, reach), 9, msg, "n_perm = 0, between 1 and 2^20");
    expect_msg(call(ok, 0, 2, rows, (1 << 20) + 1, nullptr, cuts, 2, max_n, gi, gj, reach), 9, msg, "n_perm = 1048577");
    expect_msg(call(ok, 0, 2, rows, 3, nullptr, cuts, -1, max_n, gi, gj, reach), 10, msg, "n_cuts = -1, between 0 and 8");
    expect_msg(call(ok, 0, 2, rows, 3, nullptr, cuts, 9, max_n, gi, gj, reach), 10, msg, "n_cuts = 9");
    expect_msg(call(ok, 0, 2, nullptr, 3, nullptr, cuts, 2, max_n, gi, gj, reach), 11, msg, "must not be null");
    expect_msg(call(ok, 0, 2, rows, 3, nullptr, cuts, 2, nullptr, gi, gj, reach), 11, msg, "must not be null");
    expect_msg(call(ok, 0, 2, rows, 3, nullptr, cuts, 2, max_n, nullptr, gj, reach), 11, msg, "must not be null");
    expect_msg(call(ok, 0, 2, rows, 3, nullptr, cuts, 2, max_n, gi, nullptr, reach), 11, msg, "must not be null");
    expect_msg(call(ok, 0, 2, rows, 3, nullptr, cuts, 2, max_n, gi, gj, nullptr), 11, msg, "nor cuts and n_reach with n_cuts = 2");
    expect_msg(call(ok, 0, 2, rows, 3, nullptr, nullptr, 2, max_n, gi, gj, reach), 11, msg, "nor cuts and n_reach with n_cuts = 2");
    int64_t neg[2] = {4, -1};
    expect_msg(call(ok, 0, 2, rows, 3, nullptr, neg, 2, max_n, gi, gj, reach), 12, msg, "cuts[1] = -1, a cut of |N| is not negative");
    const int32_t one[12] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};
    expect_msg(tn_check_args(ok, one, 1, -1, rows, 3, nullptr, cuts, 2, max_n, gi, gj, reach, &s_a, &s_b, msg, sizeof msg), 14, msg,
               "side A has 12 samples and side B 0, both sides need at least one");
    uint8_t bad[3 * 12];
    memcpy(bad, rows, sizeof bad);
    bad[2 * 12 + 7] = 3;
    expect_msg(call(ok, 0, 2, bad, 3, nullptr, cuts, 2, max_n, gi, gj, reach), 15, msg, "row 2 of sides holds the byte 3 in column 7");
    memcpy(bad, rows, sizeof bad);
    bad[12 + 2] = 0;                                                                        // a sample of group 1 takes part
    expect_msg(call(ok, 0, 2, bad, 3, nullptr, cuts, 2, max_n, gi, gj, reach), 16, msg, "row 1 of sides holds the byte 0 in column 2, whose sample is on neither side");
    memcpy(bad, rows, sizeof bad);
    bad[0] = 2;                                                                             // a sample of group 0 takes no part
    expect_msg(call(ok, 0, 2, bad, 3, nullptr, cuts, 2, max_n, gi, gj, reach), 16, msg, "row 0 of sides holds the byte 2 in column 0, whose sample is on one of the sides");
    memcpy(bad, rows, sizeof bad);
    bad[2 * 12 + 4] = 1;                                                                    // a zero became a one
    expect_msg(call(ok, 0, 2, bad, 3, nullptr, cuts, 2, max_n, gi, gj, reach), 17, msg, "row 2 of sides has 5 ones and 2 zeros, side A has 4 samples and side B 3");
    expect(call(ok, 0, 2, bad, 2, nullptr, cuts, 2, max_n, gi, gj, reach) == 0, "the rows in front of the wrong one are in order");
    mask[299] = 2;
    expect_msg(call(ok, 0, 2, rows, 3, mask, cuts, 2, max_n, gi, gj, reach), 18, msg, "gene_mask[299] = 2");
}

void check_rows()
{
    uint8_t obs[12];
    for (int s = 0; s < 12; ++s) obs[s] = tn_column_byte(kGid[s], 1, 2, 3);
    const uint8_t want[12] = {2, 2, 1, 1, 0, 0, 2, 1, 0, 2, 1, 1};
    expect(memcmp(obs, want, 12) == 0, "group 1 against group 2");
    expect(tn_column_byte(-1, 0, -1, 3) == 2 && tn_column_byte(3, 0, -1, 3) == 2 && tn_column_byte(2, 0, -1, 3) == 0, "labels outside the groups take no part");
    int64_t at = 0, got = 0;
    expect(tn_check_row(obs, obs, 12, 5, &at, &got) == 0, "the observed row");
    uint8_t row[12];
    memcpy(row, obs, 12);
    std::swap(row[2], row[4]);
    expect(tn_check_row(row, obs, 12, 5, &at, &got) == 0, "a shuffle");
    row[11] = 9;
    expect(tn_check_row(row, obs, 12, 5, &at, &got) == 1 && at == 11 && got == 9, "a byte above 2", at, got);
    memcpy(row, obs, 12);
    std::swap(row[0], row[2]);
    expect(tn_check_row(row, obs, 12, 5, &at, &got) == 2 && at == 0 && got == 1, "a 2 moved: the first differing column", at, got);
    memcpy(row, obs, 12);
    row[4] = 1;
    expect(tn_check_row(row, obs, 12, 5, &at, &got) == 3 && at == -1 && got == 6, "six ones", at, got);
}

void check_words()
{
    // 100 samples of three groups, interleaved (34, 33, 33); the slots group by group, every group padded to whole blocks of 32: group 0 in
    // blocks 0 and 1, group 1 in blocks 2 and 3, group 2 in blocks 4 and 5 -- each second block holds one or two columns and padding
    const int S = 100, nblk = 6;
    std::vector<int32_t> gid(S), map(nblk * 32, -1);
    for (int s = 0; s < S; ++s) gid[s] = s % 3;
    int at[3] = {0, 64, 128};
    for (int s = 0; s < S; ++s) map[at[gid[s]]++] = s;
    for (int a = 0; a < 3; ++a)
        for (int b = -1; b < 3; ++b) {
            if (b == a) continue;
            std::vector<uint8_t> obs(S), row(S);
            for (int s = 0; s < S; ++s) obs[s] = tn_column_byte(gid[s], a, b, 3);
            row = obs;
            for (int s = S - 1; s > 0; --s) {   // a shuffle among the samples that take part
                const int t = static_cast<int>(rnd() % static_cast<uint64_t>(s + 1));
                if (row[s] != 2 && row[t] != 2) std::swap(row[s], row[t]);
            }
            int n_live = 0, n_a = 0, part = 0, ones = 0;
            for (int s = 0; s < S; ++s) { part += obs[s] != 2; ones += obs[s] == 1; }
            for (int blk = 0; blk < nblk; ++blk) {
                const uint32_t live = tn_live_word(row.data(), S, map.data() + blk * 32), all = pn_live_word(S, map.data() + blk * 32);
                const uint32_t aw = pn_side_word(row.data(), S, map.data() + blk * 32);
                expect(live == tn_live_word(obs.data(), S, map.data() + blk * 32), "every row gives the same live word", a, b);
                expect((live & ~all) == 0 && (aw & ~live) == 0, "A inside live inside the slots with a column", a, b);
                for (int sl = 0; sl < 32; ++sl) {
                    const int col = map[blk * 32 + sl];
                    const bool lv = (live >> sl) & 1u, av = (aw >> sl) & 1u;
                    expect(lv == (col >= 0 && row[col] != 2) && av == (col >= 0 && row[col] == 1), "bit by bit", blk, sl);
                }
                n_live += __builtin_popcount(live); n_a += __builtin_popcount(aw);
            }
            expect(n_live == part && n_a == ones, "the words count the sides", n_live, n_a);
            if (b >= 0) {   // the blocks of the third group are dead
                const int third = 3 - a - b, first_blk[4] = {0, 2, 4, 6};
                for (int blk = first_blk[third]; blk < first_blk[third + 1]; ++blk)
                    expect(tn_live_word(row.data(), S, map.data() + blk * 32) == 0, "a block of the group on neither side", third, blk);
            }
        }
    // where the words lie: [launch group][block][kPermQ]
    expect(pn_word_count(1, nblk) == static_cast<size_t>(nblk) * kPermQ && pn_word_count(17, nblk) == static_cast<size_t>(2 * nblk) * kPermQ, "whole launch groups");
    expect(pn_word_index(0, 0, nblk) == 0 && pn_word_index(15, 3, nblk) == 3 * kPermQ + 15 && pn_word_index(16, 0, nblk) == static_cast<size_t>(nblk) * kPermQ,
           "permutation 16 opens the second group");
    expect(pn_word_index(kTnBatchCap - 1, nblk - 1, nblk) == pn_word_count(kTnBatchCap, nblk) - 1, "the last word of a full batch");
}

void check_key()
{
    int64_t m = 0;
    int32_t i = 0, j = 0;
    tn_unpack(0, 300, &m, &i, &j);
    expect(m == -1 && i == -1 && j == -1, "key 0: no pair");
    expect(tn_key(0, 65533, 65534, 65535) != 0, "the last pair of the largest problem at |N| = 0 has a key");
    expect(tn_key(0, 65533, 65534, 65535) == 0xFFFFFFFFull - (65533ull * 65535ull + 65534ull), "its index field");
    expect(tn_key(0x7FFFFFFFull, 0, 1, 2) >> 63 == 0, "63 bits");
    struct Pair { uint64_t n; int i, j; };
    for (const int G : {2, 300, 4096, 65535}) {
        std::vector<Pair> ps;
        for (int t = 0; t < 400; ++t) {
            int a = static_cast<int>(rnd() % static_cast<uint64_t>(G)), b = static_cast<int>(rnd() % static_cast<uint64_t>(G));
            if (a == b) { a = 0; b = G - 1; }
            ps.push_back(Pair{rnd() % 5 == 0 ? 0x7FFFFFFFull : rnd() % 7, std::min(a, b), std::max(a, b)});
        }
        for (const Pair &p : ps) {
            const uint64_t k = tn_key(p.n, p.i, p.j, G);
            tn_unpack(k, G, &m, &i, &j);
            expect(k != 0 && m == static_cast<int64_t>(p.n) && i == p.i && j == p.j, "the fields come back", i, j);
        }
        for (size_t x = 0; x + 1 < ps.size(); ++x) {
            const Pair &p = ps[x], &q = ps[x + 1];
            const bool first = p.n != q.n ? p.n > q.n : (p.i != q.i ? p.i < q.i : p.j < q.j);
            const bool same = p.n == q.n && p.i == q.i && p.j == q.j;
            const uint64_t kp = tn_key(p.n, p.i, p.j, G), kq = tn_key(q.n, q.i, q.j, G);
            expect(same ? kp == kq : (first ? kp > kq : kp < kq), "a larger key is a larger |N| or an earlier pair", static_cast<long>(x), G);
        }
    }
}

void check_batch()
{
    expect(tn_batch(1000, 0) == 64 && tn_batch(1000, -3) == 64, "the cap");
    expect(tn_batch(1000, 20) == 20 && tn_batch(1000, 1) == 1 && tn_batch(1000, 500) == 64, "the environment can only lower it");
    expect(tn_batch(17, 0) == 17 && tn_batch(17, 16) == 16 && tn_batch(1, 64) == 1, "never more than the permutations");
    expect(kTnBatchCap % kPermQ == 0 && kTnMaxCuts == 8 && kTnMaxPerms == 1 << 20, "the constants of the header");
}

}  // namespace

int main()
{
    check_args();
    check_rows();
    check_words();
    check_key();
    check_batch();
    if (g_fail) { fprintf(stderr, "%ld of %ld checks failed\n", g_fail, g_checks); return 1; }
    printf("ok %ld\n", g_checks);
    return 0;
}
