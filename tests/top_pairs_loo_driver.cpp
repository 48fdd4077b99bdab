// Host-only driver for csrc/top_pairs_loo.h (tests/test_top_pairs_loo_cpu.py builds it with -fsanitize=address,undefined and runs it): the
// functions that reo_top_pairs_loo runs on the host and shares with the kernels of csrc/toppairsloo.hip.
//   - loo_num, loo_shift, loo_outcome against brute force: seeded outcomes of a pair and seeded lo + hi of two genes over small sides; every
//     fold is recounted from scratch without its sample and must give tp_num / tp_shift of the recount; the move of |N| stays within
//     2 max(S_A, S_B), the step of the bound;
//   - loo_before against the packed key of top_pairs.h (tp_pack, tp_before) on seeded triples, equal fields included;
//   - loo_index_key, loo_word_index;
//   - loo_cut, loo_disjoint (a list with repeats, a list that is too short, genes out of range);
//   - loo_capacity, loo_first_records, loo_bytes, loo_check_count with the count and the cut in its messages;
//   - loo_check_args and loo_check_sides: every check with its number and message, the context's refusals under the call's own name.
//   Prints "ok <checks>"; anything on stderr is a failure.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "top_pairs_loo.h"

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

// One pair and two genes over s_a + s_b samples: the outcome of the pair per sample (2 above, 1 tied, 0 below) and lo + hi of both genes.
void fold_arithmetic()
{
    for (int round = 0; round < 60; ++round) {
        const int s_a = 2 + static_cast<int>(rnd() % 7), s_b = 2 + static_cast<int>(rnd() % 7), S = s_a + s_b;
        std::vector<int> out(S), side(S);
        std::vector<int64_t> vi(S), vj(S);
        for (int s = 0; s < S; ++s) {
            side[s] = s < s_a ? 0 : 1;
            out[s] = static_cast<int>(rnd() % 3);
            vi[s] = static_cast<int64_t>(rnd() % 400); vj[s] = static_cast<int64_t>(rnd() % 400);
        }
        const auto count = [&](int skip, TpRec *r, int64_t *sa, int64_t *sb, int64_t sum_i[2], int64_t sum_j[2]) {
            *r = TpRec{3, 7, 0, 0, 0, 0};
            *sa = *sb = 0; sum_i[0] = sum_i[1] = sum_j[0] = sum_j[1] = 0;
            for (int s = 0; s < S; ++s) {
                if (s == skip) continue;
                if (side[s] == 0) { ++*sa; r->gt_a += out[s] == 2; r->eq_a += out[s] == 1; }
                else { ++*sb; r->gt_b += out[s] == 2; r->eq_b += out[s] == 1; }
                sum_i[side[s]] += vi[s]; sum_j[side[s]] += vj[s];
            }
        };
        TpRec full, part;
        int64_t fa, fb, pa, pb, fi[2], fj[2], pi[2], pj[2];
        count(-1, &full, &fa, &fb, fi, fj);
        expect(fa == s_a && fb == s_b, "full sizes");
        const int64_t n_full = tp_num(full.gt_a, full.eq_a, full.gt_b, full.eq_b, fa, fb);
        for (int s = 0; s < S; ++s) {
            count(s, &part, &pa, &pb, pi, pj);
            const uint32_t gt_bit = out[s] == 2, eq_bit = out[s] == 1;
            const int64_t n = loo_num(full, side[s], gt_bit, eq_bit, s_a, s_b);
            expect(n == tp_num(part.gt_a, part.eq_a, part.gt_b, part.eq_b, pa, pb), "N of the fold", s, round);
            const int64_t move = n > n_full ? n - n_full : n_full - n;
            expect(move <= 2 * std::max(s_a, s_b), "one sample moves N by at most 2 max(S)", static_cast<long>(move), round);
            expect(loo_shift(fi[0], fi[1], side[s], vi[s], s_a, s_b) == tp_shift(pi[0], pi[1], pa, pb), "D of the fold, gene i", s, round);
            expect(loo_shift(fj[0], fj[1], side[s], vj[s], s_a, s_b) == tp_shift(pj[0], pj[1], pa, pb), "D of the fold, gene j", s, round);
            expect(loo_outcome(gt_bit, eq_bit) == out[s] - 1, "outcome", s, round);
        }
    }
    expect(loo_outcome(1, 0) == 1 && loo_outcome(0, 1) == 0 && loo_outcome(0, 0) == -1, "the three outcomes");
}

void order()
{
    const int G = 65535;
    for (int round = 0; round < 2000; ++round) {
        uint64_t n[2], g[2];
        int i[2], j[2];
        for (int q = 0; q < 2; ++q) {
            n[q] = rnd() % 5; g[q] = round % 3 ? rnd() % 4 : rnd() >> 16;   // (Gamma below 2^48: what the packed key holds)
            i[q] = static_cast<int>(rnd() % 40); j[q] = i[q] + 1 + static_cast<int>(rnd() % 40);
        }
        if (round % 7 == 0) { n[1] = n[0]; g[1] = g[0]; }
        const bool before = loo_before(n[0], g[0], loo_index_key(i[0], j[0], G), n[1], g[1], loo_index_key(i[1], j[1], G));
        expect(before == tp_before(tp_pack(n[0], g[0], i[0], j[0], G), tp_pack(n[1], g[1], i[1], j[1], G)), "loo_before is the packed key's order", round);
    }
    expect(!loo_before(3, 9, 17, 3, 9, 17), "a pair is not before itself");
    expect(loo_before(4, 0, 1, 3, 99, 99) && loo_before(3, 5, 1, 3, 4, 99) && loo_before(3, 5, 9, 3, 5, 8), "|N|, then Gamma, then the index key");
    expect(loo_index_key(0, 1, 65535) == 0xFFFFFFFEu && loo_index_key(65533, 65534, 65535) > 0, "no index key is 0");
    expect(loo_index_key(2, 5, 100) > loo_index_key(2, 6, 100) && loo_index_key(2, 99, 100) > loo_index_key(3, 4, 100), "(i, j) ascending");
    expect(loo_word_index(0, 5, 1000) == 5 && loo_word_index(3, 999, 1000) == 3999, "[block][candidate]");
    expect(loo_word_index(2047, (1u << 26) - 1, 1u << 26) == static_cast<size_t>(2048) * (size_t(1) << 26) - 1, "no 32-bit wrap");
}

void cut_and_walk()
{
    expect(loo_cut(2000, 33, 31) == 2000 - 132 && loo_cut(100, 33, 31) == 0 && loo_cut(132, 31, 33) == 0 && loo_cut(133, 31, 33) == 1, "T = max(v - 4 max(S), 0)");
    const int32_t gi[8] = {0, 0, 2, 1, 4, 4, 6, 0}, gj[8] = {1, 2, 3, 3, 5, 7, 7, 9};
    int64_t last = -5;
    expect(loo_disjoint(gi, gj, 8, 10, 3, &last) == 3 && last == 4, "(0,1) (2,3) (4,5)", last);
    expect(loo_disjoint(gi, gj, 8, 10, 4, &last) == 4 && last == 6, "the fourth is (6,7)", last);
    expect(loo_disjoint(gi, gj, 8, 10, 5, &last) == 4 && last == 6, "no fifth disjoint pair", last);
    expect(loo_disjoint(gi, gj, 1, 10, 2, &last) == 1 && last == 0, "a list of one");
    expect(loo_disjoint(gi, gj, 0, 10, 2, &last) == 0 && last == -1, "an empty list");
    expect(loo_disjoint(gi, gj, 8, 6, 4, &last) == 3 && last == 4, "genes outside [0, G) are passed over", last);
}

void capacity()
{
    char msg[320];
    expect(loo_capacity(0) == kLooMaxRecords && loo_capacity(-3) == kLooMaxRecords && loo_capacity(500) == 500, "the cap and the environment's");
    expect(loo_capacity(kLooMaxRecords + 1) == kLooMaxRecords, "the environment can only lower it");
    expect(loo_first_records(kLooMaxRecords, 0) == kLooFirstRecords && loo_first_records(1000, 0) == 1000 && loo_first_records(1000, 16) == 16, "the first buffer");
    expect(loo_first_records(kLooMaxRecords, kLooFirstRecords + 5) == kLooFirstRecords, "never above 2^18");
    expect(loo_bytes(10, 4) == 10 * (24 + 32) && sizeof(TpRec) == 24, "records and two words per block");
    expect(loo_check_count(500, 7, 500, 4, 1 << 20, msg, sizeof msg) == 0, "at the cap");
    expect_msg(loo_check_count(501, 7, 500, 4, 1 << 20, msg, sizeof msg), 1, msg, "reo_top_pairs_loo: 501 pairs reach the cut |N| >= 7, at most 500 candidate records per call");
    expect_msg(loo_check_count(500, 9, 1000, 4, 27999, msg, sizeof msg), 2, msg, "500 pairs reach the cut |N| >= 9 and need 28000 bytes of device memory, 27999 are free");
    expect(loo_check_count(500, 9, 1000, 4, 28000, msg, sizeof msg) == 0, "just fits");
    expect(loo_check_count(kLooMaxRecords, 0, kLooMaxRecords, 2048, ~0ull, msg, sizeof msg) == 0, "the largest call: no overflow of the byte count");
}

void check_args()
{
    char msg[320];
    const TpState ok{false, 1, false, 300, 12, 3};
    uint8_t mask[300];
    memset(mask, 1, sizeof mask);
    int32_t gi[1], gj[1];
    int64_t num[1], gam[1], stats[4];
    int8_t out[1], side[1];
    const auto call = [&](const TpState &st, int32_t a, int32_t b, const uint8_t *gm, int32_t kmax) {
        return loo_check_args(st, a, b, gm, kmax, gi, gj, num, gam, out, side, stats, msg, sizeof msg);
    };
    expect(call(ok, 0, 2, nullptr, 1) == 0 && call(ok, 1, -1, mask, 64) == 0, "in order");
    TpState st = ok;
    st.multi = true;
    expect_msg(call(st, 0, 2, nullptr, 5), 1, msg, "reo_top_pairs_loo is not available on a reo_create_multi context");
    st = ok; st.world = 4;
    expect_msg(call(st, 0, 2, nullptr, 5), 2, msg, "reo_top_pairs_loo is not available on a sharded context (reo_set_shard: 4 shards");
    st = ok; st.has_mask = true;
    expect_msg(call(st, 0, 2, nullptr, 5), 3, msg, "reo_top_pairs_loo compares on the bit planes of the whole matrix");
    st = ok; st.G = 65536;
    expect_msg(call(st, 0, 2, nullptr, 5), 4, msg, "G = 65536, at most 65535 genes");
    st = ok; st.S = 65536;
    expect_msg(call(st, 0, 2, nullptr, 5), 5, msg, "S = 65536, at most 65535 samples");
    expect_msg(call(ok, 3, 2, nullptr, 5), 6, msg, "reo_top_pairs_loo: a = 3 is outside the groups [0, 3)");
    expect_msg(call(ok, 0, 3, nullptr, 5), 7, msg, "b = 3 is outside the groups [0, 3) and not -1");
    expect_msg(call(ok, 1, 1, nullptr, 5), 8, msg, "reo_top_pairs_loo: b == a == 1, the two sides must differ");
    expect_msg(call(ok, 0, 2, nullptr, 0), 9, msg, "reo_top_pairs_loo: kmax = 0, between 1 and 64 picks per fold");
    expect_msg(call(ok, 0, 2, nullptr, 65), 9, msg, "kmax = 65, between 1 and 64");
    expect_msg(loo_check_args(ok, 0, 2, nullptr, 5, gi, nullptr, num, gam, out, side, stats, msg, sizeof msg), 10, msg, "must not be null");
    expect_msg(loo_check_args(ok, 0, 2, nullptr, 5, gi, gj, num, gam, out, side, nullptr, msg, sizeof msg), 10, msg, "side and stats must not be null");
    mask[299] = 2;
    expect_msg(call(ok, 0, 2, mask, 5), 11, msg, "reo_top_pairs_loo: gene_mask[299] = 2, a byte of the mask is 0 or 1");
    expect(loo_check_sides(2, 2, msg, sizeof msg) == 0 && loo_check_sides(40, 2, msg, sizeof msg) == 0, "two samples are enough");
    expect_msg(loo_check_sides(1, 20, msg, sizeof msg), 12, msg, "reo_top_pairs_loo: side A has 1 samples, a fold leaves one out: each side needs at least two");
    expect_msg(loo_check_sides(20, 0, msg, sizeof msg), 13, msg, "side B has 0 samples");
}

}  // namespace

int main()
{
    fold_arithmetic();
    order();
    cut_and_walk();
    capacity();
    check_args();
    if (g_fail) { fprintf(stderr, "%ld of %ld checks failed\n", g_fail, g_checks); return 1; }
    printf("ok %ld\n", g_checks);
    return 0;
}
