// Host-only driver for csrc/masked_pairs.h (tests/test_masked_pairs_cpu.py builds it with -fsanitize=address,undefined and runs it): the
// functions that the kernels of csrc/maskedpairs.hip share with the host, and the checks that reo_set_valid_mask, reo_build_pairs_masked and
// reo_pair_counts_masked run before anything is uploaded.
//   - mp_side_class against a table of hand cases: n below, at and above min_complete; a = m(n); n - a = m(n); n = 0; n = 1;
//   - mp_valid_word on masks of exactly G x S bytes (a read past them is the sanitizer's to report): padding slots, genes >= G, a group of
//     exactly 32 samples, interleaved columns;
//   - mp_count_block for hand words and seeded random ones against a loop over the bits;
//   - reo_lower_count / mp_threshold_table: "thr <pval> <n> <m>" lines for the sizes the test compares with tests/golden/thresholds.json,
//     the table equal to the function entry by entry, pval_reo = 1 has no table; mp_first_informative_n;
//   - every argument check with its number and message.
// Prints the thr lines and "ok <checks>"; anything on stderr is a failure.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "masked_pairs.h"

namespace {

long g_checks = 0, g_fail = 0;

uint64_t g_state = 0x243F6A8885A308D3ULL;
uint32_t rnd()   // splitmix64, seeded: the same words on every run
{
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return static_cast<uint32_t>((z ^ (z >> 31)) >> 16);
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
}

void side_class_cases()
{
    // {a, n, m, min_complete, class}
    const int cases[][5] = {
        {0, 0, 0, 1, 2},     // n = 0: short, although a >= m(0) = 0 would read "stable"
        {1, 1, 1, 1, 3},     // n = 1 with min_complete 1: the fallback threshold m(1) = 1, unanimous
        {0, 1, 1, 1, 1},
        {1, 1, 1, 2, 2},     // n = 1 below min_complete
        {3, 3, 3, 8, 2},     // never "stable by unanimity of three samples"
        {7, 7, 7, 8, 2},     // one below min_complete
        {8, 8, 8, 8, 3},     // at min_complete, a = m(n)
        {0, 8, 8, 8, 1},     // n - a = m(n)
        {7, 8, 8, 8, 2},     // no majority
        {1, 8, 8, 8, 2},
        {10, 11, 11, 8, 2},  // above min_complete, one short of m(n)
        {11, 11, 11, 8, 3},
        {24, 32, 24, 8, 3},  // a = m(32) at 0.01
        {23, 32, 24, 8, 2},
        {8, 32, 24, 8, 1},   // n - a = m(n)
        {9, 32, 24, 8, 2},
        {30, 32, 24, 33, 2}, // min_complete above the side
    };
    for (const auto &c : cases) expect(reo::mp_side_class(c[0], c[1], c[2], c[3]) == c[4], "side class", c[0], c[1]);
    for (int ic = 1; ic <= 3; ++ic)
        for (int it = 1; it <= 3; ++it) {
            const uint32_t code = reo::mp_pair_code(ic, it);
            expect(code == static_cast<uint32_t>(3 * (ic - 1) + (it - 1)), "pair code");
            expect(reo::mp_pair_code(reo::mp_mirror_side(ic), reo::mp_mirror_side(it)) == 8 - code, "the mirrored pair has 8 minus the code");
        }
}

void valid_word_cases()
{
    // two groups, 32 and 5 samples, columns interleaved: slots 0 .. 31 group 0 (no padding), 32 .. 63 group 1 (27 padding slots)
    const int64_t G = 7, S = 37;
    std::vector<int32_t> gid(S), slot2col(64, -1);
    int n0 = 0, n1 = 0;
    for (int64_t s = 0; s < S; ++s) {
        const int g = (s % 2 == 1 && n1 < 5) ? 1 : 0;
        gid[static_cast<size_t>(s)] = g;
        if (g == 0) slot2col[static_cast<size_t>(n0++)] = static_cast<int32_t>(s);
        else slot2col[static_cast<size_t>(32 + n1++)] = static_cast<int32_t>(s);
    }
    expect(n0 == 32 && n1 == 5, "a group of exactly 32 samples", n0, n1);
    std::vector<uint8_t> valid(static_cast<size_t>(G * S));   // exactly G x S bytes
    for (auto &b : valid) b = static_cast<uint8_t>((rnd() & 3) ? (1 + (rnd() & 0x7F)) : 0);   // nonzero = observed, any nonzero value
    for (int64_t s = 0; s < S; ++s) { valid[static_cast<size_t>(s * G + 0)] = 1; valid[static_cast<size_t>(s * G + 1)] = 0; }
    for (int64_t gene = 0; gene < G; ++gene)
        for (int b = 0; b < 2; ++b) {
            const uint32_t w = reo::mp_valid_word(valid.data(), G, S, gene, slot2col.data() + 32 * b);
            uint32_t want = 0;
            for (int s = 0; s < 32; ++s) {
                const int32_t col = slot2col[static_cast<size_t>(32 * b + s)];
                if (col >= 0 && valid[static_cast<size_t>(col * G + gene)]) want |= 1u << s;
            }
            expect(w == want, "validity word", static_cast<long>(gene), b);
            if (b == 1) expect((w >> 5) == 0, "padding slots are 0", static_cast<long>(gene));
        }
    expect(reo::mp_valid_word(valid.data(), G, S, 0, slot2col.data()) == 0xFFFFFFFFu, "a complete gene, a full block");
    expect(reo::mp_valid_word(valid.data(), G, S, 0, slot2col.data() + 32) == 0x1Fu, "a complete gene, five slots");
    expect(reo::mp_valid_word(valid.data(), G, S, 1, slot2col.data()) == 0u, "a gene never observed");
    expect(reo::mp_valid_word(valid.data(), G, S, G, slot2col.data()) == 0u, "gene G is padding");
    expect(reo::mp_valid_word(valid.data(), G, S, 1023, slot2col.data()) == 0u, "genes past G are padding");
    expect(reo::mp_valid_word(valid.data(), G, S, -1, slot2col.data()) == 0u, "a negative gene");
    std::vector<int32_t> wild(32, -1);
    wild[3] = static_cast<int32_t>(S);       // a column outside the matrix is never read
    wild[4] = static_cast<int32_t>(S - 1);
    expect(reo::mp_valid_word(valid.data(), G, S, 0, wild.data()) == (1u << 4), "columns outside [0, S) read as invalid");
}

void count_block_cases()
{
    uint32_t gt = 0, eq = 0, n = 0;
    reo::mp_count_block(0xFFFFFFFFu, 0xFFFFFFFFu, 0u, gt, eq, n);
    expect(gt == 0 && eq == 0 && n == 0, "nothing valid, nothing counted");
    reo::mp_count_block(0x0000000Fu, 0x000000FFu, 0xFFFFFFFFu, gt, eq, n);
    expect(gt == 4 && eq == 4 && n == 32, "all valid", static_cast<long>(gt), static_cast<long>(eq));
    reo::mp_count_block(0x0000000Fu, 0x000000FFu, 0x00000033u, gt, eq, n);
    expect(gt == 6 && eq == 6 && n == 36, "the counts add up over blocks", static_cast<long>(gt), static_cast<long>(eq));
    for (int t = 0; t < 2000; ++t) {
        const uint32_t lt0 = rnd() ^ (rnd() << 16), le = lt0 | (rnd() ^ (rnd() << 16)), v = rnd() ^ (rnd() << 16);
        const uint32_t lt = lt0 & le;   // lt implies le
        uint32_t a = 0, b = 0, c = 0, wa = 0, wb = 0, wc = 0;
        reo::mp_count_block(lt, le, v, a, b, c);
        for (int s = 0; s < 32; ++s) {
            if (!((v >> s) & 1u)) continue;
            ++wc;
            if ((lt >> s) & 1u) ++wa;
            else if ((le >> s) & 1u) ++wb;
        }
        expect(a == wa && b == wb && c == wc, "random words", static_cast<long>(t));
    }
}

void threshold_cases()
{
    const double pvals[2] = {0.01, 0.05};
    const int sizes[] = {2, 3, 5, 7, 8, 10, 11, 32, 64, 100, 500, 2000, 4000};
    for (double p : pvals)
        for (int n : sizes) printf("thr %.2f %d %d\n", p, n, reo::reo_lower_count(n, p));
    std::vector<int32_t> m;
    expect(reo::mp_threshold_table(100, 0.01, m) && m.size() == 101, "table of a side of 100 samples");
    for (int n = 0; n <= 100; ++n) expect(m[static_cast<size_t>(n)] == reo::reo_lower_count(n, 0.01), "table entry", n);
    for (int n = 0; n < 8; ++n) expect(m[static_cast<size_t>(n)] == n, "the fallback branch: m(n) = n", n);
    expect(m[8] == 8 && m[11] == 11 && m[12] < 12, "leaving the fallback branch", m[12]);
    expect(reo::mp_threshold_table(0, 0.01, m) && m.size() == 1 && m[0] == 0, "a side of no samples");
    expect(!reo::mp_threshold_table(20, 1.0, m), "pval_reo = 1 has no threshold");
    expect(reo::mp_first_informative_n(0.01) == 8, "n* at 0.01", reo::mp_first_informative_n(0.01));
    expect(reo::mp_first_informative_n(0.05) == 6, "n* at 0.05", reo::mp_first_informative_n(0.05));
    expect(reo::mp_first_informative_n(1.0) == 2, "n* at 1", reo::mp_first_informative_n(1.0));
}

void argument_checks()
{
    char msg[320];
    reo::MpState st{};
    st.multi = false; st.world = 1; st.G = 72; st.S = 80; st.ngroups = 2; st.has_mask = true;
    const int32_t mc[2] = {8, 8};
    expect(reo::mp_check_mask_args(st, 72, 80, 72, msg, sizeof msg) == 0, "mask in order");
    expect(reo::mp_check_mask_args(st, 72, 80, 100, msg, sizeof msg) == 0, "a larger leading dimension");
    reo::MpState none = st; none.G = 0; none.S = 0;
    expect_msg(reo::mp_check_mask_args(none, 72, 80, 72, msg, sizeof msg), 1, msg, "no expression matrix set");
    expect_msg(reo::mp_check_mask_args(st, 72, 81, 72, msg, sizeof msg), 2, msg, "the mask is 72 x 81, the matrix 72 x 80");
    expect_msg(reo::mp_check_mask_args(st, 71, 80, 72, msg, sizeof msg), 2, msg, "the mask is 71 x 80");
    expect_msg(reo::mp_check_mask_args(st, 72, 80, 71, msg, sizeof msg), 3, msg, "leading dimension 71 < G = 72");

    expect(reo::mp_check_build_args(st, 0, 0.01, mc, msg, sizeof msg) == 0, "build in order");
    expect(reo::mp_check_build_args(st, 1, 1.0, mc, msg, sizeof msg) == 0, "pval_reo = 1 passes the range check");
    reo::MpState s2 = st; s2.multi = true;
    expect_msg(reo::mp_check_build_args(s2, 0, 0.01, mc, msg, sizeof msg), 1, msg, "reo_build_pairs_masked is not available on a reo_create_multi context");
    s2 = st; s2.world = 2;
    expect_msg(reo::mp_check_build_args(s2, 0, 0.01, mc, msg, sizeof msg), 2, msg, "sharded context");
    s2 = st; s2.has_mask = false;
    expect_msg(reo::mp_check_build_args(s2, 0, 0.01, mc, msg, sizeof msg), 3, msg, "no validity mask of the matrix's shape (72 x 80)");
    s2 = st; s2.S = 65536;
    expect_msg(reo::mp_check_build_args(s2, 0, 0.01, mc, msg, sizeof msg), 4, msg, "at most 65535 samples");
    s2 = st; s2.G = 65536;
    expect_msg(reo::mp_check_build_args(s2, 0, 0.01, mc, msg, sizeof msg), 5, msg, "at most 65535 genes (the 16-plane layout only)");
    s2 = st; s2.G = 65535; s2.S = 65535;
    expect(reo::mp_check_build_args(s2, 0, 0.01, mc, msg, sizeof msg) == 0, "the largest shape");
    expect_msg(reo::mp_check_build_args(st, 0, 0.01, nullptr, msg, sizeof msg), 6, msg, "min_complete must not be null");
    const int32_t mc0[2] = {0, 8}, mc1[2] = {8, -3};
    expect_msg(reo::mp_check_build_args(st, 0, 0.01, mc0, msg, sizeof msg), 7, msg, "min_complete = (0, 8)");
    expect_msg(reo::mp_check_build_args(st, 0, 0.01, mc1, msg, sizeof msg), 7, msg, "min_complete = (8, -3)");
    expect_msg(reo::mp_check_build_args(st, 0, 0.0, mc, msg, sizeof msg), 8, msg, "pval_reo = 0 is outside (0, 1]");
    expect_msg(reo::mp_check_build_args(st, 0, 1.5, mc, msg, sizeof msg), 8, msg, "outside (0, 1]");
    expect_msg(reo::mp_check_build_args(st, 0, -0.01, mc, msg, sizeof msg), 8, msg, "outside (0, 1]");
    const double nan = __builtin_nan("");
    expect_msg(reo::mp_check_build_args(st, 0, nan, mc, msg, sizeof msg), 8, msg, "outside (0, 1]");
    expect_msg(reo::mp_check_build_args(st, 2, 0.01, mc, msg, sizeof msg), 9, msg, "comparison 2 outside [0,2)");
    expect_msg(reo::mp_check_build_args(st, -1, 0.01, mc, msg, sizeof msg), 9, msg, "comparison -1 outside [0,2)");

    int32_t out[1] = {0};
    expect(reo::mp_check_counts_args(st, 0, 72, 0, 72, out, out, out, msg, sizeof msg) == 0, "counts in order");
    s2 = st; s2.has_mask = false;
    expect_msg(reo::mp_check_counts_args(s2, 0, 72, 0, 72, out, out, out, msg, sizeof msg), 3, msg, "reo_pair_counts_masked: no validity mask");
    s2 = st; s2.world = 4;
    expect_msg(reo::mp_check_counts_args(s2, 0, 72, 0, 72, out, out, out, msg, sizeof msg), 2, msg, "reo_pair_counts_masked is not available on a sharded context");
    expect_msg(reo::mp_check_counts_args(st, 0, 72, 0, 72, out, nullptr, out, msg, sizeof msg), 6, msg, "must not be null");
    expect_msg(reo::mp_check_counts_args(st, 0, 72, 0, 72, out, out, nullptr, msg, sizeof msg), 6, msg, "must not be null");
    expect_msg(reo::mp_check_counts_args(st, 0, 73, 0, 72, out, out, out, msg, sizeof msg), 7, msg, "bad pair block [0,73) x [0,72)");
    expect_msg(reo::mp_check_counts_args(st, 5, 5, 0, 72, out, out, out, msg, sizeof msg), 7, msg, "bad pair block");
    expect_msg(reo::mp_check_counts_args(st, 0, 72, -1, 72, out, out, out, msg, sizeof msg), 7, msg, "bad pair block");
    s2 = st; s2.G = 65535;
    expect_msg(reo::mp_check_counts_args(s2, 0, 65535, 0, 65535, out, out, out, msg, sizeof msg), 8, msg, "at most 2^28 counts per call");
    expect(reo::mp_check_counts_args(s2, 0, 2048, 0, 65535, out, out, out, msg, sizeof msg) == 0, "a row strip fits");

    reo::mp_query_refusal("reo_sample_tests", msg, sizeof msg);
    expect(strstr(msg, "reo_sample_tests") && strstr(msg, "validity mask") && strstr(msg, "reo_set_valid_mask(NULL)"), "the refusal names the call and the mask");
}

}  // namespace

int main()
{
    side_class_cases();
    valid_word_cases();
    count_block_cases();
    threshold_cases();
    argument_checks();
    if (g_fail) return 1;
    printf("ok %ld\n", g_checks);
    return 0;
}
