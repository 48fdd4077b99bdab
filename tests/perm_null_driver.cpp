// Host-only driver for csrc/perm_null.h (tests/test_perm_null_cpu.py builds it with -fsanitize=address,undefined and runs it): the functions
// that the kernels of csrc/permpairs.hip share with the host, and the checks that reo_perm_null and reo_perm_codes run before anything is
// touched.
//   - "words": reads  S B ngroups / the group ids / B label rows  from stdin, builds the slot map with sc_slot_map (sample_counts.h) and prints
//     the live words and every row's A-words (pn_side_word, pn_live_word through pn_word_index's layout) for the test to compare with its
//     numpy restatement; the rows are allocated at exactly B x S bytes (a read past them is the sanitizer's to report);
//   - pn_check_row: a wrong count of ones, a byte other than 0 / 1, the place and the value it reports;
//   - pn_exceeds at equality, at delta1 = 0, with signs and with NaN;
//   - pn_batch_tables: memory bound, cap, environment cap, n_perm, nothing fits;
//   - every argument check with its number and message.
// Prints "ok <checks>"; anything on stderr is a failure.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "perm_null.h"
#include "sample_counts.h"

namespace {

long g_checks = 0, g_fail = 0;

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

int words_mode()
{
    long S = 0, B = 0, ng = 0;
    if (scanf("%ld %ld %ld", &S, &B, &ng) != 3 || S < 1 || B < 1 || ng < 1) return 2;
    std::vector<int32_t> gid(static_cast<size_t>(S));
    for (auto &g : gid) { int v; if (scanf("%d", &v) != 1) return 2; g = v; }
    std::vector<uint8_t> rows(static_cast<size_t>(S * B));   // exactly B x S bytes
    for (auto &r : rows) { int v; if (scanf("%d", &v) != 1) return 2; r = static_cast<uint8_t>(v); }
    std::vector<int32_t> map;
    if (!reo::sc_slot_map(gid.data(), S, static_cast<int>(ng), map)) return 3;
    const int64_t nblk = static_cast<int64_t>(map.size()) / 32;
    std::vector<uint32_t> aw(reo::pn_word_count(B, nblk), 0u);
    for (int64_t p = 0; p < B; ++p)
        for (int64_t b = 0; b < nblk; ++b) aw[reo::pn_word_index(p, b, nblk)] = reo::pn_side_word(rows.data() + p * S, S, map.data() + 32 * b);
    printf("live");
    for (int64_t b = 0; b < nblk; ++b) printf(" %u", reo::pn_live_word(S, map.data() + 32 * b));
    printf("\n");
    for (int64_t p = 0; p < B; ++p) {
        printf("row");
        for (int64_t b = 0; b < nblk; ++b) printf(" %u", aw[reo::pn_word_index(p, b, nblk)]);
        printf("\n");
    }
    // rows past B inside the last launch group were never written: still 0
    for (int64_t p = B; p < (B + reo::kPermQ - 1) / reo::kPermQ * reo::kPermQ; ++p)
        for (int64_t b = 0; b < nblk; ++b) expect(aw[reo::pn_word_index(p, b, nblk)] == 0u, "padding rows of the last group stay 0", p, b);
    return g_fail ? 1 : 0;
}

void row_checks()
{
    const uint8_t ok[6] = {1, 0, 1, 0, 0, 1}, few[6] = {1, 0, 0, 0, 0, 1}, many[6] = {1, 1, 1, 0, 1, 1}, two[6] = {1, 0, 2, 0, 0, 1}, ff[6] = {0, 0, 0, 0, 0, 255};
    int64_t at = -7, got = -7;
    expect(reo::pn_check_row(ok, 6, 3, &at, &got) == 0, "a row in order");
    expect(reo::pn_check_row(few, 6, 3, &at, &got) == 2 && got == 2 && at == -1, "too few ones", static_cast<long>(got));
    expect(reo::pn_check_row(many, 6, 3, &at, &got) == 2 && got == 5, "too many ones", static_cast<long>(got));
    expect(reo::pn_check_row(two, 6, 3, &at, &got) == 1 && at == 2 && got == 2, "the byte 2 (its ones would have added up)", static_cast<long>(at));
    expect(reo::pn_check_row(ff, 6, 0, &at, &got) == 1 && at == 5 && got == 255, "the byte 255", static_cast<long>(at));
    expect(reo::pn_check_row(ok, 0, 0, &at, &got) == 0, "an empty row has no ones");
    // words: a byte other than 1 never sets a bit, whatever the check said
    int32_t map[32];
    for (int s = 0; s < 32; ++s) map[s] = s < 6 ? 5 - s : -1;   // slots in reverse column order, 26 padding slots
    expect(reo::pn_side_word(ok, 6, map) == 0x29u, "reverse slot order", reo::pn_side_word(ok, 6, map));
    expect(reo::pn_side_word(two, 6, map) == 0x21u, "the byte 2 sets no bit");
    expect(reo::pn_live_word(6, map) == 0x3Fu, "six live slots");
    map[7] = 6;   // a column outside [0, S) is never read
    expect(reo::pn_live_word(6, map) == 0x3Fu && reo::pn_side_word(ok, 6, map) == 0x29u, "columns outside [0, S) are padding");
    expect((reo::pn_side_word(ok, 6, map) & ~reo::pn_live_word(6, map)) == 0u, "A is a subset of live");
}

void exceed_cases()
{
    expect(reo::pn_exceeds(0.25, 0.25), "equality counts");
    expect(reo::pn_exceeds(-0.25, 0.25) && reo::pn_exceeds(0.25, -0.25), "the sign does not matter");
    expect(reo::pn_exceeds(0.0, 0.0) && reo::pn_exceeds(-0.0, 0.0), "0 against 0 counts");
    expect(!reo::pn_exceeds(0.0, 1e-300), "0 does not reach the smallest observed shift");
    expect(reo::pn_exceeds(1e-300, 0.0), "anything reaches an observed 0");
    expect(!reo::pn_exceeds(std::nextafter(0.25, 0.0), 0.25), "one ulp below does not");
    expect(reo::pn_exceeds(std::nextafter(0.25, 1.0), 0.25), "one ulp above does");
    const double nan = __builtin_nan("");
    expect(!reo::pn_exceeds(nan, 0.0) && !reo::pn_exceeds(0.5, nan) && !reo::pn_exceeds(nan, nan), "a NaN never counts");
}

void batch_cases()
{
    const uint64_t tb = 1000;
    expect(reo::pn_batch_tables(100000, tb, 500, 0) == 50, "half of the free memory");
    expect(reo::pn_batch_tables(10000000, tb, 500, 0) == reo::kPermBatchCap, "the cap");
    expect(reo::pn_batch_tables(10000000, tb, 500, 3) == 3, "the environment's cap");
    expect(reo::pn_batch_tables(10000000, tb, 500, 1000) == reo::kPermBatchCap, "an environment cap above the cap");
    expect(reo::pn_batch_tables(10000000, tb, 5, 0) == 5, "no more than n_perm");
    expect(reo::pn_batch_tables(1500, tb, 5, 0) == 1, "one table fits, half the memory does not hold it");
    expect(reo::pn_batch_tables(999, tb, 5, 0) == 0, "not even one table");
    expect(reo::pn_batch_tables(999, 0, 5, 0) == 0, "no table size");
}

void argument_checks()
{
    char msg[320];
    reo::PnState st{};
    st.multi = false; st.world = 1; st.G = 70; st.S = 6; st.ngroups = 2; st.n_labels = 6; st.has_mask = false; st.thr_set = true;
    st.built_k = 0; st.plain_table = true;
    const uint8_t rows[12] = {1, 0, 1, 0, 0, 1, 0, 1, 1, 0, 1, 0};
    const uint8_t bad_count[12] = {1, 0, 1, 0, 0, 1, 0, 1, 0, 0, 1, 0}, bad_byte[12] = {1, 0, 1, 0, 0, 1, 0, 3, 1, 0, 1, 0};
    const uint8_t ref[70] = {1};
    double d[70];
    int32_t n[70];
    auto null_check = [&](const reo::PnState &s, int32_t k, const uint8_t *side, int64_t np) {
        return reo::pn_check_null_args(s, k, side, np, 3, ref, 1.0, 0.05, d, n, n, n, d, msg, sizeof msg);
    };
    expect(null_check(st, 0, rows, 2) == 0, "in order");
    expect_msg(reo::pn_check_null_args(st, 0, rows, 2, 3, nullptr, 1.0, 0.05, d, n, n, n, d, msg, sizeof msg), 10, msg, "must not be null");
    expect_msg(reo::pn_check_null_args(st, 0, rows, 2, 3, ref, 1.0, 0.05, nullptr, n, n, n, d, msg, sizeof msg), 10, msg, "must not be null");
    expect_msg(reo::pn_check_null_args(st, 0, rows, 2, 3, ref, 1.0, 0.05, d, n, n, n, nullptr, msg, sizeof msg), 10, msg, "must not be null");
    expect_msg(null_check(st, 0, nullptr, 2), 10, msg, "must not be null");
    reo::PnState s2 = st; s2.multi = true;
    expect_msg(null_check(s2, 0, rows, 2), 1, msg, "reo_perm_null is not available on a reo_create_multi context");
    s2 = st; s2.world = 2;
    expect_msg(null_check(s2, 0, rows, 2), 2, msg, "sharded context");
    s2 = st; s2.G = 0; s2.S = 0;
    expect_msg(null_check(s2, 0, rows, 2), 3, msg, "no expression matrix");
    s2 = st; s2.n_labels = 5;
    expect_msg(null_check(s2, 0, rows, 2), 3, msg, "group labels of its width");
    s2 = st; s2.has_mask = true;
    expect_msg(null_check(s2, 0, rows, 2), 4, msg, "validity mask");
    s2 = st; s2.S = 65536; s2.n_labels = 65536;
    expect_msg(null_check(s2, 0, rows, 2), 5, msg, "at most 65535 samples");
    s2 = st; s2.G = 65536;
    expect_msg(null_check(s2, 0, rows, 2), 6, msg, "at most 65535 genes (the 16-plane layout only)");
    expect_msg(null_check(st, 2, rows, 2), 7, msg, "comparison 2 outside [0,2)");
    expect_msg(null_check(st, -1, rows, 2), 7, msg, "comparison -1 outside [0,2)");
    s2 = st; s2.thr_set = false;
    expect_msg(null_check(s2, 0, rows, 2), 8, msg, "thresholds not set");
    s2 = st; s2.built_k = -1;
    expect_msg(null_check(s2, 0, rows, 2), 9, msg, "no class table of comparison 0 is resident");
    s2 = st; s2.built_k = 1;
    expect_msg(null_check(s2, 0, rows, 2), 9, msg, "no class table of comparison 0");
    s2 = st; s2.plain_table = false;
    expect_msg(null_check(s2, 0, rows, 2), 9, msg, "a contrast or masked table does not count");
    expect_msg(null_check(st, 0, rows, 0), 11, msg, "n_perm = 0");
    expect_msg(null_check(st, 0, rows, -4), 11, msg, "n_perm = -4");
    expect_msg(null_check(st, 0, bad_byte, 2), 12, msg, "row 1 of side_a holds the byte 3 in column 1");
    expect_msg(null_check(st, 0, bad_count, 2), 13, msg, "row 1 of side_a has 2 ones, side A of the comparison has 3 samples");
    expect(null_check(st, 0, bad_count, 1) == 0, "only the rows of the call are read");
    expect_msg(reo::pn_check_null_args(st, 0, rows, 2, 3, ref, -0.5, 0.05, d, n, n, n, d, msg, sizeof msg), 14, msg, "neither may be negative or NaN");
    expect_msg(reo::pn_check_null_args(st, 0, rows, 2, 3, ref, 1.0, __builtin_nan(""), d, n, n, n, d, msg, sizeof msg), 14, msg, "neither may be negative or NaN");

    uint8_t code[4];
    s2 = st; s2.built_k = -1; s2.plain_table = false;
    expect(reo::pn_check_codes_args(s2, 0, rows, 3, 0, 70, 0, 70, code, msg, sizeof msg) == 0, "reo_perm_codes needs no resident table");
    expect_msg(reo::pn_check_codes_args(st, 0, rows, 3, 0, 70, 0, 70, nullptr, msg, sizeof msg), 10, msg, "side_a and code must not be null");
    expect_msg(reo::pn_check_codes_args(st, 0, rows + 6, 2, 0, 70, 0, 70, code, msg, sizeof msg), 13, msg, "reo_perm_codes: row 0 of side_a has 3 ones");
    expect_msg(reo::pn_check_codes_args(st, 0, rows, 3, 0, 71, 0, 70, code, msg, sizeof msg), 15, msg, "bad pair block [0,71) x [0,70)");
    expect_msg(reo::pn_check_codes_args(st, 0, rows, 3, 5, 5, 0, 70, code, msg, sizeof msg), 15, msg, "bad pair block");
    s2 = st; s2.has_mask = true;
    expect_msg(reo::pn_check_codes_args(s2, 0, rows, 3, 0, 70, 0, 70, code, msg, sizeof msg), 4, msg, "reo_perm_codes compares on the bit planes");
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc > 1 && strcmp(argv[1], "words") == 0) return words_mode();
    row_checks();
    exceed_cases();
    batch_cases();
    argument_checks();
    if (g_fail) return 1;
    printf("ok %ld\n", g_checks);
    return 0;
}
