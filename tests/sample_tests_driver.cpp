// Host-only driver for csrc/sample_tests.h (tests/test_sample_tests_cpu.py builds it with -fsanitize=address,undefined and runs it): the
// functions that the kernel of csrc/sampletests.hip shares with the host.
//   - every argument check of sample_tests_check_args with its number and message; st_batch_rows; st_lf_entries;
//   - st_table: the 2 x 2 table and the reported integers from six counts, and its refusals;
//   - st_tails over a log-factorial table of EXACTLY st_lf_entries(G) doubles, G = background size + 1, so that a read past
//     2 (G - 1) is the sanitizer's to report; every read also goes through REO_ST_LF_AT, replaced here by a read that checks
//     0 <= i <= N < entries;
//   - the degenerate tables (an empty J, all tied, u at either end of the support, u at the mode) and a seeded grid with background
//     sizes up to 12, 70, 300 and 4 200.
// Prints "tail <size> <a> <b> <u> <d> <p_up> <p_down>" (hex doubles) per table, for Python to compare with exact tails, and "ok <checks>";
// anything on stderr is a failure.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {
long g_checks = 0, g_fail = 0, g_reads = 0;
inline double lf_at(const double *lf, int64_t i, int64_t N, int64_t entries)
{
    ++g_reads;
    if (i < 0 || i > N || N >= entries) {
        fprintf(stderr, "FAIL lf index %lld with N = %lld and %lld entries\n", (long long)i, (long long)N, (long long)entries);
        ++g_fail;
        return 0.0;
    }
    return lf[i];
}
}  // namespace
#define REO_ST_LF_AT(lf, i, N, entries) lf_at((lf), (i), (N), (entries))

#include "sample_tests.h"

namespace {

uint64_t g_state = 0x13198A2E03707344ULL;
uint32_t rnd()   // splitmix64, seeded: the same tables on every run
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

void expect_check(int want, int64_t G, const int32_t *genes, int64_t n, const double *up, const double *down, const char *needle)
{
    char msg[320] = "";
    const int got = reo::sample_tests_check_args(G, genes, n, up, down, msg, sizeof msg);
    ++g_checks;
    if (got != want || (want != 0 && !strstr(msg, needle)) || (want != 0 && !strstr(msg, "reo_sample_tests"))) {
        fprintf(stderr, "FAIL sample_tests_check_args: check %d expected %d (\"%s\"), message \"%s\"\n", got, want, needle, msg);
        ++g_fail;
    }
}

void run_checks()
{
    int32_t *genes = new int32_t[3]{4, 0, 4};   // exactly n_genes entries; repeats and any order are fine
    double *up = new double[1], *down = new double[1];
    expect_check(0, 5, genes, 3, up, down, "");
    expect_check(1, 5, nullptr, 3, up, down, "must not be null");
    expect_check(1, 5, genes, 3, nullptr, down, "must not be null");
    expect_check(1, 5, genes, 3, up, nullptr, "must not be null");
    expect_check(2, 5, genes, 0, up, down, "n_genes = 0");
    expect_check(2, 5, genes, -1, up, down, "n_genes = -1");
    expect_check(2, 5, genes, (int64_t(1) << 30) + 1, up, down, "2^30");
    expect_check(3, 4, genes, 3, up, down, "genes[0] = 4 is outside [0, 4)");
    genes[1] = -1;
    expect_check(3, 5, genes, 3, up, down, "genes[1] = -1");
    delete[] genes; delete[] up; delete[] down;
    // batches: rows of twice the length in sc_batch_rows' budget, at least one row, never more than the queries, the environment only lowers
    const int64_t fit = reo::kScBudgetBytes / (64 * 8);
    expect(reo::st_batch_rows(10, 64, 0) == 10, "batch <= queries");
    expect(reo::st_batch_rows(fit + 5, 64, 0) == fit, "batch from the budget");
    expect(fit * 64 * 8 <= reo::kScBudgetBytes && fit * 64 * 4 <= reo::kScBudgetBytes, "every buffer of a batch stays under the budget");
    expect(reo::st_batch_rows(8, 64, 3) == 3, "batch from the environment");
    expect(reo::st_batch_rows(8, 64, 1) == 1, "batch of one");
    expect(reo::st_batch_rows(fit + 5, 64, fit + 1) == fit, "the environment cannot raise the batch");
    expect(reo::st_batch_rows(8, reo::kScBudgetBytes, -2) == 1, "at least one row");
    expect(reo::st_lf_entries(1) == 1 && reo::st_lf_entries(2) == 3 && reo::st_lf_entries(4201) == 8401 && reo::st_lf_entries(0) == 1, "st_lf_entries");
    expect(reo::kStMaskAbove == 0x1C0 && reo::kStMaskBelow == 0x007, "the two class masks");
}

void run_tables()
{
    reo::StTable t;
    // G = 10: 5 partners above in the control group (2 of them below the gene in the sample, 1 tied), 3 below (1 above... )
    expect(reo::st_table(10, 5, 3, 2, 1, 1, 0, &t), "st_table accepts");
    expect(t.a == 5 && t.b == 3 && t.u == 3 && t.d == 4 && t.tied == 1 && t.rev_up == 1 && t.rev_down == 2, "st_table fields", (long)t.u, (long)t.d);
    expect(reo::st_table(10, 9, 0, 9, 0, 0, 0, &t) && t.u == 9 && t.d == 0 && t.rev_down == 0, "a full row above");
    expect(reo::st_table(10, 0, 0, 0, 0, 0, 0, &t) && t.a + t.b + t.u + t.d == 0, "an empty background");
    t.a = -7;
    expect(!reo::st_table(10, 5, 5, 0, 0, 0, 0, &t) && t.a == -7, "more partners than G - 1");
    expect(!reo::st_table(10, -1, 3, 0, 0, 0, 0, &t), "a negative count");
    expect(!reo::st_table(10, 5, 3, 4, 2, 0, 0, &t), "more outcomes than partners (A)");
    expect(!reo::st_table(10, 5, 3, 0, 0, 3, 1, &t), "more outcomes than partners (B)");
    expect(!reo::st_table(10, 0x7FFFFFFF, 0x7FFFFFFF, 0, 0, 0, 0, &t), "sums beyond int32");
    expect(!reo::st_table(10, 5, 3, 0x7FFFFFFF, 0x7FFFFFFF, 0, 0, &t), "outcome sums beyond int32");
}

// one table over a log-factorial table sized for background size `size` exactly
void tail(int size, const std::vector<double> &lf, int64_t a, int64_t b, int64_t u, int64_t d)
{
    double up = -1.0, down = -1.0;
    const long before = g_reads;
    reo::st_tails(lf.data(), static_cast<int64_t>(lf.size()), a, b, u, d, &up, &down);
    expect(up >= 0.0 && up <= 1.0 && down >= 0.0 && down <= 1.0, "tails inside [0, 1]", (long)a, (long)u);
    expect(u + d == 0 ? g_reads == before : g_reads == before + 9, "nine table reads per cell");
    printf("tail %d %lld %lld %lld %lld %a %a\n", size, (long long)a, (long long)b, (long long)u, (long long)d, up, down);
}

void run_size(int size)
{
    std::vector<double> lf;
    reo::st_build_lf(size + 1, lf);   // G = size + 1 genes: a background of at most `size` partners, N <= 2 size
    expect(static_cast<int64_t>(lf.size()) == 2 * int64_t(size) + 1 && lf[0] == 0.0 && lf[1] == 0.0, "lf size", size);
    const int64_t J = size;
    // ---- degenerate tables
    tail(size, lf, 0, 0, 0, 0);                       // an empty J
    tail(size, lf, J / 2, J - J / 2, 0, 0);           // all tied
    tail(size, lf, J / 2, J - J / 2, 0, J);           // u = 0: the lower end of the support
    tail(size, lf, J / 2, J - J / 2, J, 0);           // d = 0: u = n, the upper end
    tail(size, lf, 0, J, J, 0);                       // a = 0 and d = 0: the rarest table, 1 / C(2 J, J)
    tail(size, lf, J, 0, 0, J);                       // b = 0 and u = 0: its mirror
    tail(size, lf, 0, J, J / 3, J - J / 3);           // a = 0: u = K
    tail(size, lf, J, 0, J / 3, J - J / 3);           // b = 0: u at the lower end (u - b)
    tail(size, lf, J - 1, 1, J, 0);
    tail(size, lf, 1, J - 1, 0, J);
    {   // u at the mode: floor((n + 1)(K + 1) / (N + 2)) = u with K = a + u
        const int64_t a = (2 * J) / 3, b = J - a, n = J - J / 8, N = a + b + n;
        bool found = false;
        for (int64_t u = 0; u <= n && !found; ++u)
            if (((n + 1) * (a + u + 1)) / (N + 2) == u) { tail(size, lf, a, b, u, n - u); found = true; }
        expect(found, "a table with u at the mode", size);
    }
    // ---- the seeded grid
    const int cases = size > 1000 ? 160 : 240;
    for (int k = 0; k < cases; ++k) {
        const int64_t Jk = (k % 4 == 0) ? J : 1 + rnd() % J;
        const int64_t a = rnd() % (Jk + 1), b = Jk - a;
        const int64_t tied = (k % 3 == 0) ? 0 : rnd() % (Jk / 8 + 1);
        const int64_t n = Jk - tied;
        int64_t u;
        switch (k % 5) {
        case 0: u = rnd() % (n + 1); break;                                    // anywhere
        case 1: u = (a * n) / Jk + rnd() % 5; break;                           // near the null
        case 2: u = (a * n) / Jk - rnd() % 5; break;
        case 3: u = (a * n) / Jk + rnd() % (n / 4 + 1); break;                 // a moderate shift up ...
        default: u = (a * n) / Jk - rnd() % (n / 4 + 1); break;                // ... and down
        }
        if (u < 0) u = 0;
        if (u > n) u = n;
        tail(size, lf, a, b, u, n - u);
    }
    // a table that the lf table was not sized for: refused with NaN before anything is read
    double up = 0.0, down = 0.0;
    const long before = g_reads;
    reo::st_tails(lf.data(), static_cast<int64_t>(lf.size()), J, 1, J, 0, &up, &down);
    expect(up != up && down != down && g_reads == before, "N beyond the table is refused", size);
    reo::st_tails(lf.data(), static_cast<int64_t>(lf.size()), -1, 1, 0, 0, &up, &down);
    expect(up != up && down != down && g_reads == before, "a negative entry is refused", size);
}

}  // namespace

int main()
{
    run_checks();
    run_tables();
    for (int size : {12, 70, 300, 4200}) run_size(size);
    if (g_fail) { fprintf(stderr, "%ld failures\n", g_fail); return 1; }
    printf("ok %ld\n", g_checks);
    return 0;
}
