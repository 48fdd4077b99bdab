// Host-only driver for csrc/sample_calls.h (tests/test_sample_calls_cpu.py builds it with -fsanitize=address,undefined and runs it): the
// functions that the kernels of csrc/samplecalls.hip share with the host.
//   - every argument check of sample_calls_check_args with its number and message, and their order; the batch and memory arithmetic;
//   - call_bh_rank against a plain search for the smallest r with p (n / r) <= al over a grid of (p, n, al) that holds p = 0, p = 1,
//     al = 0, al = 1, n = 1 and, at n = 200, p = al k / n for every k with its two neighbours: every rounding boundary of the rule;
//   - the cell word's pack and unpack at n = 1 and at the largest n taken;
//   - call_cut on hand-made histograms;
//   - the whole rule, rank -> histogram -> cut -> call, on seeded columns of n in {1, 2, 17, 200, 5000} rows for sixteen threshold pairs.
// Prints per column "column <id> <n>" and n lines "p <p_up> <p_down>" (hex doubles), then per threshold pair
// "calls <id> <pval_deg> <padj_deg> <cut> <n_up> <n_down> <one of + - 0 per row>", for Python to compare with SampleTests.calls, and
// "ok <checks>"; anything on stderr is a failure.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "sample_calls.h"

namespace {

long g_checks = 0, g_fail = 0;

uint64_t g_state = 0x243F6A8885A308D3ULL;
uint64_t rnd64()   // splitmix64, seeded: the same columns on every run
{
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
double rnd01() { return static_cast<double>(rnd64() >> 11) * 0x1p-53; }

void expect(bool ok, const char *what, long a = 0, long b = 0)
{
    ++g_checks;
    if (!ok) { fprintf(stderr, "FAIL %s (%ld, %ld)\n", what, a, b); ++g_fail; }
}

void expect_check(int want, int64_t G, const int32_t *genes, int64_t n, double a, double b, const int8_t *calls, const char *needle)
{
    char msg[320] = "";
    const int got = reo::sample_calls_check_args(G, genes, n, a, b, calls, msg, sizeof msg);
    ++g_checks;
    if (got != want || (want != 0 && !strstr(msg, needle)) || (want != 0 && !strstr(msg, "reo_sample_calls"))) {
        fprintf(stderr, "FAIL sample_calls_check_args: check %d expected %d (\"%s\"), message \"%s\"\n", got, want, needle, msg);
        ++g_fail;
    }
}

void run_checks()
{
    int32_t *genes = new int32_t[3]{4, 0, 4};   // exactly n_genes entries; repeats and any order are fine
    int8_t *calls = new int8_t[1];
    const double nan = std::nan("");
    expect_check(0, 5, genes, 3, 1.0, 0.05, calls, "");
    expect_check(0, 5, genes, 3, 0.0, 0.0, calls, "");
    expect_check(0, 5, genes, 3, 1.0, 1.0, calls, "");
    expect_check(1, 5, nullptr, 3, 1.0, 0.05, calls, "genes and calls must not be null");
    expect_check(1, 5, genes, 3, 1.0, 0.05, nullptr, "genes and calls must not be null");
    expect_check(2, 5, genes, 0, 1.0, 0.05, calls, "n_genes = 0");
    expect_check(2, 5, genes, -1, 1.0, 0.05, calls, "n_genes = -1");
    expect_check(2, 5, genes, reo::kCallMaxQueries + 1, 1.0, 0.05, calls, "2^29 - 2");
    expect_check(3, 5, genes, 3, nan, 0.05, calls, "pval_deg = nan");
    expect_check(3, 5, genes, 3, -0.1, 0.05, calls, "pval_deg = -0.1");
    expect_check(3, 5, genes, 3, 1.5, 0.05, calls, "pval_deg = 1.5");
    expect_check(4, 5, genes, 3, 1.0, nan, calls, "padj_deg = nan");
    expect_check(4, 5, genes, 3, 1.0, -0.1, calls, "padj_deg = -0.1");
    expect_check(4, 5, genes, 3, 1.0, 1.5, calls, "padj_deg = 1.5");
    expect_check(5, 4, genes, 3, 1.0, 0.05, calls, "genes[0] = 4 is outside [0, 4)");
    // the order: a null array before the count, the count before the thresholds, pval_deg before padj_deg, the thresholds before the genes
    expect_check(1, 4, nullptr, 0, nan, nan, calls, "must not be null");
    expect_check(2, 4, genes, 0, nan, nan, calls, "n_genes = 0");
    expect_check(3, 4, genes, 3, nan, nan, calls, "pval_deg");
    expect_check(4, 4, genes, 3, 0.5, nan, calls, "padj_deg");
    genes[1] = -1;
    expect_check(5, 5, genes, 3, 1.0, 0.05, calls, "genes[1] = -1");
    delete[] genes; delete[] calls;
    expect(reo::kCallMaxQueries == (int64_t(1) << 29) - 2, "the largest n taken");
    expect(reo::call_padded_rows(1) == 32 && reo::call_padded_rows(32) == 32 && reo::call_padded_rows(33) == 64 && reo::call_padded_rows(20000) == 20000, "padded rows");
    expect(reo::call_batch_rows(10, 64, 0) == reo::st_batch_rows(10, 64, 0) && reo::call_batch_rows(8, 64, 3) == 3 && reo::call_batch_rows(8, 64, 1) == 1, "the batch of reo_sample_tests");
    expect(reo::call_batch_rows(1 << 20, 64, 0) == reo::kScBudgetBytes / (64 * 8), "batch from the budget");
    // 20 000 x 1 000 with 1 024 slots: 80 MB of words, 20 MB of calls, and the batch
    const int64_t b = reo::call_batch_rows(20000, 1024, 0);
    expect(reo::call_device_bytes(20000, 1000, 1024, b) == int64_t(80000000) + 20000000 + 80000 + 16000 + b * (8 + 16 * 1024 + 16000) + 4, "device bytes", (long)b);
    expect(reo::call_device_bytes(reo::kCallMaxQueries, 1 << 20, 1 << 20, 1) > 0, "the arithmetic stays inside int64");
}

int32_t plain_rank(double p, int32_t n, double al)
{
    const double nd = static_cast<double>(n);
    for (int32_t r = 1; r <= n; ++r)
        if (p * (nd / static_cast<double>(r)) <= al) return r;
    return n + 1;
}

void rank_case(double p, int32_t n, double al)
{
    const int32_t got = reo::call_bh_rank(p, n, al), want = plain_rank(p, n, al);
    ++g_checks;
    if (got != want) { fprintf(stderr, "FAIL call_bh_rank(%a, %d, %a) = %d, the plain search finds %d\n", p, n, al, got, want); ++g_fail; }
}

void run_ranks()
{
    const double als[] = {0.0, 1.0, 0.05, 0.2, 0.5, 1e-300, 5e-324, 0x1p-52, 0.999};
    const int32_t ns[] = {1, 2, 3, 17, 200, 1000, 5000};
    for (double al : als)
        for (int32_t n : ns) {
            const double ps[] = {0.0, 1.0, 5e-324, 1e-300, 1e-17, al, al / n, std::nextafter(al, 2.0), std::nextafter(al, -1.0), 0.5, 0.05};
            for (double p : ps)
                if (p >= 0.0 && p <= 1.0) rank_case(p, n, al);
            for (int k = 0; k < 40; ++k) { const double u = rnd01(); rank_case(u * u * u, n, al); rank_case(u * al, n, al); }
        }
    // al = 0: rank 1 iff p == 0, else none; p = 0: always rank 1; n = 1: p <= al
    expect(reo::call_bh_rank(0.0, 7, 0.0) == 1 && reo::call_bh_rank(5e-324, 7, 0.0) == 8 && reo::call_bh_rank(1.0, 1, 0.0) == 2, "al = 0");
    expect(reo::call_bh_rank(0.0, 1, 0.05) == 1 && reo::call_bh_rank(0.0, 5000, 1e-300) == 1, "p = 0");
    expect(reo::call_bh_rank(0.05, 1, 0.05) == 1 && reo::call_bh_rank(std::nextafter(0.05, 1.0), 1, 0.05) == 2, "n = 1");
    expect(reo::call_bh_rank(1.0, 200, 1.0) == 200 && reo::call_bh_rank(std::nan(""), 200, 1.0) == 201, "p = 1 at al = 1; a NaN has no rank");
    // every rounding boundary at n = 200: p = al k / n and its two neighbours
    for (double al : {0.05, 0.2, 1.0, 0.0, 0x1p-30})
        for (int k = 0; k <= 200; ++k) {
            const double p = al * k / 200.0;
            rank_case(p, 200, al);
            if (p > 0.0) rank_case(std::nextafter(p, -1.0), 200, al);
            if (p < 1.0) rank_case(std::nextafter(p, 2.0), 200, al);
        }
}

void run_words()
{
    for (int32_t n : {int32_t(1), int32_t(reo::kCallMaxQueries)})
        for (int32_t rank : {int32_t(1), n, n + 1})
            for (uint32_t dir : {0u, reo::kCallUp, reo::kCallDown})
                for (bool ok : {false, true}) {
                    const uint32_t w = reo::call_pack(rank, dir, ok);
                    expect(reo::call_word_rank(w) == rank && reo::call_word_dir(w) == dir && reo::call_word_pval_ok(w) == ok, "pack and unpack", rank, (long)dir);
                    const int8_t want = (ok && rank <= n && dir) ? (dir == reo::kCallUp ? 1 : -1) : 0;
                    expect(reo::call_of(w, n) == want && reo::call_of(w, rank - 1) == 0, "call_of", rank, (long)dir);
                }
    expect(reo::call_pval(0.25, 0.9) == 0.5 && reo::call_pval(0.9, 0.25) == 0.5 && reo::call_pval(0.5, 0.5) == 1.0 && reo::call_pval(0.7, 0.6) == 1.0 &&
           reo::call_pval(0.0, 1.0) == 0.0, "the two-sided value");
    expect(reo::call_direction(0.1, 0.9) == reo::kCallUp && reo::call_direction(0.9, 0.1) == reo::kCallDown && reo::call_direction(0.5, 0.5) == 0, "direction");
}

void run_cuts()
{
    const int32_t n = 9;
    std::vector<int32_t> h(n, 0);   // exactly n bins: a read past the last is the sanitizer's to report
    expect(reo::call_cut(h.data(), n) == 0, "an empty histogram");
    h[0] = n;
    expect(reo::call_cut(h.data(), n) == n, "all in bin 1");
    h[0] = 0; h[n - 1] = n;
    expect(reo::call_cut(h.data(), n) == n, "all in bin n");
    h[n - 1] = n - 1;
    expect(reo::call_cut(h.data(), n) == 0, "one row short in bin n");
    h.assign(n, 1); h[0] = 0;   // H(r) = r - 1 throughout
    expect(reo::call_cut(h.data(), n) == 0, "H(r) = r - 1 throughout");
    h[4] = 2;   // H(r) = r from r = 5 on
    expect(reo::call_cut(h.data(), n) == n, "H(r) = r from 5 on");
    h.assign(n, 0); h[0] = 1; h[2] = 2;   // H = 1 1 3 3 3 ...: r = 1 and r = 3 qualify, 2 does not
    expect(reo::call_cut(h.data(), n) == 3, "the largest r, not the first gap");
    int32_t one = 1;
    expect(reo::call_cut(&one, 1) == 1, "n = 1");
}

struct Column {
    std::vector<double> up, down;
};

// a row with the two-sided value v exactly (v / 2 and its double are exact), the direction drawn; v = 1: equal tails, no direction
void push(Column &c, double v)
{
    const double small = v / 2.0, large = 1.0 - small;
    if (v >= 1.0) { c.up.push_back(0.5); c.down.push_back(rnd64() & 1 ? 0.5 : 1.0); return; }
    if (rnd64() & 1) { c.up.push_back(small); c.down.push_back(large); } else { c.up.push_back(large); c.down.push_back(small); }
}

int g_column = 0;

void emit(const Column &c)
{
    const int32_t n = static_cast<int32_t>(c.up.size());
    const int id = g_column++;
    printf("column %d %d\n", id, n);
    for (int32_t i = 0; i < n; ++i) printf("p %a %a\n", c.up[i], c.down[i]);
    const double thr[] = {0.0, 0.05, 0.2, 1.0};
    std::vector<uint32_t> w(n);
    std::vector<int32_t> hist(n);
    std::string line(n, '0');
    for (double a : thr)
        for (double b : thr) {
            hist.assign(n, 0);
            for (int32_t i = 0; i < n; ++i) {
                w[i] = reo::call_word(c.up[i], c.down[i], n, a, b);
                const int32_t m = reo::call_word_rank(w[i]);
                expect(m >= 1 && m <= n + 1, "a rank in 1 .. n + 1", m, n);
                if (m >= 1 && m <= n) ++hist[m - 1];   // (the test the kernel makes before it indexes)
            }
            const int32_t kstar = reo::call_cut(hist.data(), n);
            int32_t cut = 0, up = 0, down = 0;
            for (int32_t i = 0; i < n; ++i) {
                const int8_t call = reo::call_of(w[i], kstar);
                cut += reo::call_word_rank(w[i]) <= kstar;
                up += call > 0;
                down += call < 0;
                line[i] = call > 0 ? '+' : (call < 0 ? '-' : '0');
            }
            expect(cut == kstar, "the rows within the cut number k*", cut, kstar);
            printf("calls %d %a %a %d %d %d %s\n", id, a, b, cut, up, down, line.c_str());
        }
}

void run_columns()
{
    for (int32_t n : {1, 2, 17, 200, 5000}) {
        Column c;
        for (int32_t i = 0; i < n; ++i) push(c, 0.04);   // all equal: one long tie
        emit(c);
        c = Column();
        for (int32_t i = 0; i < n; ++i) push(c, 0.0);
        emit(c);
        c = Column();
        for (int32_t i = 0; i < n; ++i) push(c, 1.0);
        emit(c);
        for (double al : {0.05, 0.2}) {   // the boundary column: p = al k / n, k = 1 .. n, shuffled by a stride
            c = Column();
            for (int32_t i = 0; i < n; ++i) push(c, al * (1 + (i * 7919LL) % n) / n);
            emit(c);
        }
        c = Column();   // random^3, a tenth of the rows tied at one value
        for (int32_t i = 0; i < n; ++i) { const double u = rnd01(); push(c, rnd64() % 10 == 0 ? 0.03125 : u * u * u); }
        emit(c);
    }
}

}  // namespace

int main()
{
    run_checks();
    run_ranks();
    run_words();
    run_cuts();
    run_columns();
    if (g_fail) { fprintf(stderr, "%ld failures\n", g_fail); return 1; }
    printf("ok %ld\n", g_checks);
    return 0;
}
