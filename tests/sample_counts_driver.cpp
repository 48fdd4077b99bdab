// Host-only driver for csrc/sample_counts.h (tests/test_sample_counts_cpu.py builds it with -fsanitize=address,undefined and runs it): the
// functions that the kernel of csrc/samplecounts.hip shares with the host.
//   - sc_counter_add against per-bit integer counting for 1, 2, 63, 64, 65 and 127 additions of seeded random words, into exactly
//     sc_counter_planes(n) planes (a carry out of the last plane or a touch past it is a failure or the sanitizer's to report);
//   - sc_counter_planes at each of those, and at 0, 3, 4, 128;
//   - sc_counter_at / sc_counter_expand against the same integers;
//   - sc_slot_map for interleaved labels (33 / 37), for groups of 1, 31, 32 and 33 samples, and for a label out of range;
//   - sc_batch_rows, and every argument check of sample_counts_check_args with its number and message.
// Prints "adds <n> <planes>" per case and "ok <checks>"; anything on stderr is a failure.
// With the arguments "map <ngroups> <S>" it reads S group ids from stdin instead, checks sc_slot_map on them as above and prints the map
// (tests/test_wide_sample_cases_cpu.py compares it with the numpy restatement of tests/perm_null_cases.py on layouts of 13 and 17 blocks).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sample_counts.h"

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

void run_adds(int n, int kind)
{
    const int planes = reo::sc_counter_planes(n);
    std::vector<uint32_t> c(static_cast<size_t>(planes), 0u);   // exactly the planes that n additions need
    uint32_t want[32] = {0};
    for (int a = 0; a < n; ++a) {
        const uint32_t w = kind == 0 ? rnd() : (kind == 1 ? 0xFFFFFFFFu : (rnd() & rnd()));   // random, every bit every time, sparse
        for (int s = 0; s < 32; ++s) want[s] += (w >> s) & 1u;
        reo::sc_counter_add(c.data(), planes, w);
    }
    uint32_t got[32];
    reo::sc_counter_expand(c.data(), planes, got);
    for (int s = 0; s < 32; ++s) {
        expect(got[s] == want[s], "sc_counter_expand", n, s);
        expect(reo::sc_counter_at(c.data(), planes, s) == want[s], "sc_counter_at", n, s);
    }
    if (kind == 1) expect(want[0] == static_cast<uint32_t>(n), "all-ones words count n", n);
}

void check_map(const std::vector<int32_t> &gid, int ngroups)
{
    std::vector<int32_t> map;
    const int64_t S = static_cast<int64_t>(gid.size());
    expect(reo::sc_slot_map(gid.data(), S, ngroups, map), "sc_slot_map accepts", S, ngroups);
    std::vector<int> size(static_cast<size_t>(ngroups), 0);
    for (int32_t g : gid) ++size[static_cast<size_t>(g)];
    size_t at = 0;
    std::vector<char> seen(gid.size(), 0);
    for (int g = 0; g < ngroups; ++g) {   // group by group: its samples in column order, then padding up to a whole block
        const size_t padded = (static_cast<size_t>(size[g]) + 31) / 32 * 32;
        int32_t last = -1;
        for (size_t k = 0; k < padded; ++k, ++at) {
            if (at >= map.size()) { expect(false, "map too short", g); return; }
            if (k < static_cast<size_t>(size[g])) {
                const int32_t col = map[at];
                const bool ok = col > last && col < S && gid[static_cast<size_t>(col)] == g && !seen[static_cast<size_t>(col)];
                expect(ok, "slot holds the group's next column", g, static_cast<long>(k));
                if (ok) { seen[static_cast<size_t>(col)] = 1; last = col; }
            } else {
                expect(map[at] == -1, "padding slot", g, static_cast<long>(k));
            }
        }
    }
    expect(at == map.size() && map.size() % 32 == 0, "map length", static_cast<long>(map.size()));
}

void run_maps()
{
    std::vector<int32_t> inter;   // 70 samples, labels interleaved 33 / 37: not the identity, pads on both sides
    for (int s = 0; s < 70; ++s) inter.push_back(s < 66 ? s % 2 : 1);
    check_map(inter, 2);
    for (int n : {1, 31, 32, 33}) {
        std::vector<int32_t> gid;
        for (int s = 0; s < n; ++s) gid.push_back(1);
        for (int s = 0; s < 5; ++s) gid.push_back(0);
        for (int s = 0; s < n; ++s) gid.push_back(2);
        check_map(gid, 3);
    }
    std::vector<int32_t> two = {0, 1};
    check_map(two, 2);
    std::vector<int32_t> bad = {0, 2, 1}, map = {7};
    expect(!reo::sc_slot_map(bad.data(), 3, 2, map) && map.size() == 1 && map[0] == 7, "a label outside [0, ngroups) is refused");
    bad[1] = -1;
    expect(!reo::sc_slot_map(bad.data(), 3, 2, map), "a negative label is refused");
}

void expect_check(int want, int64_t G, const int32_t *genes, int64_t n, uint32_t mask, const int32_t *n_gt, const char *needle)
{
    char msg[320] = "";
    const int got = reo::sample_counts_check_args(G, genes, n, mask, n_gt, msg, sizeof msg);
    ++g_checks;
    if (got != want || (want != 0 && !strstr(msg, needle)) || (want != 0 && !strstr(msg, "reo_sample_counts"))) {
        fprintf(stderr, "FAIL sample_counts_check_args: check %d expected %d (\"%s\"), message \"%s\"\n", got, want, needle, msg);
        ++g_fail;
    }
}

void run_checks()
{
    int32_t *genes = new int32_t[3]{4, 0, 4};   // exactly n_genes entries; repeats and any order are fine
    int32_t *n_gt = new int32_t[1];
    expect_check(0, 5, genes, 3, 0x44, n_gt, "");
    expect_check(0, 5, genes, 3, 0x1FF, n_gt, "");
    expect_check(1, 5, nullptr, 3, 0x44, n_gt, "must not be null");
    expect_check(1, 5, genes, 3, 0x44, nullptr, "must not be null");
    expect_check(2, 5, genes, 0, 0x44, n_gt, "n_genes = 0");
    expect_check(2, 5, genes, -1, 0x44, n_gt, "n_genes = -1");
    expect_check(2, 5, genes, (int64_t(1) << 30) + 1, 0x44, n_gt, "2^30");
    expect_check(3, 5, genes, 3, 0, n_gt, "no class");
    expect_check(3, 5, genes, 3, 0x200, n_gt, "bits above 8");
    expect_check(3, 5, genes, 3, 0x80000001u, n_gt, "bits above 8");
    expect_check(4, 4, genes, 3, 0x44, n_gt, "genes[0] = 4 is outside [0, 4)");
    genes[1] = -1;
    expect_check(4, 5, genes, 3, 0x44, n_gt, "genes[1] = -1");
    delete[] genes; delete[] n_gt;
    // batches: the budget, at least one row, never more than the queries, the environment only lowers
    const int64_t fit = reo::kScBudgetBytes / (64 * 4);
    expect(reo::sc_batch_rows(10, 64, 0) == 10, "batch <= queries");
    expect(reo::sc_batch_rows(fit + 5, 64, 0) == fit, "batch from the budget");
    expect(reo::sc_batch_rows(8, 64, 3) == 3, "batch from the environment");
    expect(reo::sc_batch_rows(fit + 5, 64, fit + 1) == fit, "the environment cannot raise the batch");
    expect(reo::sc_batch_rows(8, reo::kScBudgetBytes, -2) == 1, "at least one row");
}

// "map <ngroups> <S>" and S group ids on stdin: the structural checks of check_map on that layout, then sc_slot_map's slots on one line
int print_map(int ngroups, long S)
{
    if (ngroups < 1 || S < 1 || S > (1 << 20)) { fprintf(stderr, "map: bad sizes\n"); return 2; }
    std::vector<int32_t> gid(static_cast<size_t>(S)), map;
    for (long s = 0; s < S; ++s) {
        long v = -1;
        if (scanf("%ld", &v) != 1 || v < 0 || v >= ngroups) { fprintf(stderr, "map: bad group id at %ld\n", s); return 2; }
        gid[static_cast<size_t>(s)] = static_cast<int32_t>(v);
    }
    check_map(gid, ngroups);
    if (g_fail || !reo::sc_slot_map(gid.data(), S, ngroups, map)) { fprintf(stderr, "%ld failures\n", g_fail); return 1; }
    for (size_t t = 0; t < map.size(); ++t) printf(t ? " %d" : "%d", map[t]);
    printf("\nok %ld\n", g_checks);
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc == 4 && !strcmp(argv[1], "map")) return print_map(atoi(argv[2]), atol(argv[3]));
    for (int n : {1, 2, 63, 64, 65, 127}) {
        for (int kind = 0; kind < 3; ++kind) run_adds(n, kind);
        printf("adds %d %d\n", n, reo::sc_counter_planes(n));
    }
    const int np[][2] = {{0, 0}, {1, 1}, {2, 2}, {3, 2}, {4, 3}, {63, 6}, {64, 7}, {65, 7}, {127, 7}, {128, 8}};
    for (const auto &e : np) expect(reo::sc_counter_planes(e[0]) == e[1], "sc_counter_planes", e[0], e[1]);
    expect(reo::kScTileCols / reo::kScLanes == 64 && reo::sc_counter_planes(reo::kScTileCols / reo::kScLanes) <= reo::kScMaxPlanes, "a lane's share of a tile fits the kernel's planes");
    run_maps();
    run_checks();
    if (g_fail) { fprintf(stderr, "%ld failures\n", g_fail); return 1; }
    printf("ok %ld\n", g_checks);
    return 0;
}
