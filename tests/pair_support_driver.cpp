// Host-only driver for csrc/pair_support.h (tests/test_pair_support_cpu.py builds it with -fsanitize=address,undefined and runs it): the
// functions that reo_pair_support runs on the host before anything is uploaded, and the byte expansion that the kernel of
// csrc/pairsupport.hip shares with the host.
//   - pair_support_check_args: every check with its number and message, on arrays of exactly the listed sizes (a read past them is the
//     sanitizer's to report);
//   - ps_build_items for rows of 0, 1, 63, 64, 65, 128 and 129 entries, for empty rows between full ones, and for batches whose cut lands
//     inside a row (batch sizes 1, 3, 64, 100 and the whole list): the items of all batches together cover every entry exactly once, in
//     order, never span two rows, hold 1 .. 64 entries, carry the row's gene, and offsets count from the batch's first entry;
//   - ps_batch_entries: the budget, the outcome buffer, at least one entry, the environment only lowers;
//   - ps_outcome_byte / ps_outcome_expand for every (lt, le) bit pair that the chain can produce, and for seeded random words.
// Prints "items <row entries> <items>" per single-row case and "ok <checks>"; anything on stderr is a failure.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pair_support.h"

namespace {

long g_checks = 0, g_fail = 0;

uint64_t g_state = 0x13198A2E03707344ULL;
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

// The items of every batch of `batch` entries over the CSR with these row lengths; returns the number of items.
long run_items(const std::vector<int> &len, int64_t batch)
{
    const int64_t n = static_cast<int64_t>(len.size());
    std::vector<int32_t> genes(len.size());
    std::vector<int64_t> rowptr(len.size() + 1, 0);
    for (size_t q = 0; q < len.size(); ++q) { genes[q] = static_cast<int32_t>(1000 + 7 * q); rowptr[q + 1] = rowptr[q] + len[q]; }
    const int64_t total = rowptr[len.size()];
    std::vector<int> row_of(static_cast<size_t>(total));
    for (size_t q = 0; q < len.size(); ++q)
        for (int64_t e = rowptr[q]; e < rowptr[q + 1]; ++e) row_of[static_cast<size_t>(e)] = static_cast<int>(q);
    std::vector<reo::PsItem> items;
    int64_t row = 0, covered = 0;
    long n_items = 0;
    for (int64_t e0 = 0; e0 < total; e0 += batch) {
        const int64_t e1 = e0 + batch < total ? e0 + batch : total;
        reo::ps_build_items(genes.data(), rowptr.data(), n, e0, e1, &row, items);
        expect(!items.empty() && static_cast<int64_t>(items.size()) <= e1 - e0, "a batch has items, no more than entries", static_cast<long>(e0));
        int64_t at = e0;
        const reo::PsItem *prev = nullptr;
        for (const reo::PsItem &it : items) {
            expect(it.count >= 1 && it.count <= reo::kPsLanes, "item holds 1 .. 64 entries", it.count);
            expect(e0 + it.first == at, "items follow each other from the batch's first entry", it.first, static_cast<long>(at - e0));
            expect(it.row >= 0 && it.row < n && it.gene == genes[static_cast<size_t>(it.row)], "item carries its row's gene", it.row);
            bool same = it.first >= 0 && e0 + it.first + it.count <= e1;
            expect(same, "item inside the batch", it.first, it.count);
            if (!same) return n_items;
            for (int k = 0; k < it.count; ++k) same = same && row_of[static_cast<size_t>(e0 + it.first + k)] == it.row;
            expect(same, "item inside one row", it.row);
            if (prev && prev->row == it.row) expect(prev->count == reo::kPsLanes, "only a row's last item of a batch is short", prev->count);
            prev = &it;
            at += it.count;
            ++n_items;
        }
        expect(at == e1, "the batch's items cover its entries", static_cast<long>(at), static_cast<long>(e1));
        expect(row >= 0 && row <= n && (e1 == total || (rowptr[static_cast<size_t>(row)] <= e1 && e1 <= rowptr[static_cast<size_t>(row) + 1])),
               "the row cursor holds the batch's end", static_cast<long>(row));
        covered += at - e0;
    }
    expect(covered == total, "every entry once", static_cast<long>(covered), static_cast<long>(total));
    return n_items;
}

void run_item_cases()
{
    const int single[] = {0, 1, 63, 64, 65, 128, 129};
    const long want[] = {0, 1, 1, 1, 2, 2, 3};
    for (size_t k = 0; k < sizeof single / sizeof single[0]; ++k) {
        // the row alone would be an empty list for 0: put a one-entry row behind it
        std::vector<int> len = {single[k], 1};
        const long got = run_items(len, 1 << 20) - 1;
        expect(got == want[k], "items of a row", single[k], got);
        printf("items %d %ld\n", single[k], got);
    }
    const std::vector<int> mixed = {0, 129, 0, 0, 64, 1, 0, 65, 63, 0, 128, 0};   // empty rows first, last and between full ones
    expect(run_items(mixed, 1 << 20) == 3 + 1 + 1 + 2 + 1 + 2, "items of the mixed list, one batch");
    for (int64_t batch : {1, 3, 64, 100, 450}) run_items(mixed, batch);   // cuts inside rows, at row ends, and the whole list
    expect(run_items(mixed, 1) == 450, "one entry per batch: one item per entry");
    // a cut inside a row: 100 entries of the 129-entry row, then 29 + the rest
    {
        std::vector<int32_t> genes = {5, 9};
        std::vector<int64_t> rowptr = {0, 129, 140};
        std::vector<reo::PsItem> items;
        int64_t row = 0;
        reo::ps_build_items(genes.data(), rowptr.data(), 2, 0, 100, &row, items);
        expect(items.size() == 2 && items[0].count == 64 && items[1].first == 64 && items[1].count == 36 && row == 0, "first batch ends inside row 0");
        reo::ps_build_items(genes.data(), rowptr.data(), 2, 100, 140, &row, items);
        expect(items.size() == 2 && items[0].row == 0 && items[0].first == 0 && items[0].count == 29 && items[0].gene == 5 && items[1].row == 1 &&
                   items[1].first == 29 && items[1].count == 11 && items[1].gene == 9,
               "second batch goes on in row 0, then row 1");
    }
}

void expect_check(int want, int64_t G, const int32_t *genes, int64_t n, const int64_t *rowptr, const int32_t *partner, const int32_t *n_gt,
                  const char *needle)
{
    char msg[320] = "";
    const int got = reo::pair_support_check_args(G, genes, n, rowptr, partner, n_gt, msg, sizeof msg);
    ++g_checks;
    if (got != want || (want != 0 && !strstr(msg, needle)) || (want != 0 && !strstr(msg, "reo_pair_support"))) {
        fprintf(stderr, "FAIL pair_support_check_args: check %d expected %d (\"%s\"), message \"%s\"\n", got, want, needle, msg);
        ++g_fail;
    }
}

void run_checks()
{
    int32_t *genes = new int32_t[3]{4, 0, 4};   // exactly n_genes entries; repeats and any order are fine
    int64_t *rowptr = new int64_t[4]{0, 2, 2, 5};
    int32_t *partner = new int32_t[5]{3, 0, 1, 1, 2};   // unsorted, repeated; row 1 is empty
    int32_t *n_gt = new int32_t[1];
    expect_check(0, 5, genes, 3, rowptr, partner, n_gt, "");
    expect_check(1, 5, nullptr, 3, rowptr, partner, n_gt, "must not be null");
    expect_check(1, 5, genes, 3, nullptr, partner, n_gt, "must not be null");
    expect_check(1, 5, genes, 3, rowptr, partner, nullptr, "must not be null");
    expect_check(2, 5, genes, 0, rowptr, partner, n_gt, "n_genes = 0");
    expect_check(2, 5, genes, -1, rowptr, partner, n_gt, "n_genes = -1");
    expect_check(2, 5, genes, (int64_t(1) << 30) + 1, rowptr, partner, n_gt, "2^30");
    expect_check(3, 4, genes, 3, rowptr, partner, n_gt, "genes[0] = 4 is outside [0, 4)");
    genes[1] = -1;
    expect_check(3, 5, genes, 3, rowptr, partner, n_gt, "genes[1] = -1");
    genes[1] = 0;
    rowptr[0] = 1;
    expect_check(4, 5, genes, 3, rowptr, partner, n_gt, "rowptr[0] = 1");
    rowptr[0] = 0; rowptr[2] = 1;
    expect_check(4, 5, genes, 3, rowptr, partner, n_gt, "rowptr decreases at row 1");
    rowptr[2] = 2;
    expect_check(5, 5, genes, 3, rowptr, nullptr, n_gt, "partner is null and rowptr lists 5 entries");
    {
        int64_t *empty = new int64_t[4]{0, 0, 0, 0};   // no entries at all: a null partner is fine
        expect_check(0, 5, genes, 3, empty, nullptr, n_gt, "");
        delete[] empty;
    }
    partner[3] = 5;
    expect_check(6, 5, genes, 3, rowptr, partner, n_gt, "partner[3] = 5 (row 2) is outside [0, 5)");
    partner[3] = -2;
    expect_check(6, 5, genes, 3, rowptr, partner, n_gt, "partner[3] = -2");
    partner[3] = 4;
    expect_check(7, 5, genes, 3, rowptr, partner, n_gt, "partner[3] = 4 is the gene of its own row 2");
    partner[3] = 1; partner[1] = 4;
    expect_check(7, 5, genes, 3, rowptr, partner, n_gt, "own row 0");
    delete[] genes; delete[] rowptr; delete[] partner; delete[] n_gt;
    // batches
    const int64_t budget = reo::kPsBudgetBytes;
    expect(reo::ps_batch_entries(10, 2, 500, false, 0) == 10, "batch <= entries");
    expect(reo::ps_batch_entries(budget, 2, 500, false, 0) == budget / 8, "batch from the count buffers");
    expect(reo::ps_batch_entries(budget, 2, 500, true, 0) == budget / 500, "batch from the outcome buffer");
    expect(reo::ps_batch_entries(budget, 33, 8, true, 0) == budget / (33 * 4), "many groups: the count buffers again");
    expect(reo::ps_batch_entries(8, 2, 500, true, 3) == 3, "batch from the environment");
    expect(reo::ps_batch_entries(budget, 2, 500, true, budget) == budget / 500, "the environment cannot raise the batch");
    expect(reo::ps_batch_entries(8, 2, budget * 2, true, -2) == 1, "at least one entry");
    expect(reo::ps_batch_entries(budget, 1, 1, true, 0) == (int64_t(1) << 23), "never more than 2^23 entries");
}

void run_outcomes()
{
    // bit by bit: the three pairs the chain can produce (lt implies le)
    expect(reo::ps_outcome_byte(0u, 0u, 0) == 0, "below");
    expect(reo::ps_outcome_byte(0u, 1u, 0) == 1, "tied");
    expect(reo::ps_outcome_byte(1u, 1u, 0) == 2, "above");
    expect(reo::ps_outcome_byte(0x80000000u, 0x80000000u, 31) == 2 && reo::ps_outcome_byte(0x80000000u, 0x80000000u, 30) == 0, "bit 31 alone");
    for (int r = 0; r < 200; ++r) {
        const uint32_t le = r == 0 ? 0u : (r == 1 ? 0xFFFFFFFFu : rnd()), lt = le & (r == 1 ? 0xFFFFFFFFu : rnd());
        uint8_t *out = new uint8_t[32];   // exactly 32 bytes
        reo::ps_outcome_expand(lt, le, out);
        int n2 = 0, n1 = 0;
        for (int s = 0; s < 32; ++s) {
            const int want = ((lt >> s) & 1u) ? 2 : (((le >> s) & 1u) ? 1 : 0);
            expect(out[s] == want, "ps_outcome_expand", r, s);
            n2 += out[s] == 2; n1 += out[s] == 1;
        }
        expect(n2 == __builtin_popcount(lt) && n1 == __builtin_popcount(le) - __builtin_popcount(lt), "the bytes sum to the counts", r);
        delete[] out;
    }
}

}  // namespace

int main()
{
    run_item_cases();
    run_checks();
    run_outcomes();
    if (g_fail) { fprintf(stderr, "%ld failures\n", g_fail); return 1; }
    printf("ok %ld\n", g_checks);
    return 0;
}
