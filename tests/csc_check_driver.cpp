// Host-only driver for csrc/csc_check.h (tests/test_csc_device_cpu.py builds it with -fsanitize=address,undefined and runs it): the
// predicates that the kernel csc_validate evaluates on device CSC arrays, run here column by column over containers whose arrays are
// allocated at EXACTLY S + 1 and nnz elements, so that a read which a bad colptr would have caused is the sanitizer's to report.
// Every case is evaluated for int32 and int64 indices and for 1, 3 and 256 workers per column (the kernel's workgroup); the verdict --
// class and lowest offending column -- must be the expected one and must agree with what the host readers of upload_csc.h
// (check_colptr_run, then read_rows column by column) say about the same container.  Prints one line per case and index width:
//   case <name> <bits> <class> <column> ref <class> <column>       (ref - -: the container is not expressible for the host readers)
// and "ok <cases>".
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "csc_check.h"

namespace {

long g_cases = 0, g_fail = 0;

struct Case {
    const char *name;
    int64_t G, nnz;                 // nnz: the ARGUMENT (the length of the row array), not necessarily colptr[S]
    std::vector<int64_t> colptr;
    std::vector<int64_t> rows;      // nnz of them
    int want;                       // CscVerdict
    int64_t at;                     // the lowest offending column (-1: none)
    bool wide_only;                 // holds a value that does not fit 32 bits: int64 indices only, no host reference
};

template <class I>
I *exact(const std::vector<int64_t> &v)   // a heap array of exactly v.size() elements
{
    I *p = new I[v.size()];
    for (size_t i = 0; i < v.size(); ++i) p[i] = static_cast<I>(v[i]);
    return p;
}

// what reo_set_matrix_csc_* decides on the host for the same container: colptr[0], check_colptr_run, colptr[S], read_rows per column
void reference(const Case &k, int *cls, int64_t *at)
{
    const int64_t S = static_cast<int64_t>(k.colptr.size()) - 1;
    int64_t *cp = exact<int64_t>(k.colptr);
    int32_t *ri = exact<int32_t>(k.rows);
    *cls = reo::kCscOk; *at = -1;
    if (cp[0] != 0) { *cls = reo::kCscColptr; *at = 0; }
    else if (reo::check_colptr_run(cp, 0, S, k.G, k.nnz, at) != reo::kCscOk) *cls = reo::kCscColptr;
    else if (cp[S] != k.nnz) { *cls = reo::kCscColptr; *at = S - 1; }
    else {
        *at = -1;
        for (int64_t c = 0; c < S && *cls == reo::kCscOk; ++c) {
            const reo::CscVerdict v = reo::read_rows<int32_t>(cp, c, 1, ri, k.G, 0, cp[c + 1] - cp[c], nullptr);
            if (v != reo::kCscOk) { *cls = v; *at = c; }
        }
    }
    delete[] cp; delete[] ri;
}

template <class I>
void run(const Case &k, int bits)
{
    const int64_t S = static_cast<int64_t>(k.colptr.size()) - 1;
    if (static_cast<int64_t>(k.rows.size()) != k.nnz) { fprintf(stderr, "FAIL %s: the case's row array is not nnz long\n", k.name); ++g_fail; return; }
    I *cp = exact<I>(k.colptr);
    I *ri = exact<I>(k.rows);
    int cls = -1;
    int64_t at = -2;
    for (int stride : {1, 3, 256}) {
        uint64_t worst = reo::kCscClean;
        for (int64_t c = 0; c < S; ++c)
            for (int lane = 0; lane < stride; ++lane) {
                const uint64_t w = reo::csc_check_share<I>(cp, ri, c, S, k.G, k.nnz, lane, stride);
                worst = w < worst ? w : worst;
            }
        const int v = reo::csc_class(worst);
        const int64_t col = v == reo::kCscOk ? -1 : reo::csc_column(worst);
        ++g_cases;
        if (v != k.want || col != k.at) { fprintf(stderr, "FAIL %s (%d bits, %d workers): %d at %" PRId64 ", expected %d at %" PRId64 "\n", k.name, bits, stride, v, col, k.want, k.at); ++g_fail; }
        if (cls != -1 && (cls != v || at != col)) { fprintf(stderr, "FAIL %s (%d bits): the verdict depends on the number of workers\n", k.name, bits); ++g_fail; }
        cls = v; at = col;
    }
    delete[] cp; delete[] ri;
    if (k.wide_only) { printf("case %s %d %d %" PRId64 " ref - -\n", k.name, bits, cls, at); return; }
    int rcls; int64_t rat;
    reference(k, &rcls, &rat);
    ++g_cases;
    if (rcls != cls || rat != at) { fprintf(stderr, "FAIL %s (%d bits): %d at %" PRId64 ", the host readers say %d at %" PRId64 "\n", k.name, bits, cls, at, rcls, rat); ++g_fail; }
    printf("case %s %d %d %" PRId64 " ref %d %" PRId64 "\n", k.name, bits, cls, at, rcls, rat);
}

}  // namespace

int main()
{
    using namespace reo;
    const std::vector<int64_t> cp3 = {0, 3, 7, 9}, rows9 = {1, 5, 9, 0, 2, 3, 4, 3, 8};   // G = 10: descending across both column boundaries (legal)
    auto with = [](std::vector<int64_t> v, size_t i, int64_t x) { v[i] = x; return v; };
    std::vector<int64_t> full;   // one full column of G = 300 rows between an empty and a short one: more entries than 256 workers
    for (int64_t r = 0; r < 300; ++r) full.push_back(r);
    full.push_back(299);
    const std::vector<Case> cases = {
        // ---- valid containers
        {"empty_and_full_columns", 4, 5, {0, 0, 4, 5, 5}, {0, 1, 2, 3, 2}, kCscOk, -1, false},
        {"G2", 2, 3, {0, 2, 2, 3}, {0, 1, 1}, kCscOk, -1, false},
        {"no_entries", 3, 0, {0, 0, 0}, {}, kCscOk, -1, false},
        {"descending_across_columns", 10, 9, cp3, rows9, kCscOk, -1, false},
        {"full_column_of_300", 300, 301, {0, 0, 300, 301}, full, kCscOk, -1, false},
        // ---- row faults
        {"index_equal_G", 10, 9, cp3, with(rows9, 4, 10), kCscRowRange, 1, false},
        {"negative_index", 10, 9, cp3, with(rows9, 8, -1), kCscRowRange, 2, false},
        {"equal_pair", 10, 9, cp3, with(rows9, 5, 2), kCscRowOrder, 1, false},
        {"descending_pair", 10, 9, cp3, with(with(rows9, 5, 4), 6, 3), kCscRowOrder, 1, false},
        {"order_then_range_in_one_column", 100, 3, {0, 3, 3}, {5, 3, 100}, kCscRowOrder, 0, false},
        {"range_then_order_in_one_column", 100, 3, {0, 3, 3}, {5, 100, 3}, kCscRowRange, 0, false},
        {"fault_in_entry_299_of_300", 300, 301, {0, 0, 300, 301}, with(full, 299, 298), kCscRowOrder, 1, false},
        {"two_faulty_columns_the_lower_one", 10, 9, cp3, with(with(rows9, 8, 10), 1, 1), kCscRowOrder, 0, false},
        {"index_2_pow_32_plus_1", 10, 9, cp3, with(rows9, 4, (int64_t(1) << 32) + 1), kCscRowRange, 1, true},   // (its low 32 bits are a valid row)
        // ---- colptr faults: the row array is `nnz` long and must not be read where colptr points outside it
        {"colptr_starts_at_1", 10, 9, {1, 3, 7, 9}, rows9, kCscColptr, 0, false},
        {"colptr_decreasing", 10, 9, {0, 3, 2, 9}, rows9, kCscColptr, 1, false},
        {"colptr_end_beyond_nnz", 10, 9, {0, 3, 7, 14}, rows9, kCscColptr, 2, false},
        {"colptr_end_short_of_nnz", 10, 9, {0, 3, 7, 8}, rows9, kCscColptr, 2, false},
        {"colptr_negative", 10, 9, {0, -2, 7, 9}, rows9, kCscColptr, 0, false},
        {"colptr_middle_beyond_nnz", 10, 9, {0, 3, 700, 9}, rows9, kCscColptr, 1, false},
        {"column_longer_than_G", 4, 5, {0, 5, 5, 5}, {0, 1, 2, 3, 3}, kCscColptr, 0, false},
        {"colptr_fault_behind_a_row_fault", 10, 9, {0, 3, 7, 14}, with(rows9, 1, 99), kCscColptr, 2, false},
        {"colptr_2_pow_40", 10, 9, {0, 3, int64_t(1) << 40, 9}, rows9, kCscColptr, 1, true},
    };
    for (const Case &k : cases) {
        if (!k.wide_only) run<int32_t>(k, 32);
        run<int64_t>(k, 64);
    }
    if (g_fail) { fprintf(stderr, "%ld failures\n", g_fail); return 1; }
    printf("ok %ld\n", g_cases);
    return 0;
}
