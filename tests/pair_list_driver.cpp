// Host-only driver for csrc/pair_list.h (tests/test_pair_list_cpu.py builds it with -fsanitize=address,undefined and runs it): the
// selected-pair word that both kernels of csrc/pairlist.hip form, checked bit by bit against a naive decode of the four planes.
//   - all 511 class masks on seeded random plane words that respect "not L and H at once" (a pair is in one class per side);
//   - G = 33, 64, 65 and 127, so that the last word has a tail (or, at 64, exactly none) and words past the last gene exist;
//   - query rows whose diagonal bit is the first, a middle and the last bit of a word, and the last gene;
//   - a partner mask ANDed into `valid`, as the kernels do;
//   - pair_code_at against the same decode, pair_list_rowptr, and every argument check of pair_list_check_args with its number.
// Prints "case <G> <checked bits>" per G and "ok <checks>"; anything on stderr is a failure.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pair_list.h"

namespace {

long g_checks = 0, g_fail = 0;

uint64_t g_state = 0x9E3779B97F4A7C15ULL;
uint32_t rnd()   // splitmix64, seeded: the same words on every run
{
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return static_cast<uint32_t>((z ^ (z >> 31)) >> 16);
}

void fail(const char *what, int G, int row, int w, uint32_t mask)
{
    fprintf(stderr, "FAIL %s: G %d row %d word %d class_mask 0x%X\n", what, G, row, w, mask);
    ++g_fail;
}

// the class of bit b, decoded the way k_decode does it: L wins, then H, else the middle
int naive_code(uint32_t cl, uint32_t ch, uint32_t tl, uint32_t th, int b)
{
    const int l = (cl >> b) & 1, h = (ch >> b) & 1, t0 = (tl >> b) & 1, t1 = (th >> b) & 1;
    const int ic = l ? 0 : (h ? 2 : 1), it = t0 ? 0 : (t1 ? 2 : 1);
    return 3 * ic + it;
}

void run_G(int G)
{
    const int W = 8;   // words per row here: columns 0 .. 255, more than any G of this driver
    long bits = 0;
    std::vector<int> rows = {0, 15, 31, 32, G / 2, G - 2, G - 1};
    for (int row : rows) {
        if (row < 0 || row >= G) continue;
        // exactly W words per plane, so that a read past the row is the sanitizer's to report
        std::vector<uint32_t> cl(W), ch(W), tl(W), th(W), pm(W);
        for (int w = 0; w < W; ++w) {
            const uint32_t a = rnd(), b = rnd(), c = rnd(), d = rnd();
            cl[w] = a & ~b; ch[w] = b & ~a;   // never both
            tl[w] = c & ~d; th[w] = d & ~c;
            pm[w] = rnd() | rnd();
        }
        for (uint32_t mask = 1; mask <= reo::kPairClassAll; ++mask)
            for (int w = 0; w < W; ++w) {
                const uint32_t valid = reo::pair_valid_word(row, w, G);
                const uint32_t got = reo::pair_select_word(cl[w], ch[w], tl[w], th[w], valid & pm[w], mask);
                uint32_t want = 0;
                for (int b = 0; b < 32; ++b) {
                    const int j = 32 * w + b;
                    if (j >= G || j == row || !((pm[w] >> b) & 1)) continue;
                    const int code = naive_code(cl[w], ch[w], tl[w], th[w], b);
                    if ((mask >> code) & 1) want |= 1u << b;
                    if (mask == 1) {
                        ++g_checks;
                        if (static_cast<int>(reo::pair_code_at(cl[w], ch[w], tl[w], th[w], b)) != code) fail("pair_code_at", G, row, w, mask);
                    }
                }
                ++g_checks; bits += 32;
                if (got != want) fail("pair_select_word", G, row, w, mask);
            }
        // the valid word itself: columns < G without the diagonal
        for (int w = 0; w < W; ++w) {
            uint32_t want = 0;
            for (int b = 0; b < 32; ++b)
                if (32 * w + b < G && 32 * w + b != row) want |= 1u << b;
            ++g_checks;
            if (reo::pair_valid_word(row, w, G) != want) fail("pair_valid_word", G, row, w, 0);
        }
    }
    printf("case %d %ld\n", G, bits);
}

void expect_check(int want, int64_t G, const int32_t *genes, int64_t n, uint32_t mask, const int64_t *rowptr, const int32_t *partner,
                  const uint8_t *code, int64_t cap, const char *needle)
{
    char msg[320] = "";
    const int got = reo::pair_list_check_args(G, genes, n, mask, rowptr, partner, code, cap, msg, sizeof msg);
    ++g_checks;
    if (got != want || (want != 0 && !strstr(msg, needle))) {
        fprintf(stderr, "FAIL pair_list_check_args: check %d expected %d (\"%s\"), message \"%s\"\n", got, want, needle, msg);
        ++g_fail;
    }
}

void run_checks()
{
    int32_t *genes = new int32_t[3]{4, 0, 4};   // exactly n_genes entries; repeats and any order are fine
    int64_t *rowptr = new int64_t[4];
    int32_t *partner = new int32_t[2];
    uint8_t *code = new uint8_t[2];
    expect_check(0, 5, genes, 3, 0x44, rowptr, partner, code, 2, "");
    expect_check(0, 5, genes, 3, 0x1FF, rowptr, nullptr, nullptr, 0, "");
    expect_check(0, 5, genes, 3, 0x1, rowptr, partner, code, 0, "");
    expect_check(1, 5, nullptr, 3, 0x44, rowptr, partner, code, 2, "must not be null");
    expect_check(1, 5, genes, 3, 0x44, nullptr, partner, code, 2, "must not be null");
    expect_check(2, 5, genes, 0, 0x44, rowptr, partner, code, 2, "at least one query gene");
    expect_check(2, 5, genes, -1, 0x44, rowptr, partner, code, 2, "n_genes = -1");
    expect_check(3, 5, genes, 3, 0, rowptr, partner, code, 2, "no class");
    expect_check(3, 5, genes, 3, 0x200, rowptr, partner, code, 2, "bits above 8");
    expect_check(3, 5, genes, 3, 0x80000001u, rowptr, partner, code, 2, "bits above 8");
    expect_check(4, 5, genes, 3, 0x44, rowptr, partner, nullptr, 2, "both");
    expect_check(4, 5, genes, 3, 0x44, rowptr, nullptr, code, 0, "both");
    expect_check(5, 5, genes, 3, 0x44, rowptr, partner, code, -1, "capacity -1");
    expect_check(5, 5, genes, 3, 0x44, rowptr, nullptr, nullptr, 7, "capacity 7");
    expect_check(6, 4, genes, 3, 0x44, rowptr, partner, code, 2, "genes[0] = 4 is outside [0, 4)");
    genes[1] = -1;
    expect_check(6, 5, genes, 3, 0x44, rowptr, partner, code, 2, "genes[1] = -1");
    // the two checks that the other query entry points share with this one, called directly (genes is {4, -1, 4} here)
    char msg[320] = "";
    const auto expect_shared = [&](bool got, bool want, const char *needle) {
        ++g_checks;
        if (got != want || (!want && !strstr(msg, needle))) {
            fprintf(stderr, "FAIL shared query check: %d expected %d (\"%s\"), message \"%s\"\n", got, want, needle, msg);
            ++g_fail;
        }
    };
    expect_shared(reo::query_genes_in_range("reo_x", 5, nullptr, 3, msg, sizeof msg), true, "");   // (null genes: the caller's own refusal)
    expect_shared(reo::query_genes_in_range("reo_x", 5, genes, 0, msg, sizeof msg), true, "");
    expect_shared(reo::query_genes_in_range("reo_x", 5, genes, 1, msg, sizeof msg), true, "");
    expect_shared(reo::query_genes_in_range("reo_x", 4, genes, 1, msg, sizeof msg), false, "reo_x: genes[0] = 4 is outside [0, 4)");
    expect_shared(reo::query_genes_in_range("reo_x", 5, genes, 3, msg, sizeof msg), false, "reo_x: genes[1] = -1 is outside [0, 5)");
    expect_shared(reo::query_class_mask_ok("reo_x", 0x1FF, msg, sizeof msg), true, "");
    expect_shared(reo::query_class_mask_ok("reo_x", 0, msg, sizeof msg), false, "reo_x: class_mask 0x0 selects no class");
    expect_shared(reo::query_class_mask_ok("reo_x", 0x200, msg, sizeof msg), false, "reo_x: class_mask 0x200 selects bits above 8");
    const int32_t count[3] = {2, 0, 5};
    ++g_checks;
    if (reo::pair_list_rowptr(count, 3, rowptr) != 7 || rowptr[0] != 0 || rowptr[1] != 2 || rowptr[2] != 2 || rowptr[3] != 7) {
        fprintf(stderr, "FAIL pair_list_rowptr\n");
        ++g_fail;
    }
    delete[] genes; delete[] rowptr; delete[] partner; delete[] code;
}

}  // namespace

int main()
{
    for (int G : {33, 64, 65, 127}) run_G(G);
    run_checks();
    if (g_fail) { fprintf(stderr, "%ld failures\n", g_fail); return 1; }
    printf("ok %ld\n", g_checks);
    return 0;
}
