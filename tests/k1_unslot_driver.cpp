// The word forms of the column un-permute (csrc/k1_slots.h: unslot_*) without a GPU.  The serial host model of k1_unslot_words runs the
// kernel's own steps -- in-transpose, T, gather, out-transpose, the tails -- through the functions the kernel uses; its table must be
// what slot_unpermute_row makes of every bit row.  Built with AddressSanitizer and UBSan by tests/test_unslot_cpu.py: the table and T
// are allocated at exactly the sizes the rules report, so a stray index is an error and not a lucky hit.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <vector>

#include "k1_slots.h"

using namespace reo;

static int fails = 0;
#define CHECK(cond, ...)                                                    \
    do {                                                                    \
        if (!(cond)) { ++fails; std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    } while (0)

enum Perm { kRandom, kIdentity, kReversal };
static const char *perm_name[] = {"random", "identity", "reversal"};

// g2s over Gp slots: a permutation of 0 .. G-1 in front, padding slots map to themselves
static std::vector<uint32_t> make_g2s(int G, int Gp, Perm p, std::mt19937 &rng)
{
    std::vector<uint32_t> first(G), g2s(Gp), s2g(Gp);
    std::iota(first.begin(), first.end(), 0u);
    if (p == kRandom) std::shuffle(first.begin(), first.end(), rng);
    if (p == kReversal) std::reverse(first.begin(), first.end());
    slot_invert(first.data(), G, Gp, g2s.data(), s2g.data());
    for (int k = G; k < Gp; ++k) CHECK(g2s[k] == static_cast<uint32_t>(k) && s2g[k] == static_cast<uint32_t>(k), "padding slot %d", k);
    return g2s;
}

// one table of n_rows rows in slot order (random bits in EVERY column, the padded ones too: the kernel must zero them), through the
// model group by group, against slot_unpermute_row; the rows behind n_rows keep their canary
template <int R>
static void run_table(int G, int Gp, int n_rows, const std::vector<uint32_t> &g2s, std::mt19937 &rng, const char *what)
{
    const int Wp = Gp / 32, spare = R;
    const size_t row_words = static_cast<size_t>(4) * Wp;
    std::vector<uint32_t> table((n_rows + spare) * row_words), want(table.size()), T(unslot_lds_bytes(R, Gp) / sizeof(uint32_t));
    for (auto &v : table) v = rng();
    want = table;
    for (int rp = 0; rp < 4 * n_rows; ++rp) slot_unpermute_row(table.data() + static_cast<size_t>(rp) * Wp, want.data() + static_cast<size_t>(rp) * Wp, Wp, g2s.data(), G);
    const int groups = (n_rows + R - 1) / R;
    for (int b = 0; b < groups + 1; ++b) {   // (one group past the table: it does nothing)
        std::fill(T.begin(), T.end(), 0xDEADBEEFu);
        unslot_group_model<R>(table.data(), b * R, n_rows, G, Wp, g2s.data(), T.data());
    }
    size_t bad = 0;
    for (size_t i = 0; i < table.size(); ++i) bad += table[i] != want[i];
    CHECK(bad == 0, "%s R %d G %d Gp %d rows %d: %zu words differ", what, R, G, Gp, n_rows, bad);
    for (int rp = 0; rp < 4 * n_rows; ++rp)   // columns from G on are zero
        for (int j = G; j < Gp; ++j) CHECK(!((table[static_cast<size_t>(rp) * Wp + (j >> 5)] >> (j & 31)) & 1u), "%s R %d G %d: column %d of bit row %d", what, R, G, j, rp);
}

template <int R>
static void lds_rule(int Gp)
{
    const size_t entry = R == kUnslotWide ? 4 : 2, n = unslot_lds_bytes(R, Gp) / entry;
    CHECK(unslot_lds_bytes(R, Gp) % 4 == 0, "whole words");
    std::vector<unsigned char> seen(n, 0);
    for (int k = 0; k < Gp; ++k) {
        const size_t i = unslot_lds_index(R, static_cast<uint32_t>(k));
        CHECK(i < n, "R %d Gp %d: slot %d at entry %zu of %zu", R, Gp, k, i, n);
        if (i < n) { CHECK(!seen[i], "R %d Gp %d: slot %d shares entry %zu", R, Gp, k, i); seen[i] = 1; }
    }
    // a wave's in-phase stores (64 neighbouring slot words, one entry index b) fall on 32 different banks per half wave
    for (int b = 0; b < (R == kUnslotWide ? 32 : 16); ++b) {
        unsigned banks = 0;
        for (int w = 0; w < 32; ++w) banks |= 1u << ((unslot_lds_index(R, 32u * w + b) * entry / 4) & 31u);   // (Gp is a multiple of 1 024: 32 words at least)
        CHECK(banks == 0xFFFFFFFFu, "R %d: entry %d of neighbouring words shares a bank (%08x)", R, b, banks);
    }
}

int main()
{
    std::mt19937 rng(20261019u);
    // the bits of an entry: one per (row, plane), the planes of a row together
    for (int R : {kUnslotWide, kUnslotNarrow}) {
        std::vector<int> seen(4 * R, 0);
        for (int r = 0; r < R; ++r)
            for (int p = 0; p < 4; ++p) { const int q = unslot_bit(r, p); CHECK(q >= 0 && q < 4 * R && !seen[q], "bit of (%d, %d)", r, p); if (q >= 0 && q < 4 * R) seen[q] = 1; }
    }
    // the transposes are their own inverse and move bit (q, b) to (b, q)
    {
        uint32_t a[32], b[32];
        for (auto &v : a) v = rng();
        std::copy(a, a + 32, b);
        unslot_transpose<32>(b);
        for (int q = 0; q < 32; ++q)
            for (int i = 0; i < 32; ++i) CHECK(((b[i] >> q) & 1u) == ((a[q] >> i) & 1u), "32 x 32 bit (%d, %d)", q, i);
        unslot_transpose<32>(b);
        CHECK(std::equal(a, a + 32, b), "32 x 32 twice");
        uint32_t c[16], d[16];
        for (auto &v : c) v = rng();
        std::copy(c, c + 16, d);
        unslot_transpose<16>(d);
        for (int q = 0; q < 16; ++q)
            for (int i = 0; i < 32; ++i) CHECK(((d[i & 15] >> (q + 16 * (i >> 4))) & 1u) == ((c[q] >> i) & 1u), "16 x 32 bit (%d, %d)", q, i);
        unslot_transpose<16>(d);
        CHECK(std::equal(c, c + 16, d), "16 x 32 twice");
        std::printf("ok transposes\n");
    }
    const int Gs[] = {2, 31, 32, 33, 257, 1000, 1025, 9000};
    for (int p = kRandom; p <= kReversal; ++p) {
        for (int G : Gs) {
            const int Gp = (G + 1023) / 1024 * 1024;
            const std::vector<uint32_t> g2s = make_g2s(G, Gp, static_cast<Perm>(p), rng);
            // the last group holds 1 row, R - 1 rows, all R
            for (int extra : {1, kUnslotWide - 1, kUnslotWide}) run_table<kUnslotWide>(G, Gp, kUnslotWide + extra, g2s, rng, perm_name[p]);
            for (int extra : {1, kUnslotNarrow - 1, kUnslotNarrow}) run_table<kUnslotNarrow>(G, Gp, kUnslotNarrow + extra, g2s, rng, perm_name[p]);
            if (G <= 33) {   // the class table itself: G rows (2 of 8, 7 of 8, 8 of 8, 1 of 8 in the last group)
                run_table<kUnslotWide>(G, Gp, G, g2s, rng, perm_name[p]);
                run_table<kUnslotNarrow>(G, Gp, G, g2s, rng, perm_name[p]);
            }
        }
        std::printf("ok %s\n", perm_name[p]);
    }
    // the LDS index: one entry per slot, inside the bytes the rule reports
    for (int Gp : {1024, 2048, 9216, 20480, 38912}) lds_rule<kUnslotWide>(Gp);
    for (int Gp : {1024, 2048, 9216, 20480, 38912, 39936, 65536}) lds_rule<kUnslotNarrow>(Gp);
    std::printf("ok lds_index\n");
    // the form chosen: narrow up to 25 600 slots, wide up to 38 912 (its last), narrow from 39 936 (its first) to 65 536
    CHECK(unslot_form(1024) == kUnslotNarrow && unslot_form(20480) == kUnslotNarrow && unslot_form(25600) == kUnslotNarrow, "narrow while three workgroups fit");
    CHECK(3 * unslot_lds_bytes(kUnslotNarrow, 25600) <= kUnslotLdsLimit && 3 * unslot_lds_bytes(kUnslotNarrow, 26624) > kUnslotLdsLimit, "the limit of three");
    CHECK(unslot_form(26624) == kUnslotWide && unslot_form(30720) == kUnslotWide && unslot_form(38912) == kUnslotWide, "wide from 26 624 up to 38 912");
    CHECK(unslot_lds_bytes(kUnslotWide, 38912) <= kUnslotLdsLimit && unslot_lds_bytes(kUnslotWide, 39936) > kUnslotLdsLimit, "the wide form's limit");
    CHECK(unslot_form(39936) == kUnslotNarrow && unslot_form(65536) == kUnslotNarrow, "narrow from 39 936");
    CHECK(unslot_lds_bytes(kUnslotNarrow, 65536) <= kUnslotLdsLimit, "the narrow form fits every slot build");
    // threads: whole waves, within the bound, every word taken, no trip more than the bound needs
    for (int Wp = 32; Wp <= 2048; Wp += 32) {
        const int t = unslot_threads(Wp);
        CHECK(t % 64 == 0 && t >= 64 && t <= kUnslotThreadsMax, "threads %d at Wp %d", t, Wp);
        CHECK((Wp + t - 1) / t == (Wp + kUnslotThreadsMax - 1) / kUnslotThreadsMax, "trips at Wp %d", Wp);
    }
    std::printf("ok form wide_bytes_38912 %zu narrow_bytes_65536 %zu threads_640 %d threads_1056 %d\n", unslot_lds_bytes(kUnslotWide, 38912),
                unslot_lds_bytes(kUnslotNarrow, 65536), unslot_threads(640), unslot_threads(1056));
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    return 0;
}
