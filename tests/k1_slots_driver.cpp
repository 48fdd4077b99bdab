// Driver of tests/test_slot_order_cpu.py: the index rules of the pair kernel's slot order (csrc/k1_slots.h) on random data.  Plain host
// C++ with its own main, built with -fsanitize=address,undefined.  Prints one "ok <case>" line per case; any failed check ends it with 1.
//   g++ -std=c++17 -fsanitize=address,undefined -I rankcompv3.jl_amd/csrc -o driver tests/k1_slots_driver.cpp && ./driver
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "k1_slots.h"

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

// G genes on `levels` base levels with noise, two sides of n samples: positions = ranks inside a sample, as the transform makes them
static int run_case(const char *name, int G, int levels, int noise, int n, uint32_t seed)
{
    using namespace reo;
    std::mt19937 rng(seed);
    const int Gp = (G + 1023) / 1024 * 1024, W = Gp / 32;
    std::vector<uint32_t> gmm(2 * static_cast<size_t>(G), slot_pack(kSlotNoMin, kSlotNoMax));
    std::vector<int> base(G);
    for (int g = 0; g < G; ++g) base[g] = static_cast<int>(rng() % static_cast<uint32_t>(levels));
    std::vector<std::pair<uint64_t, int>> col(G);
    for (int side = 0; side < 2; ++side)
        for (int s = 0; s < n; ++s) {
            for (int g = 0; g < G; ++g) col[g] = {static_cast<uint64_t>(base[g] * 16 + static_cast<int>(rng() % static_cast<uint32_t>(16 * noise + 1))) << 20 | (rng() & 0xFFFFFu), g};
            std::sort(col.begin(), col.end());   // tie-free: the random low bits and the gene break every tie
            for (int r = 0; r < G; ++r) {
                uint32_t &w = gmm[static_cast<size_t>(side) * G + col[r].second];
                w = slot_join(w, slot_pack(static_cast<uint32_t>(r), static_cast<uint32_t>(r)));
            }
        }
    std::vector<uint32_t> key(G), rank(G), g2s(Gp), s2g(Gp, 0xFFFFFFFFu);
    for (int g = 0; g < G; ++g) {
        key[g] = slot_key(gmm[g], gmm[G + g]);
        CHECK(key[g] == slot_min(gmm[g]) + slot_max(gmm[g]) + slot_min(gmm[G + g]) + slot_max(gmm[G + g]));
    }
    slot_rank(key.data(), G, rank.data());
    slot_invert(rank.data(), G, Gp, g2s.data(), s2g.data());
    // the order is a permutation, sorted by (key, gene); g2s o s2g is the identity; padding slots map to themselves
    std::vector<char> seen(Gp, 0);
    for (int k = 0; k < Gp; ++k) {
        CHECK(s2g[k] < static_cast<uint32_t>(Gp) && !seen[s2g[k]]);
        seen[s2g[k]] = 1;
        CHECK(g2s[s2g[k]] == static_cast<uint32_t>(k));
        CHECK((k < G) == (s2g[k] < static_cast<uint32_t>(G)));
        if (k >= G) CHECK(s2g[k] == static_cast<uint32_t>(k));
        if (k > 0 && k < G) CHECK(slot_order_key(key[s2g[k - 1]], s2g[k - 1]) < slot_order_key(key[s2g[k]], s2g[k]));
    }
    // tile and chunk ranges over the slots below G; the predicate against the genes' own ranges, and never for a tile inside its chunk
    const int NT = Gp / kSlotTile, NQ = Gp / kSlotChunk;
    size_t separated = 0, live = 0;
    for (int side = 0; side < 2; ++side) {
        std::vector<uint32_t> trng(NT, slot_pack(kSlotNoMin, kSlotNoMax)), crng(NQ, slot_pack(kSlotNoMin, kSlotNoMax));
        for (int k = 0; k < G; ++k) {
            const uint32_t w = gmm[static_cast<size_t>(side) * G + s2g[k]];
            trng[k / kSlotTile] = slot_join(trng[k / kSlotTile], w);
            crng[k / kSlotChunk] = slot_join(crng[k / kSlotChunk], w);
        }
        for (int t = 0; t * kSlotTile < G; ++t)
            for (int q = 0; q * kSlotChunk < G; ++q) {
                const int sep = slot_separated(trng[t], crng[q]);
                if (t / (kSlotChunk / kSlotTile) == q) CHECK(sep == 0);
                if (kSlotChunk * q + kSlotChunk - 1 >= (kSlotTile * t / 64) * 64) { ++live; separated += sep != 0; }
                if (!sep) continue;
                for (int i = t * kSlotTile; i < std::min(G, (t + 1) * kSlotTile); ++i)
                    for (int j = q * kSlotChunk; j < std::min(G, (q + 1) * kSlotChunk); ++j) {
                        const uint32_t wi = gmm[static_cast<size_t>(side) * G + s2g[i]], wj = gmm[static_cast<size_t>(side) * G + s2g[j]];
                        if (sep > 0) CHECK(slot_max(wj) < slot_min(wi));   // column gene below row gene in every sample: every sample counts
                        else CHECK(slot_max(wi) < slot_min(wj));           // ... above: none does
                    }
            }
    }
    // a row of the table: un-permute, then permute, is the identity on the bits of the slots below G; columns from G on come out zero
    for (int rep = 0; rep < 8; ++rep) {
        std::vector<uint32_t> row(W), gene_row(W), back(W);
        for (int w = 0; w < W; ++w) row[w] = static_cast<uint32_t>(rng());
        for (int k = G; k < Gp; ++k) row[k >> 5] &= ~(1u << (k & 31));   // (the pair kernel writes no bit of a padding slot)
        slot_unpermute_row(row.data(), gene_row.data(), W, g2s.data(), G);
        for (int j = 0; j < Gp; ++j) {
            const uint32_t bit = (gene_row[j >> 5] >> (j & 31)) & 1u;
            if (j < G) CHECK(bit == ((row[g2s[j] >> 5] >> (g2s[j] & 31)) & 1u));
            else CHECK(bit == 0);
        }
        slot_permute_row(gene_row.data(), back.data(), W, s2g.data(), G);
        CHECK(back == row);
    }
    // the item fields
    CHECK(slot_item_tile(1u << 31 | 77u << 16 | 0x8000u | 0x4000u | 613u) == 613 && slot_item_chunk(1u << 31 | 77u << 16 | 0xC000u | 613u) == 77);
    CHECK(slot_item_side(1u << 31 | 5u) == 1 && slot_item_halves(0x8000u | 5u) == 1 && slot_item_halves(5u) == 2);
    printf("ok %s G %d live %zu separated %zu\n", name, G, live, separated);
    return 0;
}

int main()
{
    int bad = 0;
    bad |= run_case("levels64", 3000, 64, 4, 6, 1);        // the T0 family's shape: most items separated
    bad |= run_case("odd_G", 2049, 64, 4, 5, 2);           // a one-gene last tile, G no multiple of 32
    bad |= run_case("tiny", 37, 4, 1, 3, 3);               // one tile, one chunk: nothing can be separated
    bad |= run_case("one_level", 1500, 1, 40, 4, 4);       // no levels: (almost) nothing separated
    bad |= run_case("equal_keys", 1100, 2, 0, 1, 5);       // one sample per side: many equal keys, the gene breaks them
    return bad;
}
