// The PER-SIDE slot order (csrc/k1_slots.h: slot_side_key, slot_rank32, slot_maps_sides, slot_ranges_side, unslot_pair_model) without a
// GPU.  Part one: on levelled data whose two sides carry different orders of the genes, the per-side host rank, invert and ranges
// against brute force -- a sort of (key, gene) pairs, the maps' inverses, every slot's range joined by hand -- and the 32-bit order
// key against the 64-bit one.  Part two: the pair form of the word un-permute, a side's plane pair of 2R rows per group with that
// side's map, must leave what slot_unpermute_row makes of every bit row of the pair, with two DIFFERENT maps for the two sides, and
// must not touch the rows behind the table.  Built with AddressSanitizer and UBSan by tests/test_slot_sides_cpu.py: every buffer is
// allocated at exactly the size the rules report.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <utility>
#include <vector>

#include "k1_slots.h"

using namespace reo;

static int fails = 0;
#define CHECK(cond, ...)                                                    \
    do {                                                                    \
        if (!(cond)) { ++fails; std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    } while (0)

constexpr int kRankGenes = 2049;   // the counting ranks (G^2 comparisons) run up to here
static_assert(kRankGenes <= kSlotKey32Genes, "both host ranks apply");

static int padded(int G) { return (G + 1023) / 1024 * 1024; }

// gmm[z][g]: ranges of G genes on L levels per side, the sides' levels two independent permutations of the genes' classes; `flat0`: every
// gene of side 0 has the same key (ranges [g, K - g]: the gene index decides)
static std::vector<uint32_t> make_ranges(int G, int Gp, int L, bool flat0, std::mt19937 &rng)
{
    std::vector<uint32_t> gmm(2 * static_cast<size_t>(Gp), slot_pack(kSlotNoMin, kSlotNoMax));
    std::vector<int> lev[2];
    for (auto &v : lev) { v.resize(L); std::iota(v.begin(), v.end(), 0); std::shuffle(v.begin(), v.end(), rng); }
    const uint32_t width = static_cast<uint32_t>(std::max(1, G / L));   // positions of a level: [level * width, level * width + width)
    for (int g = 0; g < G; ++g) {
        const int cls = static_cast<int>(rng() % static_cast<unsigned>(L));
        for (int z = 0; z < 2; ++z) {
            uint32_t a = static_cast<uint32_t>(lev[z][cls]) * width + rng() % width, b = static_cast<uint32_t>(lev[z][cls]) * width + rng() % width;
            if (a > b) std::swap(a, b);
            if (z == 0 && flat0) { a = static_cast<uint32_t>(g) / 2; b = static_cast<uint32_t>(G) - a; }
            gmm[static_cast<size_t>(z) * Gp + g] = slot_pack(a, b);
        }
    }
    return gmm;
}

// part one for one size; returns the number of (tile, later chunk) pairs that are separated on either side
static long maps_case(int G, int L, bool flat0, std::mt19937 &rng, const char *what)
{
    const int Gp = padded(G);
    const std::vector<uint32_t> gmm = make_ranges(G, Gp, L, flat0, rng);
    std::vector<uint32_t> key(2 * static_cast<size_t>(Gp)), g2s(key.size()), s2g(key.size()), rank_G(G);
    if (G <= kRankGenes) slot_maps_sides(gmm.data(), G, Gp, key.data(), g2s.data(), s2g.data(), rank_G.data());
    else   // (above: no G^2 rank here -- the 64-bit slot_rank is the common order's, pinned by k1_slots_driver.cpp; the maps come from a sort)
        for (int z = 0; z < 2; ++z) {
            const size_t o = static_cast<size_t>(z) * Gp;
            std::vector<uint32_t> by(G);
            std::iota(by.begin(), by.end(), 0u);
            for (int g = 0; g < G; ++g) key[o + g] = slot_side_key(gmm[o + g]);
            std::stable_sort(by.begin(), by.end(), [&](uint32_t a, uint32_t b) { return key[o + a] < key[o + b]; });
            for (int k = 0; k < G; ++k) rank_G[by[k]] = static_cast<uint32_t>(k);
            slot_invert(rank_G.data(), G, Gp, g2s.data() + o, s2g.data() + o);
        }
    long separated = 0;
    for (int z = 0; z < 2; ++z) {
        const size_t o = static_cast<size_t>(z) * Gp;
        // brute force: the genes sorted by (key of the side alone, gene)
        std::vector<std::pair<uint32_t, uint32_t>> order(G);
        for (int g = 0; g < G; ++g) order[g] = {slot_min(gmm[o + g]) + slot_max(gmm[o + g]), static_cast<uint32_t>(g)};
        std::sort(order.begin(), order.end());
        size_t bad = 0;
        for (int k = 0; k < G; ++k) bad += s2g[o + k] != order[k].second || g2s[o + order[k].second] != static_cast<uint32_t>(k);
        CHECK(bad == 0, "%s G %d side %d: %zu slots differ from the sorted order", what, G, z, bad);
        for (int k = G; k < Gp; ++k) CHECK(g2s[o + k] == static_cast<uint32_t>(k) && s2g[o + k] == static_cast<uint32_t>(k), "%s G %d side %d: padding slot %d", what, G, z, k);
        if (G <= kRankGenes) {   // the 32-bit key orders as the 64-bit one: the same rank from both host forms
            std::vector<uint32_t> r64(G);
            {
                slot_rank(key.data() + o, G, r64.data());
                bad = 0;
                for (int g = 0; g < G; ++g) bad += r64[g] != g2s[o + g];
                CHECK(bad == 0, "%s G %d side %d: %zu ranks differ between the 32- and 64-bit keys", what, G, z, bad);
            }
            for (int g = 0; g < G; ++g) CHECK(key[o + g] < (1u << 17), "%s G %d: key %u of gene %d", what, G, key[o + g], g);
        }
        // ranges: every tile and chunk joined by hand from the genes in its slots
        std::vector<uint32_t> trng(Gp / kSlotTile), crng(Gp / kSlotChunk);
        slot_ranges_side(gmm.data() + o, s2g.data() + o, G, Gp, trng.data(), crng.data());
        for (int t = 0; t < Gp / kSlotTile; ++t) {
            uint32_t mn = kSlotNoMin, mx = kSlotNoMax;
            for (int k = t * kSlotTile; k < std::min(G, (t + 1) * kSlotTile); ++k) { mn = std::min(mn, slot_min(gmm[o + order[k].second])); mx = std::max(mx, slot_max(gmm[o + order[k].second])); }
            CHECK(trng[t] == slot_pack(mn, mx), "%s G %d side %d: tile %d", what, G, z, t);
        }
        for (int q = 0; q < Gp / kSlotChunk; ++q) {
            uint32_t mn = kSlotNoMin, mx = kSlotNoMax;
            for (int k = q * kSlotChunk; k < std::min(G, (q + 1) * kSlotChunk); ++k) { mn = std::min(mn, slot_min(gmm[o + order[k].second])); mx = std::max(mx, slot_max(gmm[o + order[k].second])); }
            CHECK(crng[q] == slot_pack(mn, mx), "%s G %d side %d: chunk %d", what, G, z, q);
        }
        // a side in its own order: a later chunk never lies below a tile (the count n_side cannot occur), a tile's own chunk never separates
        const int NT = (G + kSlotTile - 1) / kSlotTile, NQ = (G + kSlotChunk - 1) / kSlotChunk;
        for (int t = 0; t < NT; ++t)
            for (int q = t * kSlotTile / kSlotChunk; q < NQ; ++q) {
                const int s = slot_separated(trng[t], crng[q]);
                CHECK(s <= 0, "%s G %d side %d: chunk %d below tile %d", what, G, z, q, t);
                if (q == t * kSlotTile / kSlotChunk) CHECK(s == 0, "%s G %d side %d: tile %d apart from its own chunk", what, G, z, t);
                separated += s != 0;
            }
    }
    return separated;
}

// part two: a table of n_rows rows whose plane pairs are in the sides' slot orders, through the pair model group by group and side by side
template <int R>
static void pair_table(int G, int Gp, int n_rows, const std::vector<uint32_t> (&g2s)[2], std::mt19937 &rng)
{
    const int Wp = Gp / 32, spare = 2 * R;
    const size_t row_words = static_cast<size_t>(4) * Wp;
    std::vector<uint32_t> table((n_rows + spare) * row_words), want, T(unslot_lds_bytes(R, Gp) / sizeof(uint32_t));
    for (auto &v : table) v = rng();
    want = table;
    for (int rp = 0; rp < 4 * n_rows; ++rp)   // bit row rp: row rp / 4, plane rp % 4 -- the map of side (rp % 4) / 2
        slot_unpermute_row(table.data() + static_cast<size_t>(rp) * Wp, want.data() + static_cast<size_t>(rp) * Wp, Wp, g2s[(rp & 3) >> 1].data(), G);
    const int groups = (n_rows + 2 * R - 1) / (2 * R);
    for (int side = 1; side >= 0; --side)
        for (int b = 0; b < groups + 1; ++b) {   // (one group past the table: it does nothing)
            std::fill(T.begin(), T.end(), 0xDEADBEEFu);
            unslot_pair_model<R>(table.data(), b * 2 * R, n_rows, side, G, Wp, g2s[side].data(), T.data());
        }
    size_t bad = 0;
    for (size_t i = 0; i < table.size(); ++i) bad += table[i] != want[i];
    CHECK(bad == 0, "pair form R %d G %d Gp %d rows %d: %zu words differ", R, G, Gp, n_rows, bad);
}

int main()
{
    std::mt19937 rng(20261019u);
    // the bits of a pair entry: one per (row of 2R, plane of the pair), and the word each stands for
    for (int R : {kUnslotWide, kUnslotNarrow}) {
        std::vector<int> seen(4 * R, 0);
        for (int r = 0; r < 2 * R; ++r)
            for (int p = 0; p < 2; ++p) {
                const int q = unslot_pair_bit(r, p);
                CHECK(q >= 0 && q < 4 * R && !seen[q], "bit of (%d, %d)", r, p);
                if (q >= 0 && q < 4 * R) seen[q] = 1;
                for (int side = 0; side < 2; ++side) CHECK(unslot_pair_word(q, side, 7, 3) == static_cast<size_t>((r * 4 + 2 * side + p) * 7 + 3), "word of (%d, %d, side %d)", r, p, side);
            }
    }
    std::printf("ok bits\n");
    // which builds: the rule and the switch
    CHECK(slot_sides_wanted(7, 8, 0) == 1 && slot_sides_wanted(8, 8, 0) == 2 && slot_sides_wanted(15, 1, 0) == 2 && slot_sides_wanted(16, 16, 0) == 2, "the rule");
    CHECK(slot_sides_wanted(16, 16, 1) == 1 && slot_sides_wanted(1, 1, 2) == 2, "the switch");
    CHECK(slot_order_key32_fits(32768) && !slot_order_key32_fits(32769), "the 32-bit key's limit");
    CHECK(slot_order_key32(4u * 32767u, 32767u) > slot_order_key32(4u * 32767u, 32766u) && slot_order_key32(4u * 32767u, 32767u) != 0xFFFFFFFFu, "the largest 32-bit key");
    std::printf("ok rule\n");
    const int Gs[] = {2, 33, 257, 1000, 2049, 65535};
    long separated = 0;
    for (int G : Gs) {
        separated += maps_case(G, G < 64 ? 2 : 8, false, rng, "levels");
        if (G <= 2049) maps_case(G, 8, true, rng, "flat side 0");
    }
    CHECK(separated > 0, "no separated item at all");
    std::printf("ok maps separated %ld\n", separated);
    for (int G : Gs) {
        const int Gp = padded(G);
        std::vector<uint32_t> g2s[2];
        for (auto &m : g2s) {   // two different random maps, padding slots to themselves
            std::vector<uint32_t> first(G), s2g(Gp);
            std::iota(first.begin(), first.end(), 0u);
            std::shuffle(first.begin(), first.end(), rng);
            m.resize(Gp);
            slot_invert(first.data(), G, Gp, m.data(), s2g.data());
        }
        CHECK(G < 3 || g2s[0] != g2s[1], "two maps");
        // the last group holds 1 row, 2R - 1 rows, all 2R; up to 33 genes the class table itself (G rows)
        // (the host model of the wide form runs at every size; the kernel takes it only where its T fits a workgroup's LDS)
        for (int extra : {1, 2 * kUnslotWide - 1, 2 * kUnslotWide}) pair_table<kUnslotWide>(G, Gp, 2 * kUnslotWide + extra, g2s, rng);
        for (int extra : {1, 2 * kUnslotNarrow - 1, 2 * kUnslotNarrow}) pair_table<kUnslotNarrow>(G, Gp, 2 * kUnslotNarrow + extra, g2s, rng);
        if (G <= 33) { pair_table<kUnslotWide>(G, Gp, G, g2s, rng); pair_table<kUnslotNarrow>(G, Gp, G, g2s, rng); }
    }
    std::printf("ok pair_form\n");
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    return 0;
}
