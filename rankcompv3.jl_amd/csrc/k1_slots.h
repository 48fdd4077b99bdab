// The index rules of the pair kernel's SLOT ORDER (kernels.hip, launch_k1 -> k1_slots): tie-free data of two groups is counted with
// the genes ordered by level, so that most (i-tile, wave chunk, side) items hold pairs whose order is the same in every sample -- their
// count is 0 or the side's size and the count loop is skipped.  Plain C++ without a context: the device kernels and a CPU test
// (tests/k1_slots_driver.cpp) use the same functions.
//   key(g)  = pmin_0 + pmax_0 + pmin_1 + pmax_1          the per-side extremes of gene g's positions over the side's real samples
//   slot(g) = #{ g' : (key(g'), g') < (key(g), g) }     a counting rank: a permutation of 0 .. G-1
//   s2g[slot(g)] = g, g2s[g] = slot(g); slots G .. Gp-1 (padding genes) map to themselves
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define REO_SLOTS_HD __host__ __device__ inline
#else
#define REO_SLOTS_HD inline
#endif

namespace reo {

constexpr int kSlotTile = 32;     // = kTileI: rows of an item's i-tile
constexpr int kSlotChunk = 256;   // = 64 kRJ: genes of an item's wave chunk
constexpr uint32_t kSlotNoMin = 0xFFFFu, kSlotNoMax = 0u;   // the range of no gene at all (min, max): separates nothing from anything real

// the extremes of one side travel as one word: min | max << 16 (positions of at most 65 535 genes)
REO_SLOTS_HD uint32_t slot_pack(uint32_t mn, uint32_t mx) { return mn | mx << 16; }
REO_SLOTS_HD uint32_t slot_min(uint32_t w) { return w & 0xFFFFu; }
REO_SLOTS_HD uint32_t slot_max(uint32_t w) { return w >> 16; }
REO_SLOTS_HD uint32_t slot_join(uint32_t a, uint32_t b)   // the range that holds both
{
    const uint32_t mn = slot_min(a) < slot_min(b) ? slot_min(a) : slot_min(b), mx = slot_max(a) > slot_max(b) ? slot_max(a) : slot_max(b);
    return slot_pack(mn, mx);
}

REO_SLOTS_HD uint32_t slot_key(uint32_t side0, uint32_t side1) { return slot_min(side0) + slot_max(side0) + slot_min(side1) + slot_max(side1); }

// key and gene as one number: its order is the order of (key, gene)
REO_SLOTS_HD uint64_t slot_order_key(uint32_t key, uint32_t gene) { return static_cast<uint64_t>(key) << 32 | gene; }

// What an item's counts are without counting, from the ranges of its i-tile (rmin, rmax) and its wave chunk (cmin, cmax) on its side:
// 1 every real sample counts (each column gene lies below each row gene in every sample), -1 none does, 0 the loop has to run.
// The ranges of a tile inside its chunk nest (cmin <= rmin <= rmax <= cmax), so a diagonal item never qualifies.
REO_SLOTS_HD int slot_separated(uint32_t tile_rng, uint32_t chunk_rng)
{
    if (slot_max(chunk_rng) < slot_min(tile_rng)) return 1;
    if (slot_max(tile_rng) < slot_min(chunk_rng)) return -1;
    return 0;
}

// an item of the list (k1_items.h): its i-tile and wave chunk; 2 for a full item, 1 for a half-height one
REO_SLOTS_HD int slot_item_tile(uint32_t item) { return static_cast<int>(item & 0x3FFFu); }
REO_SLOTS_HD int slot_item_chunk(uint32_t item) { return static_cast<int>((item >> 16) & 0x7FFFu); }
REO_SLOTS_HD int slot_item_side(uint32_t item) { return static_cast<int>(item >> 31); }
REO_SLOTS_HD int slot_item_halves(uint32_t item) { return (item & 0x8000u) ? 1 : 2; }

// ---- host versions (the CPU test; the device kernels do the same in parallel)

// g2s from the keys: the counting rank over G^2 comparisons
inline void slot_rank(const uint32_t *key, int G, uint32_t *g2s)
{
    for (int g = 0; g < G; ++g) {
        uint32_t n = 0;
        for (int h = 0; h < G; ++h) n += slot_order_key(key[h], static_cast<uint32_t>(h)) < slot_order_key(key[g], static_cast<uint32_t>(g)) ? 1u : 0u;
        g2s[g] = n;
    }
}

// s2g from g2s, both Gp long: padding slots map to themselves
inline void slot_invert(const uint32_t *g2s_G, int G, int Gp, uint32_t *g2s, uint32_t *s2g)
{
    for (int g = 0; g < G; ++g) { g2s[g] = g2s_G[g]; s2g[g2s_G[g]] = static_cast<uint32_t>(g); }
    for (int g = G; g < Gp; ++g) g2s[g] = s2g[g] = static_cast<uint32_t>(g);
}

// One bit row of the class table (W words) from slot-order columns into gene-order columns: out bit j = in bit g2s[j] for j < G, columns
// from G on are zero.  (k1_unslot_columns does this for every row and plane.)
inline void slot_unpermute_row(const uint32_t *in, uint32_t *out, int W, const uint32_t *g2s, int G)
{
    for (int w = 0; w < W; ++w) out[w] = 0;
    for (int j = 0; j < G; ++j) {
        const uint32_t k = g2s[j];
        out[j >> 5] |= ((in[k >> 5] >> (k & 31)) & 1u) << (j & 31);
    }
}

// ... and back: out bit k = in bit s2g[k] for slots k < G (what the pair kernel's slot-order row was)
inline void slot_permute_row(const uint32_t *in, uint32_t *out, int W, const uint32_t *s2g, int G)
{
    for (int w = 0; w < W; ++w) out[w] = 0;
    for (int k = 0; k < G; ++k) {
        const uint32_t j = s2g[k];
        out[k >> 5] |= ((in[j >> 5] >> (j & 31)) & 1u) << (k & 31);
    }
}

}  // namespace reo
