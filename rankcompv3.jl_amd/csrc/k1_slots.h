// The index rules of the pair kernel's SLOT ORDER (kernels.hip, launch_k1 -> k1_slots): tie-free data of two groups is counted with
// the genes ordered by level, so that most (i-tile, wave chunk, side) items hold pairs whose order is the same in every sample -- their
// count is 0 or the side's size and the count loop is skipped.  Plain C++ without a context: the device kernels and a CPU test
// (tests/k1_slots_driver.cpp) use the same functions.
//   key(g)  = pmin_0 + pmax_0 + pmin_1 + pmax_1          the per-side extremes of gene g's positions over the side's real samples
//   slot(g) = #{ g' : (key(g'), g') < (key(g), g) }     a counting rank: a permutation of 0 .. G-1
//   s2g[slot(g)] = g, g2s[g] = slot(g); slots G .. Gp-1 (padding genes) map to themselves
// PER-SIDE ORDER: an item belongs to one side and a side's words stay inside its two planes of the table, so each side may have an order
// of its own, key_z(g) = pmin_z + pmax_z, with its own g2s / s2g: a gene whose level differs between the groups is then in its place on
// both sides instead of between its two levels on either (slot_side_key, slot_sides_wanted and the *_sides / *_pair functions below).
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

// the key of one side alone (per-side order)
REO_SLOTS_HD uint32_t slot_side_key(uint32_t side) { return slot_min(side) + slot_max(side); }

// ... in 32 bits where they fit: up to 32 768 genes a position is below 2^15, every key (of one side or of both) below 2^17 and a gene
// below 2^15.  The rank (kernels.hip: sorted spans in LDS and binary searches; here: the counting rank) then moves half the bytes.
constexpr int kSlotKey32Genes = 32768;
REO_SLOTS_HD bool slot_order_key32_fits(int G) { return G <= kSlotKey32Genes; }
REO_SLOTS_HD uint32_t slot_order_key32(uint32_t key, uint32_t gene) { return key << 15 | gene; }

// Which builds order their sides separately: those whose two sides together have at least kSlotSidesBlocks sample blocks of 32.  The
// saving is a share of the count loops, whose length is the number of blocks; the second rank, invert and map cost the same at every
// sample count.  force: 0 this rule, 1 the common order everywhere, 2 per-side order everywhere (REO_K1_SLOT_SIDES).
constexpr int kSlotSidesBlocks = 16;
REO_SLOTS_HD int slot_sides_wanted(int blocks0, int blocks1, int force)
{
    if (force == 1 || force == 2) return force;
    return blocks0 + blocks1 >= kSlotSidesBlocks ? 2 : 1;
}

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

// the 32-bit form of slot_rank (G <= kSlotKey32Genes): the same permutation
inline void slot_rank32(const uint32_t *key, int G, uint32_t *g2s)
{
    for (int g = 0; g < G; ++g) {
        uint32_t n = 0;
        for (int h = 0; h < G; ++h) n += slot_order_key32(key[h], static_cast<uint32_t>(h)) < slot_order_key32(key[g], static_cast<uint32_t>(g)) ? 1u : 0u;
        g2s[g] = n;
    }
}

// Per-side order on the host: gmm[z][g] (Gp apart) -> key[z][g], g2s[z][.], s2g[z][.] (Gp apart each; the device does the same with
// the side as a grid dimension)
inline void slot_maps_sides(const uint32_t *gmm, int G, int Gp, uint32_t *key, uint32_t *g2s, uint32_t *s2g, uint32_t *rank_G)
{
    for (int z = 0; z < 2; ++z) {
        const size_t o = static_cast<size_t>(z) * Gp;
        for (int g = 0; g < G; ++g) key[o + g] = slot_side_key(gmm[o + g]);
        if (slot_order_key32_fits(G)) slot_rank32(key + o, G, rank_G);
        else slot_rank(key + o, G, rank_G);
        slot_invert(rank_G, G, Gp, g2s + o, s2g + o);
    }
}

// the ranges of side z's 32-slot tiles and 256-slot chunks over their slots below G (k1_slot_ranges): trng[Gp / 32], crng[Gp / 256]
inline void slot_ranges_side(const uint32_t *gmm_z, const uint32_t *s2g_z, int G, int Gp, uint32_t *trng, uint32_t *crng)
{
    for (int t = 0; t < Gp / kSlotTile; ++t) trng[t] = slot_pack(kSlotNoMin, kSlotNoMax);
    for (int q = 0; q < Gp / kSlotChunk; ++q) crng[q] = slot_pack(kSlotNoMin, kSlotNoMax);
    for (int k = 0; k < G; ++k) {
        const uint32_t r = gmm_z[s2g_z[k]];
        trng[k / kSlotTile] = slot_join(trng[k / kSlotTile], r);
        crng[k / kSlotChunk] = slot_join(crng[k / kSlotChunk], r);
    }
}

// One bit row of the class table (W words) from slot-order columns into gene-order columns: out bit j = in bit g2s[j] for j < G, columns
// from G on are zero.  (k1_unslot_words and k1_unslot_columns do this for every row and plane.)
inline void slot_unpermute_row(const uint32_t *in, uint32_t *out, int W, const uint32_t *g2s, int G)
{
    for (int w = 0; w < W; ++w) out[w] = 0;
    for (int j = 0; j < G; ++j) {
        const uint32_t k = g2s[j];
        out[j >> 5] |= ((in[k >> 5] >> (k & 31)) & 1u) << (j & 31);
    }
}

// ---- the WORD forms of the column un-permute (kernels.hip, k1_unslot_words): the permutation is the same for every row and plane, so
// the bits of a group of R consecutive table rows (whole rows: four planes of Wp words) travel together.  A 4R x 32 bit block -- the
// words (row r, plane p, slot word w) -- is transposed so that ONE entry holds one slot column of all R rows and four planes; the
// entries of all slots of the group wait in LDS (T); gene word wo takes the entries of its 32 genes' slots, T[g2s[32 wo + c]], and a
// second transpose makes the group's words (row r, plane p, gene word wo) of them.
//   wide form   R = 8: 32-bit entries, one word of T per slot
//   narrow form R = 4: 16-bit entries, two per word of T (the gene counts whose wide T no longer fits a workgroup's LDS)
constexpr int kUnslotWide = 8, kUnslotNarrow = 4;   // a form is named by its rows per group
constexpr size_t kUnslotLdsLimit = 160 * 1024;       // LDS a workgroup may have
constexpr int kUnslotThreadsMax = 1024;              // threads of a workgroup at most (k1_unslot_words is compiled for this bound)

// which bit of an entry is (row r of the group, plane p)
REO_SLOTS_HD int unslot_bit(int row, int plane) { return 4 * row + plane; }

// Where slot k's entry lies in T: the WORD index (wide) or the HALFWORD index (narrow).  The 32 entries of slot word w are stored by one
// thread, neighbouring threads hold neighbouring w: 33 words per 32 entries (wide), 17 words per 32 entries with the entries of slots
// b and b + 16 sharing a word (narrow: what the 16 x 32 transpose leaves in one register), keep a wave's stores off each other's banks.
REO_SLOTS_HD uint32_t unslot_lds_index(int form, uint32_t k)
{
    const uint32_t w = k >> 5, b = k & 31u;
    return form == kUnslotWide ? 33u * w + b : 2u * (17u * w + (b & 15u)) + (b >> 4);
}

// bytes of T for Gp slots
REO_SLOTS_HD size_t unslot_lds_bytes(int form, int Gp) { return static_cast<size_t>(Gp / 32) * (form == kUnslotWide ? 33u * 4u : 17u * 4u); }

// The word form for Gp slots, from the LDS it needs: narrow while THREE of its workgroups share a CU's LDS (up to 25 600 slots: measured
// faster than wide at 5 120 and 20 480, equal within the spread at 10 240; profiles/unslot_words_forms_sweep.txt), else wide while its T fits at all (up to 38 912: one workgroup per CU, yet
// faster than two narrow ones at 30 720 and 38 912 -- half the groups, twice the bytes in flight per thread), else narrow (fits 65 536).
REO_SLOTS_HD int unslot_form(int Gp)
{
    if (3 * unslot_lds_bytes(kUnslotNarrow, Gp) <= kUnslotLdsLimit) return kUnslotNarrow;
    return unslot_lds_bytes(kUnslotWide, Gp) <= kUnslotLdsLimit ? kUnslotWide : kUnslotNarrow;
}

// threads of a workgroup whose threads each take every blockDim-th of Wp words: as few trips as the bound allows, then as few threads
REO_SLOTS_HD int unslot_threads(int Wp)
{
    const int trips = (Wp + kUnslotThreadsMax - 1) / kUnslotThreadsMax;
    return ((Wp + trips - 1) / trips + 63) / 64 * 64;
}

#if defined(__clang__)
#define REO_SLOTS_UNROLL _Pragma("unroll")
#else
#define REO_SLOTS_UNROLL
#endif

// N x N bit blocks of N words transposed in place by masked swaps (N = 32: one block; N = 16: the blocks of columns 0-15 and 16-31 side
// by side): afterwards bit q of w[i] is what bit i of w[q] was (N = 16: and bit 16 + q of w[i] what bit 16 + i of w[q] was).  Its own inverse.
template <int N>
REO_SLOTS_HD void unslot_transpose(uint32_t (&w)[N])
{
    static_assert(N == 32 || N == 16, "4 R words");
    uint32_t m = N == 32 ? 0x0000FFFFu : 0x00FF00FFu;
    REO_SLOTS_UNROLL
    for (int j = N / 2; j != 0; j >>= 1, m ^= (m << j)) {
        REO_SLOTS_UNROLL
        for (int k = 0; k < N; k = (k + j + 1) & ~j) {
            const uint32_t t = ((w[k] >> j) ^ w[k + j]) & m;
            w[k] ^= t << j;
            w[k + j] ^= t;
        }
    }
}

// The steps of k1_unslot_words for one (slot or gene) word, shared by the kernel and the host model below.  T: the LDS image as words.
// in: the 4R words (row r, plane p, slot word w) at m[unslot_bit(r, p)] (rows the group does not have: 0) -> their entries into T
template <int R>
REO_SLOTS_HD void unslot_in_word(uint32_t (&m)[4 * R], int w, uint32_t *T)
{
    unslot_transpose<4 * R>(m);
    if (R == kUnslotWide) {
        REO_SLOTS_UNROLL
        for (int b = 0; b < 4 * R; ++b) T[unslot_lds_index(R, 32u * w + b)] = m[b];
    } else {
        REO_SLOTS_UNROLL
        for (int i = 0; i < 4 * R; ++i) T[unslot_lds_index(R, 32u * w + i) >> 1] = m[i];   // (the entries of slots 32 w + i and 32 w + 16 + i)
    }
}

// out: the entries of gene word wo's 32 slots (ks[c] = g2s[32 wo + c], clamped into the table) out of T -> the 4R words (row r, plane p,
// gene word wo) in u[unslot_bit(r, p)], columns from G on zero
template <int R>
REO_SLOTS_HD void unslot_out_word(uint32_t (&u)[4 * R], const uint32_t (&ks)[32], int wo, const uint32_t *T, int G, int Gp)
{
    if (R == kUnslotWide) {
        REO_SLOTS_UNROLL
        for (int c = 0; c < 32; ++c) {
            const uint32_t k = ks[c] < static_cast<uint32_t>(Gp) ? ks[c] : static_cast<uint32_t>(Gp - 1);
            u[c % (4 * R)] = T[unslot_lds_index(R, k)];
        }
    } else {
        const uint16_t *T16 = reinterpret_cast<const uint16_t *>(T);
        REO_SLOTS_UNROLL
        for (int c = 0; c < 32; ++c) {
            const uint32_t k = ks[c] < static_cast<uint32_t>(Gp) ? ks[c] : static_cast<uint32_t>(Gp - 1);
            const uint32_t e = T16[unslot_lds_index(R, k)];
            if (c < 16) u[c % (4 * R)] = e;
            else u[c % (4 * R)] |= e << 16;
        }
    }
    unslot_transpose<4 * R>(u);
    const int left = G - 32 * wo;   // columns of this word that are genes
    const uint32_t valid = left >= 32 ? 0xFFFFFFFFu : (left <= 0 ? 0u : (1u << left) - 1u);
    REO_SLOTS_UNROLL
    for (int q = 0; q < 4 * R; ++q) u[q] &= valid;
}

// The serial host model of one workgroup of k1_unslot_words<R>: rows r0 .. r0 + R - 1 of a table of n_rows rows (whole rows, Wp words
// per plane; the class table has n_rows = G) from slot-order columns into gene-order columns, in place; rows from n_rows on are neither
// read nor written.  T: unslot_lds_bytes(R, 32 Wp).
template <int R>
inline void unslot_group_model(uint32_t *table, int r0, int n_rows, int G, int Wp, const uint32_t *g2s, uint32_t *T)
{
    const int nr = n_rows - r0 < R ? n_rows - r0 : R;
    if (nr <= 0) return;
    uint32_t *rows = table + static_cast<size_t>(r0) * 4 * Wp;
    for (int w = 0; w < Wp; ++w) {
        uint32_t m[4 * R];
        for (int q = 0; q < 4 * R; ++q) m[q] = q < 4 * nr ? rows[static_cast<size_t>(q) * Wp + w] : 0u;
        unslot_in_word<R>(m, w, T);
    }
    for (int wo = 0; wo < Wp; ++wo) {   // (behind the barrier)
        uint32_t u[4 * R], ks[32];
        for (int c = 0; c < 32; ++c) ks[c] = g2s[32 * wo + c];
        unslot_out_word<R>(u, ks, wo, T, G, 32 * Wp);
        for (int q = 0; q < 4 * nr; ++q) rows[static_cast<size_t>(q) * Wp + wo] = u[q];
    }
}

// ---- the PAIR form of the word un-permute (per-side order: k1_unslot_pair): a side's two planes have that side's slot order, so a
// workgroup takes 2R rows of ONE side's plane pair -- the same 4R x 32 bit blocks, entries, T and transposes as above, another meaning
// of an entry's bits -- and uses that side's g2s.
REO_SLOTS_HD int unslot_pair_bit(int row, int plane) { return 2 * row + plane; }   // row of the group's 2R, plane 0 / 1 of the side's pair
// where the word of entry bit q lies among the group's rows (whole rows: four planes of Wp words), in words from the group's first row
REO_SLOTS_HD size_t unslot_pair_word(int q, int side, int Wp, int w) { return (static_cast<size_t>(q >> 1) * 4 + 2 * side + (q & 1)) * Wp + w; }

// The serial host model of one workgroup of k1_unslot_pair<R>: planes 2 side and 2 side + 1 of rows r0 .. r0 + 2R - 1, in place, with
// g2s the map of that side; the side's other planes and the rows from n_rows on are neither read nor written.
template <int R>
inline void unslot_pair_model(uint32_t *table, int r0, int n_rows, int side, int G, int Wp, const uint32_t *g2s, uint32_t *T)
{
    const int nr = n_rows - r0 < 2 * R ? n_rows - r0 : 2 * R;
    if (nr <= 0) return;
    uint32_t *rows = table + static_cast<size_t>(r0) * 4 * Wp;
    for (int w = 0; w < Wp; ++w) {
        uint32_t m[4 * R];
        for (int q = 0; q < 4 * R; ++q) m[q] = q < 2 * nr ? rows[unslot_pair_word(q, side, Wp, w)] : 0u;
        unslot_in_word<R>(m, w, T);
    }
    for (int wo = 0; wo < Wp; ++wo) {   // (behind the barrier)
        uint32_t u[4 * R], ks[32];
        for (int c = 0; c < 32; ++c) ks[c] = g2s[32 * wo + c];
        unslot_out_word<R>(u, ks, wo, T, G, 32 * Wp);
        for (int q = 0; q < 2 * nr; ++q) rows[unslot_pair_word(q, side, Wp, wo)] = u[q];
    }
}

// ---- the slot form's OPERANDS straight from the 16-bit position rows (kernels.hip, k1_slot_slice).  A slot build is tie-free, so
// lo = pos in every sample: both operand sets of the pair kernel are the bit planes of pos[.][s2g[k]], in the two layouts of the gene-order
// planes (transform.hip, t_slice):
//   Ps [(b 4 + q) Gp + k]      planes 4q .. 4q + 3 of slot k in sample block b (16 bytes)
//   ALs[(b Gp + k) 4 .. + 3]   the same 16 plane words as one 64-byte record, plane p in word (p + 15) % 16
// Sample block b uses the map of the side that counts it: side 0 the blocks cb .. ce - 1, side 1 every other one (the launch's block
// ranges, not group ids: comparison 1 swaps the groups).
struct alignas(16) SlotQuad { uint32_t x, y, z, w; };   // 16 bytes that travel as one

REO_SLOTS_HD int slot_slice_side(int b, int cb, int ce) { return (b >= cb && b < ce) ? 0 : 1; }
REO_SLOTS_HD size_t slot_slice_pos_index(int b, int q, int k, int Gp) { return (static_cast<size_t>(b) * 4 + q) * Gp + k; }   // in quads
REO_SLOTS_HD size_t slot_slice_rec_index(int b, int k, int Gp) { return (static_cast<size_t>(b) * Gp + k) * 4; }               // in quads
REO_SLOTS_HD int slot_slice_rec_word(int plane) { return (plane + 15) & 15; }

// Two genes of block b and their slots k0, k1: w[s] = the position of the first in sample 32 b + s | the second's << 16.  One 32 x 32
// bit transpose makes the 16 planes of both (w[p], w[16 + p]), which leave in both layouts.
REO_SLOTS_HD void slot_slice_store(uint32_t (&w)[32], int b, int k0, int k1, int Gp, SlotQuad *Ps, SlotQuad *ALs)
{
    unslot_transpose<32>(w);
    REO_SLOTS_UNROLL
    for (int h = 0; h < 2; ++h) {
        const uint32_t *v = w + 16 * h;
        const int k = h ? k1 : k0;
        REO_SLOTS_UNROLL
        for (int q = 0; q < 4; ++q) Ps[slot_slice_pos_index(b, q, k, Gp)] = SlotQuad{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
        SlotQuad *r = ALs + slot_slice_rec_index(b, k, Gp);
        r[0] = SlotQuad{v[1], v[2], v[3], v[4]};
        r[1] = SlotQuad{v[5], v[6], v[7], v[8]};
        r[2] = SlotQuad{v[9], v[10], v[11], v[12]};
        r[3] = SlotQuad{v[13], v[14], v[15], v[0]};
    }
}

// The rule as a serial host model, by SLOTS: pos16 [32 nblk][Gp] (rows of padding slots and columns of padded genes hold zeros), s2g [2][Gp]
inline void slot_slice_model(const uint16_t *pos16, const uint32_t *s2g, int Gp, int nblk, int cb, int ce, SlotQuad *Ps, SlotQuad *ALs)
{
    for (int b = 0; b < nblk; ++b) {
        const uint32_t *map = s2g + static_cast<size_t>(slot_slice_side(b, cb, ce)) * Gp;
        for (int k = 0; k < Gp; k += 2) {
            uint32_t w[32];
            for (int s = 0; s < 32; ++s) {
                const uint16_t *row = pos16 + (static_cast<size_t>(b) * 32 + s) * Gp;
                w[s] = static_cast<uint32_t>(row[map[k]]) | static_cast<uint32_t>(row[map[k + 1]]) << 16;
            }
            slot_slice_store(w, b, k, k + 1, Gp, Ps, ALs);
        }
    }
}

// The same by GENES (the form k1_slot_slice runs: coalesced reads of the rows, the 16-byte pieces scattered to their slots): two
// neighbouring genes g (even), g + 1 go to the slots g2s[g], g2s[g + 1] of the block's side.  g2s [2][Gp] must be the inverse of s2g
// over all Gp slots (padding genes map to themselves); a common order (sides == 1) fills its first half only.
inline void slot_slice_scatter_model(const uint16_t *pos16, const uint32_t *g2s, int sides, int Gp, int nblk, int cb, int ce, SlotQuad *Ps, SlotQuad *ALs)
{
    for (int b = 0; b < nblk; ++b) {
        const uint32_t *map = g2s + static_cast<size_t>(sides == 2 ? slot_slice_side(b, cb, ce) : 0) * Gp;
        for (int g = 0; g < Gp; g += 2) {
            uint32_t w[32];
            for (int s = 0; s < 32; ++s) {
                const uint16_t *row = pos16 + (static_cast<size_t>(b) * 32 + s) * Gp;
                w[s] = static_cast<uint32_t>(row[g]) | static_cast<uint32_t>(row[g + 1]) << 16;
            }
            slot_slice_store(w, b, static_cast<int>(map[g]), static_cast<int>(map[g + 1]), Gp, Ps, ALs);
        }
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
