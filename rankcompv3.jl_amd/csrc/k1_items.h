// The item list of the wave form of the pair kernel (kernels.hip, launch_k1): which (side, wave chunk, i-tile) workgroup b of a
// launch works on.  Plain host C++ -- no context, no HIP -- so that the order, which decides what every XCD's L2 sees,
// can be pinned by a CPU test (tests/test_sharding_cpu.py, tests/golden/k1_item_lists.json).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace reo {

constexpr int kItemTileI = 32;   // = kTileI and kUnitH of reo_internal.h (kernels.hip checks both)
constexpr int kItemUnitH = 32;

struct K1ItemGeom {
    int G;              // genes
    int RJ, CJ, Q;      // genes j per lane, per j-chunk; j-chunks per panel
    uint32_t nsides;    // 2: two groups, an item per side; 1: group counts, an item counts all groups' blocks
    int sides;          // nsides 2: which sides are wanted (bit 0 the comparison's own group, bit 1 the rest)
    bool wave, wide, big;   // two groups in the wave form; more than 65 535 samples (no halves then); more than 65 535 genes
    bool halves;        // deal the items of the last round as two half-height items each (k1w_pairs only)
    int side_blocks;    // 32-sample blocks an item runs over (the larger side's; group counts: all of them)
    int order;          // REO_K1_ORDER
    int n_cus;          // compute units of the device
};

// item = side << 31 | wave chunk << 16 | i-tile (half-height items: bit 15 set, bit 14 = which half); the units
// (panel << 16 | i-range) in order, side-major, i-tile-major, wave chunks fastest -- then arranged by XCD:
inline std::vector<uint32_t> k1_item_list(const K1ItemGeom &g, const std::vector<uint32_t> &units)
{
    const int RJ = g.RJ, CJ = g.CJ, Q = g.Q, sides = g.sides, side_blocks = g.side_blocks, order = g.order;
    const uint32_t nsides = g.nsides;
    const bool wave = g.wave, big = g.big, halves = g.halves;
    const int CW = 64 * RJ, QW = Q * (CJ / CW);
    std::vector<uint32_t> items;
    // Workgroup b runs on XCD b & 7.  An item goes to the list of XCD (wave chunk & 7), and an XCD walks its list
    // group by group of its chunks (as many pos chunks of one side as fit about 2.5 MB of its 4 MiB L2), inside a
    // group side-major, then i-tile-major, chunks fastest: the group's pos planes stay in that L2 while each tile
    // operand (32 rows x the side's blocks) streams through it once per group.  (Dealing the items of the
    // unit-by-unit order one at a time made every XCD touch every chunk and re-read every tile operand per unit:
    // 2.0 GB of L2 fills per launch at config 3, against 0.24 GB algorithmic.)  The lists are then levelled by
    // moving the surplus of the long ones -- their last items -- to the short ones, and interleaved.
    std::vector<uint32_t> lists[8];
    const int G = g.G;
    size_t total_items = 0;
    const size_t chunk_side_bytes = static_cast<size_t>(CW) * std::max(side_blocks, 1) * 64;
    const int per_group = static_cast<int>(std::max<size_t>(1, (size_t(5) << 19) / chunk_side_bytes));  // chunks of one XCD per group
    uint32_t tile_block = 32;   // (order 2) i-tiles per block: their tile operands together about 1 MB, a power of two from 4 to 32
    while (tile_block > 4 && static_cast<size_t>(tile_block) * kItemTileI * std::max(side_blocks, 1) * (big ? 128 : 64) > (size_t(1) << 20)) tile_block >>= 1;
    for (uint32_t um : units)
        for (uint32_t side = 0; side < nsides; ++side) {
            if (wave && !((sides >> side) & 1)) continue;
            for (int t = 0; t < kItemUnitH; ++t)
                for (int w = 0; w < QW; ++w) {
                    const int it = static_cast<int>(um & 0xFFFFu) * kItemUnitH + t, cw = static_cast<int>(um >> 16) * QW + w;
                    const int i0 = it * kItemTileI, jw = cw * CW;
                    if (i0 >= G || jw >= G || ((jw + CW - 1) >> 6) < (i0 >> 6)) continue;  // no pair i < j < G in it
                    lists[cw & 7].push_back(side << 31 | static_cast<uint32_t>(cw) << 16 | static_cast<uint32_t>(it));
                    ++total_items;
                }
        }
    // order inside an XCD's list: chunk group, side, i-tile, chunk -- sorted as one 64-bit key per item (the comparator form,
    // with its two divisions per comparison, took 0.9 ms per side at config 3)
    std::vector<uint64_t> keys;
    for (auto &l : lists) {
        keys.resize(l.size());
        for (size_t q = 0; q < l.size(); ++q) {
            const uint32_t x = l[q], cx = (x >> 16) & 0x7FFFu;
            if (order == 0)
                keys[q] = static_cast<uint64_t>((cx >> 3) / static_cast<uint32_t>(per_group)) << 32 | static_cast<uint64_t>(x >> 31) << 31 |
                          static_cast<uint64_t>(x & 0xFFFFu) << 15 | cx;
            else if (order == 1)   // i-tiles fastest inside a chunk: the mirror words of a chunk's genes (one 32-bit word per i-tile,
                                   // neighbours in their table rows) reach L2 one after the other -- but every chunk re-reads every tile operand
                keys[q] = static_cast<uint64_t>((cx >> 3) / static_cast<uint32_t>(per_group)) << 48 | static_cast<uint64_t>(x >> 31) << 47 |
                          static_cast<uint64_t>(cx) << 16 | (x & 0xFFFFu);
            else   // 2: blocks of TB consecutive i-tiles; inside a block chunk by chunk, the block's tiles fastest: TB mirror words in a row
                   // (TB x 4 bytes of a table line) while the block's tile operands (TB x 32 rows x the side's blocks x 64 B: about 1 MB) stay in L2
                keys[q] = static_cast<uint64_t>((cx >> 3) / static_cast<uint32_t>(per_group)) << 48 | static_cast<uint64_t>(x >> 31) << 47 |
                          static_cast<uint64_t>((x & 0xFFFFu) / tile_block) << 31 | static_cast<uint64_t>(cx) << 16 | (x & 0xFFFFu);
        }
        std::sort(keys.begin(), keys.end());
        for (size_t q = 0; q < l.size(); ++q) {
            const uint64_t k = keys[q];
            if (order == 0) l[q] = static_cast<uint32_t>((k >> 31) & 1u) << 31 | static_cast<uint32_t>(k & 0x7FFFu) << 16 | static_cast<uint32_t>((k >> 15) & 0xFFFFu);
            else l[q] = static_cast<uint32_t>((k >> 47) & 1u) << 31 | static_cast<uint32_t>((k >> 16) & 0x7FFFu) << 16 | static_cast<uint32_t>(k & 0xFFFFu);
        }
    }
    const size_t per = (total_items + 7) / 8;
    std::vector<uint32_t> surplus;
    for (auto &l : lists)
        while (l.size() > per) { surplus.push_back(l.back()); l.pop_back(); }
    for (auto &l : lists)
        while (l.size() < per && !surplus.empty()) { l.push_back(surplus.back()); surplus.pop_back(); }
    items.reserve(total_items);
    for (size_t k = 0; k < per; ++k)
        for (auto &l : lists)
            if (k < l.size()) items.push_back(l[k]);
    // All items take the same time -- in the identity order.  (In slot order, k1_slots.h, they do not: a separated item writes constant
    // words and is gone, the others count for about 100 us.  There the list is not worked through in rounds of workgroups at all:
    // resident waves take its items from eight queues, item 8 m + x being entry m of queue x, and a wave whose queue is dry takes from
    // the others' -- k1_queue.h.  The list is the same for both orders: the levelling above still gives every queue the same NUMBER of
    // items, not the same time, and the halves below still shorten only the tail of a launch in rounds; neither is tuned for slot
    // order.  DESIGN 3.2 and 9.)  So the resident waves (slots) work through the list in rounds; when the last
    // round fills at most half of the slots, its items are dealt as two half-height items each (rows 0-15 and 16-31
    // of the tile: bit 15 set, bit 14 = which half) and the launch ends half an item's time earlier -- 0.45 of a round
    // out of 16.45 at config 3; a shard of one eighth of the tiles has 2.06 rounds.  Both halves of an item stay
    // on the item's XCD (the tail is a multiple of 8 items).
    if (halves && !items.empty()) {
        const size_t slots = static_cast<size_t>(g.n_cus) * 4 * (big ? 2 : 3);
        const size_t left = items.size() % slots;
        if (left > 0 && left <= slots / 2) {
            const size_t n = std::min(items.size(), (left + 7) / 8 * 8);
            const std::vector<uint32_t> tail(items.end() - static_cast<ptrdiff_t>(n), items.end());
            items.resize(items.size() - n);
            for (uint32_t half = 0; half < 2; ++half)
                for (uint32_t x : tail) items.push_back(x | 0x8000u | (half ? 0x4000u : 0u));
        }
    }
    return items;
}

}  // namespace reo
