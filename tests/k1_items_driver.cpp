// Driver of test_k1_item_lists_keep_their_order (tests/test_sharding_cpu.py): for a fixed table of launch geometries, the
// length and the 64-bit FNV-1a digest of the item list that csrc/k1_items.h makes.  Plain host C++.
//   g++ -std=c++17 -I rankcompv3.jl_amd/csrc -o driver tests/k1_items_driver.cpp && ./driver
#include <cstdio>

#include "k1_items.h"

struct Case {
    const char *name;
    int G, cblk, tblk, allblk;   // genes; 32-sample blocks of the comparison's group, of the rest, of all groups
    bool wave;                   // two groups in the wave form (an item per side); else the one-side group-counts form
    int sides, order, half, world, rank, part, nparts;   // part of nparts: the units of one wave of a pipelined exchange
};

static const Case kCases[] = {
    {"config3", 20000, 16, 16, 32, true, 3, 0, 1, 1, 0, 0, 1},            // BASELINE config 3 as the bench runs it
    {"config3_side_own", 20000, 16, 16, 32, true, 1, 0, 1, 1, 0, 0, 1},   // ... and as the pipelined upload launches its sides
    {"config3_side_rest", 20000, 16, 16, 32, true, 2, 0, 1, 1, 0, 0, 1},
    {"config3_order1", 20000, 16, 16, 32, true, 3, 1, 1, 1, 0, 0, 1},
    {"config3_order2", 20000, 16, 16, 32, true, 3, 2, 1, 1, 0, 0, 1},
    {"config3_no_halves", 20000, 16, 16, 32, true, 3, 0, 0, 1, 0, 0, 1},  // REO_K1_HALF=0
    {"config4", 30000, 63, 63, 126, true, 3, 0, 1, 1, 0, 0, 1},           // BASELINE config 4 as the bench runs it
    {"config4_order2", 30000, 63, 63, 126, true, 3, 2, 1, 1, 0, 0, 1},    // (the i-tile block of order 2 shrinks)
    {"config4_shard3of8", 30000, 63, 63, 126, true, 3, 0, 1, 8, 3, 0, 1},
    {"config4_shard3of8_wave2of4", 30000, 63, 63, 126, true, 3, 0, 1, 8, 3, 2, 4},
    {"config2", 5000, 4, 4, 8, true, 3, 0, 1, 1, 0, 0, 1},                // four j-chunks per panel
    {"g26000", 26000, 16, 16, 32, true, 3, 0, 1, 1, 0, 0, 1},
    {"big17", 70000, 4, 4, 8, true, 3, 0, 1, 1, 0, 0, 1},                 // 17 planes: two waves per SIMD
    {"big17_shard1of2", 70000, 4, 4, 8, true, 3, 0, 1, 2, 1, 0, 1},
    {"wide", 3000, 1100, 1100, 2200, true, 3, 0, 1, 1, 0, 0, 1},          // more than 65 535 samples
    {"group_counts3", 8000, 4, 8, 12, false, 3, 0, 1, 1, 0, 0, 1},        // three groups, shared counts: one side, all groups' blocks
    {"group_counts5_order1", 12000, 7, 28, 35, false, 3, 1, 1, 1, 0, 0, 1},
};

int main()
{
    constexpr int kTileI = reo::kItemTileI, kUnitH = reo::kItemUnitH, kRJ = 4, kTileJ = 256, kGenePad = 1024;
    for (const Case &t : kCases) {
        // the geometry and the owned units as launch_k1 makes them (tests/sharding_mirror.py, geometry / tile_owner)
        const int Gp = (t.G + kGenePad - 1) / kGenePad * kGenePad, RJ = kRJ, CJ = kTileJ * RJ;
        const int NJ = (Gp + CJ - 1) / CJ, NIT = Gp / kTileI;
        const size_t chunk_bytes = static_cast<size_t>(CJ) * t.allblk * 64;
        const int Q = chunk_bytes * 4 <= (2u << 20) ? 4 : (chunk_bytes * 2 <= (2u << 20) ? 2 : 1);
        const int NP = (NJ + Q - 1) / Q;
        std::vector<uint32_t> owned;
        uint32_t gu = 0, all = 0;
        for (int p = 0; p < NP; ++p) {
            const int ni = std::min(NIT, (CJ / kTileI) * Q * (p + 1));
            for (int r = 0; r * kUnitH < ni; ++r, ++gu, ++all)
                if (t.world == 1 || static_cast<int>(gu % t.world) == t.rank) owned.push_back(static_cast<uint32_t>(p) << 16 | static_cast<uint32_t>(r));
        }
        std::vector<uint32_t> units = owned;
        if (t.nparts > 1) {   // the slots of one wave: the same count on every shard
            const int maxu = std::max(1, (static_cast<int>(all) + t.world - 1) / t.world), mw = (maxu + t.nparts - 1) / t.nparts;
            units.clear();
            for (size_t m = 0; m < owned.size(); ++m)
                if (static_cast<int>(std::min<size_t>(m / mw, t.nparts - 1)) == t.part) units.push_back(owned[m]);
        }
        reo::K1ItemGeom g;
        g.G = t.G; g.RJ = RJ; g.CJ = CJ; g.Q = Q;
        g.nsides = t.wave ? 2u : 1u; g.sides = t.sides;
        g.wave = t.wave; g.wide = 32 * t.allblk > 65535; g.big = t.G > 65535;
        g.halves = g.wave && !g.wide && t.half;
        g.side_blocks = t.wave ? std::max(t.cblk, t.tblk) : t.allblk;
        g.order = t.order; g.n_cus = 256;
        const std::vector<uint32_t> items = reo::k1_item_list(g, units);
        uint64_t h = 0xcbf29ce484222325ULL;
        size_t halves = 0;
        for (uint32_t x : items) {
            for (int b = 0; b < 4; ++b) { h ^= (x >> (8 * b)) & 0xFFu; h *= 0x100000001b3ULL; }
            halves += (x >> 15) & 1u;
        }
        printf("%s %zu %zu %016llx\n", t.name, items.size(), halves, static_cast<unsigned long long>(h));
    }
    return 0;
}
