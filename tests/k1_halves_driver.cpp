// Driver of test_half_height_items_at_18_planes (tests/test_big_plane_cases_cpu.py): the items that csrc/k1_items.h deals as two
// half-height items for a two-group launch of the wave form over all units of one shard, one line "side chunk tile" per item (chunk:
// 256 columns, tile: 32 rows), after a line "items halved".  Plain host C++, the geometry as launch_k1 makes it (tests/k1_items_driver.cpp).
//   g++ -std=c++17 -I rankcompv3.jl_amd/csrc -o driver tests/k1_halves_driver.cpp && ./driver GENES SIDE_BLOCKS COMPUTE_UNITS
#include <cstdio>
#include <cstdlib>
#include <set>

#include "k1_items.h"

int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    const int G = std::atoi(argv[1]), side_blocks = std::atoi(argv[2]), n_cus = std::atoi(argv[3]);
    constexpr int kTileI = reo::kItemTileI, kUnitH = reo::kItemUnitH, kRJ = 4, kTileJ = 256, kGenePad = 1024;
    const int Gp = (G + kGenePad - 1) / kGenePad * kGenePad, CJ = kTileJ * kRJ;
    const int NJ = (Gp + CJ - 1) / CJ, NIT = Gp / kTileI;
    const size_t chunk_bytes = static_cast<size_t>(CJ) * (2 * side_blocks) * 64;
    const int Q = chunk_bytes * 4 <= (2u << 20) ? 4 : (chunk_bytes * 2 <= (2u << 20) ? 2 : 1);
    const int NP = (NJ + Q - 1) / Q;
    std::vector<uint32_t> units;
    for (int p = 0; p < NP; ++p) {
        const int ni = std::min(NIT, (CJ / kTileI) * Q * (p + 1));
        for (int r = 0; r * kUnitH < ni; ++r) units.push_back(static_cast<uint32_t>(p) << 16 | static_cast<uint32_t>(r));
    }
    reo::K1ItemGeom g;
    g.G = G; g.RJ = kRJ; g.CJ = CJ; g.Q = Q;
    g.nsides = 2u; g.sides = 3;
    g.wave = true; g.wide = false; g.big = G > 65535;
    g.halves = true;
    g.side_blocks = side_blocks;
    g.order = 0; g.n_cus = n_cus;
    const std::vector<uint32_t> items = reo::k1_item_list(g, units);
    std::set<uint32_t> halved;
    size_t half_items = 0;
    for (uint32_t x : items)
        if (x & 0x8000u) { ++half_items; halved.insert(x & ~0x4000u); }
    if (half_items != 2 * halved.size()) return 3;   // every halved item is there as both halves
    printf("%zu %zu\n", items.size() - halved.size(), halved.size());
    for (uint32_t x : halved) printf("%u %u %u\n", x >> 31, (x >> 16) & 0x7FFFu, x & 0x3FFFu);
    return 0;
}
