// The slot form's operands straight from the 16-bit position rows (csrc/k1_slots.h: slot_slice_model, the host model of k1_slot_slice)
// without a GPU.  They must be, bit for bit, what the two steps they replace make: the gene-order planes in t_slice's two layouts
//   P [(b 4 + q) Gp + g]     word p % 4 of quad q = p / 4 is plane p of pos of gene g in sample block b (bit s = sample 32 b + s)
//   AL[(b Gp + g) 4 .. + 3]  the same 16 plane words of lo (= pos: tie-free data), plane p in word (p + 15) % 16
// written here one bit at a time, and k1_slot_gather's copy Ps[.. k] = P[.. s2g_side(b)[k]], ALs[b Gp + k] = AL[b Gp + s2g_side(b)[k]],
// with the side by the launch's block ranges.  Two DIFFERENT maps, side 0 first and side 1 first, padding sample slots and padded genes
// zero, every one of the 16 plane words.  The kernel walks the GENES and scatters (slot_slice_scatter_model, through g2s): it must write
// the same words, with an order per side and with the common order's one map.  Built with AddressSanitizer and UBSan by tests/test_slot_slice_cpu.py: every buffer is allocated
// at exactly the size the rules report.
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

static int padded(int G) { return (G + 1023) / 1024 * 1024; }

// a map of Gp slots: a random permutation of the genes below G, padding slots map to themselves
static void make_map(int G, int Gp, std::mt19937 &rng, uint32_t *s2g)
{
    std::iota(s2g, s2g + Gp, 0u);
    std::shuffle(s2g, s2g + G, rng);
}

// the gene-order planes in t_slice's layouts, one bit at a time (words, four per quad)
static void planes_by_bits(const std::vector<uint16_t> &pos16, int Gp, int nblk, std::vector<uint32_t> &P, std::vector<uint32_t> &AL)
{
    P.assign(static_cast<size_t>(nblk) * 4 * Gp * 4, 0u);
    AL.assign(static_cast<size_t>(nblk) * Gp * 16, 0u);
    for (int b = 0; b < nblk; ++b)
        for (int g = 0; g < Gp; ++g)
            for (int p = 0; p < 16; ++p) {
                uint32_t word = 0;
                for (int s = 0; s < 32; ++s) word |= static_cast<uint32_t>((pos16[(static_cast<size_t>(b) * 32 + s) * Gp + g] >> p) & 1u) << s;
                P[((static_cast<size_t>(b) * 4 + p / 4) * Gp + g) * 4 + p % 4] = word;
                AL[(static_cast<size_t>(b) * Gp + g) * 16 + (p + 15) % 16] = word;
            }
}

// k1_slot_gather on the host
static void gather(const std::vector<uint32_t> &P, const std::vector<uint32_t> &AL, const std::vector<uint32_t> &s2g, int Gp, int nblk, int cb, int ce,
                   std::vector<uint32_t> &Ps, std::vector<uint32_t> &ALs)
{
    Ps.assign(P.size(), 0xDEADBEEFu);
    ALs.assign(AL.size(), 0xDEADBEEFu);
    for (int b = 0; b < nblk; ++b) {
        const uint32_t *map = s2g.data() + ((b < cb || b >= ce) ? Gp : 0);
        for (int k = 0; k < Gp; ++k) {
            const uint32_t g = map[k];
            for (int q = 0; q < 4; ++q)
                for (int e = 0; e < 4; ++e) Ps[((static_cast<size_t>(b) * 4 + q) * Gp + k) * 4 + e] = P[((static_cast<size_t>(b) * 4 + q) * Gp + g) * 4 + e];
            for (int e = 0; e < 16; ++e) ALs[(static_cast<size_t>(b) * Gp + k) * 16 + e] = AL[(static_cast<size_t>(b) * Gp + g) * 16 + e];
        }
    }
}

// one size and one order of the sides: n0 real samples on the side of blocks [cb, ce), n1 on the other
static long slice_case(int G, int blocks0, int blocks1, bool side0_first, std::mt19937 &rng)
{
    const int Gp = padded(G), nblk = blocks0 + blocks1;
    const int cb = side0_first ? 0 : blocks1, ce = cb + blocks0;
    // real samples per side: the last block of each side is partly padding (rows of zeros)
    const int n0 = blocks0 * 32 - 5, n1 = blocks1 * 32 - 17;
    std::vector<uint16_t> pos16(static_cast<size_t>(nblk) * 32 * Gp, 0);
    std::vector<uint16_t> perm(G);
    for (int b = 0; b < nblk; ++b) {
        const int side = slot_slice_side(b, cb, ce), first = side ? (side0_first ? ce : 0) : cb, real = side ? n1 : n0;
        CHECK(side == ((b >= cb && b < ce) ? 0 : 1), "the side of block %d", b);
        for (int s = 0; s < 32; ++s) {
            if ((b - first) * 32 + s >= real) continue;   // a padding slot
            std::iota(perm.begin(), perm.end(), static_cast<uint16_t>(0));   // a sample's positions: a permutation of 0 .. G - 1
            std::shuffle(perm.begin(), perm.end(), rng);
            std::copy(perm.begin(), perm.end(), pos16.begin() + (static_cast<size_t>(b) * 32 + s) * Gp);
        }
    }
    std::vector<uint32_t> s2g(2 * static_cast<size_t>(Gp));
    make_map(G, Gp, rng, s2g.data());
    make_map(G, Gp, rng, s2g.data() + Gp);
    if (G > 2) CHECK(!std::equal(s2g.begin(), s2g.begin() + Gp, s2g.begin() + Gp), "two different maps at %d genes", G);

    std::vector<uint32_t> P, AL, Ps_ref, ALs_ref;
    planes_by_bits(pos16, Gp, nblk, P, AL);
    gather(P, AL, s2g, Gp, nblk, cb, ce, Ps_ref, ALs_ref);

    const size_t nq = static_cast<size_t>(nblk) * Gp * 4;   // quads of each operand set (kernels.hip, k1_slots_alloc)
    std::vector<SlotQuad> Ps(nq, SlotQuad{0xA5A5A5A5u, 0xA5A5A5A5u, 0xA5A5A5A5u, 0xA5A5A5A5u}), ALs(Ps);
    slot_slice_model(pos16.data(), s2g.data(), Gp, nblk, cb, ce, Ps.data(), ALs.data());

    long bad = 0, nonzero = 0;
    const uint32_t *pw = reinterpret_cast<const uint32_t *>(Ps.data()), *aw = reinterpret_cast<const uint32_t *>(ALs.data());
    for (size_t i = 0; i < nq * 4; ++i) { bad += pw[i] != Ps_ref[i]; bad += aw[i] != ALs_ref[i]; nonzero += pw[i] != 0; }
    CHECK(bad == 0, "%ld words differ at %d genes, %d + %d blocks, side %d first", bad, G, blocks0, blocks1, side0_first ? 0 : 1);
    // the form by genes (what the kernel runs by default): the inverse maps, every slot written once -- with an order per side, and with
    // the common order, whose g2s has one half only
    for (int sides = 2; sides >= 1; --sides) {
        std::vector<uint32_t> g2s(static_cast<size_t>(sides) * Gp), s2g_c(s2g);
        if (sides == 1) std::copy(s2g_c.begin(), s2g_c.begin() + Gp, s2g_c.begin() + Gp);   // the one map as the map of both sides
        for (int z = 0; z < sides; ++z)
            for (int k = 0; k < Gp; ++k) g2s[static_cast<size_t>(z) * Gp + s2g_c[static_cast<size_t>(z) * Gp + k]] = static_cast<uint32_t>(k);
        std::vector<SlotQuad> Pg(nq, SlotQuad{0x5A5A5A5Au, 0x5A5A5A5Au, 0x5A5A5A5Au, 0x5A5A5A5Au}), ALg(Pg), Pk(Pg), ALk(Pg);
        slot_slice_scatter_model(pos16.data(), g2s.data(), sides, Gp, nblk, cb, ce, Pg.data(), ALg.data());
        slot_slice_model(pos16.data(), s2g_c.data(), Gp, nblk, cb, ce, Pk.data(), ALk.data());
        const uint32_t *a0 = reinterpret_cast<const uint32_t *>(Pg.data()), *a1 = reinterpret_cast<const uint32_t *>(ALg.data());
        const uint32_t *b0 = reinterpret_cast<const uint32_t *>(Pk.data()), *b1 = reinterpret_cast<const uint32_t *>(ALk.data());
        long diff = 0;
        for (size_t i = 0; i < nq * 4; ++i) { diff += a0[i] != b0[i]; diff += a1[i] != b1[i]; }
        CHECK(diff == 0, "by genes and by slots: %ld words differ at %d genes, %d order(s)", diff, G, sides);
        if (sides == 2) { long d2 = 0; for (size_t i = 0; i < nq * 4; ++i) { d2 += a0[i] != Ps_ref[i]; d2 += a1[i] != ALs_ref[i]; } CHECK(d2 == 0, "by genes: %ld words differ from the composed models", d2); }
    }
    // the index rules themselves: plane p of slot k in block b at its place in both layouts, the record's word skewed by 15
    for (int t = 0; t < 64; ++t) {
        const int b = static_cast<int>(rng() % static_cast<unsigned>(nblk)), k = static_cast<int>(rng() % static_cast<unsigned>(Gp)), p = static_cast<int>(rng() % 16u);
        const uint32_t g = s2g[static_cast<size_t>(slot_slice_side(b, cb, ce)) * Gp + k];
        uint32_t word = 0;
        for (int s = 0; s < 32; ++s) word |= static_cast<uint32_t>((pos16[(static_cast<size_t>(b) * 32 + s) * Gp + g] >> p) & 1u) << s;
        CHECK(pw[slot_slice_pos_index(b, p / 4, k, Gp) * 4 + p % 4] == word, "Ps block %d slot %d plane %d", b, k, p);
        CHECK(aw[slot_slice_rec_index(b, k, Gp) * 4 + slot_slice_rec_word(p)] == word, "ALs block %d slot %d plane %d", b, k, p);
        CHECK(slot_slice_rec_word(p) == (p + 15) % 16, "the skew of plane %d", p);
    }
    // padded genes (slots G .. Gp - 1 map to themselves) and padding sample slots read as zero
    for (int b = 0; b < nblk; ++b) {
        for (int k = G; k < Gp; ++k)
            for (int e = 0; e < 16; ++e) {
                CHECK(pw[slot_slice_pos_index(b, e / 4, k, Gp) * 4 + e % 4] == 0, "padded slot %d of block %d in Ps", k, b);
                CHECK(aw[slot_slice_rec_index(b, k, Gp) * 4 + e] == 0, "padded slot %d of block %d in ALs", k, b);
            }
    }
    const int lastb[2] = {ce - 1, side0_first ? nblk - 1 : cb - 1};
    const uint32_t padmask[2] = {~0u << (32 - 5), ~0u << (32 - 17)};   // the sample bits of the padding slots in each side's last block
    for (int z = 0; z < 2; ++z)
        for (int k = 0; k < Gp; ++k)
            for (int e = 0; e < 16; ++e) CHECK((aw[slot_slice_rec_index(lastb[z], k, Gp) * 4 + e] & padmask[z]) == 0, "padding samples of side %d, slot %d", z, k);
    return nonzero;
}

int main()
{
    std::mt19937 rng(20240917u);
    long nonzero = 0;
    int cases = 0;
    const int sizes[] = {2, 33, 257, 1000, 2049, 65535};
    for (int G : sizes)
        for (int first = 0; first < 2; ++first) {
            const bool large = G > 4096;   // (the bit-by-bit planes of 65 536 slots: two blocks are 4 M words)
            nonzero += slice_case(G, large ? 1 : 2, large ? 1 : 3, first == 0, rng);
            ++cases;
        }
    // positions of G genes use the low planes only (all 16 at 65 535): random 16-bit numbers keep every plane word busy at a small size
    // too, here with side 0's block range in the middle (side 1 on both ends)
    {
        const int G = 257, Gp = padded(G), nblk = 4, cb = 1, ce = 3;
        std::vector<uint16_t> pos16(static_cast<size_t>(nblk) * 32 * Gp, 0);
        for (size_t i = 0; i < pos16.size(); ++i) if (static_cast<int>(i % Gp) < G) pos16[i] = static_cast<uint16_t>(rng());   // every plane word busy
        std::vector<uint32_t> s2g(2 * static_cast<size_t>(Gp)), P, AL, Ps_ref, ALs_ref;
        make_map(G, Gp, rng, s2g.data());
        make_map(G, Gp, rng, s2g.data() + Gp);
        planes_by_bits(pos16, Gp, nblk, P, AL);
        gather(P, AL, s2g, Gp, nblk, cb, ce, Ps_ref, ALs_ref);
        std::vector<SlotQuad> Ps(static_cast<size_t>(nblk) * Gp * 4), ALs(Ps.size());
        slot_slice_model(pos16.data(), s2g.data(), Gp, nblk, cb, ce, Ps.data(), ALs.data());
        long bad = 0;
        const uint32_t *pw = reinterpret_cast<const uint32_t *>(Ps.data()), *aw = reinterpret_cast<const uint32_t *>(ALs.data());
        for (size_t i = 0; i < Ps.size() * 4; ++i) { bad += pw[i] != Ps_ref[i]; bad += aw[i] != ALs_ref[i]; }
        CHECK(bad == 0, "%ld words differ with side 1 on both ends and 16 busy planes", bad);
        ++cases;
    }
    if (fails) { std::printf("%d failures\n", fails); return 1; }
    std::printf("ok slice cases %d nonzero_words %ld\n", cases, nonzero);
    return 0;
}
