// Host-only driver for csrc/top_pairs.h (tests/test_top_pairs_cpu.py builds it with -fsanitize=address,undefined and runs it): the functions
// that reo_top_pairs runs on the host and shares with the kernels of csrc/toppairs.hip.
//   no argument:
//   - tp_check_context / tp_check_shift_args / tp_check_args: every check with its number and message;
//   - tp_pack, tp_shr, tp_extend, tp_digit, tp_top, tp_cmp: the fields of a key, its ten digits put together again, the order of keys against
//     the order of (|N|, Gamma, i, j), shifts across the 64-bit seam;
//   - tp_num / tp_gamma / tp_shift / tp_bound_mask / tp_capacity on hand-made values;
//   - the tile rule: for G in {1, 2, 63, 64, 65, 300} the launch grid is enumerated -- workgroup, wave, row, lane, with tp_group_live,
//     tp_tile_live and tp_lane_live as the kernel applies them -- and every pair i < j is covered by exactly one live (tile, row, lane),
//     nothing else by any;
//   - tp_pick_digit on hand-made histograms: the n-th key in the first bin, in the last bin, behind keys above the prefix, and an empty
//     histogram;
//   - tp_select on a seeded list of keys with many equal |N| against a full sort, for several n and capacities.
//   Prints "ok <checks>"; anything on stderr is a failure.
//   `select`: reads "G n_want capacity n_max g_max n_pairs" and then n_pairs lines "|N| Gamma i j" from stdin, runs the library's own pass
//   loop (tp_select) with a host histogram over those keys in place of the kernel, collects the candidates as the emit pass would, sorts them
//   with the library's comparison and prints "passes <p>", "cand <c>" and one line "i j" per selected pair.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "top_pairs.h"

using namespace reo;

namespace {

long g_checks = 0, g_fail = 0;

uint64_t g_state = 0x243F6A8885A308D3ULL;
uint64_t rnd()   // splitmix64, seeded: the same words on every run
{
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

void expect(bool ok, const char *what, long a = 0, long b = 0)
{
    ++g_checks;
    if (!ok) { fprintf(stderr, "FAIL %s (%ld, %ld)\n", what, a, b); ++g_fail; }
}

void expect_msg(int got, int want, const char *msg, const char *needle)
{
    expect(got == want, "check number", got, want);
    expect(strstr(msg, needle) != nullptr, needle);
    if (!strstr(msg, needle)) fprintf(stderr, "  message was: %s\n", msg);
}

// The histogram of one pass over a list of keys, as k_top_pairs<HIST> fills it.
struct HostHist {
    const std::vector<TpKey> &keys;
    int operator()(const TpKey &prefix, int shift, uint64_t *bins) const
    {
        for (const TpKey &k : keys) {
            const int c = tp_cmp(tp_top(k, shift), prefix);
            ++bins[c > 0 ? kTpAbove : (c < 0 ? kTpBelow : static_cast<int>(tp_digit(k, shift)))];
        }
        return 0;
    }
};

// The whole selection on the host: pass loop, emit, sort, trim.  Returns the indices of the selected keys in order.
std::vector<size_t> select_host(const std::vector<TpKey> &keys, uint64_t n_max, uint64_t g_max, uint64_t want, uint64_t capacity, TpSelect *sel)
{
    std::vector<size_t> cand;
    const int rc = tp_select(HostHist{keys}, tp_bound_mask(n_max, g_max), want, capacity, sel);
    expect(rc == 0, "tp_select returns 0", rc);
    if (rc) return cand;
    for (size_t e = 0; e < keys.size(); ++e)
        if (tp_cmp(tp_shr(keys[e], sel->shift), sel->cut) >= 0) cand.push_back(e);
    expect(cand.size() == sel->n_cand, "the emit pass finds the candidates the passes counted", static_cast<long>(cand.size()), static_cast<long>(sel->n_cand));
    expect(cand.size() <= capacity, "the candidates fit the buffer", static_cast<long>(cand.size()), static_cast<long>(capacity));
    std::sort(cand.begin(), cand.end(), [&](size_t x, size_t y) { return tp_before(keys[x], keys[y]); });
    if (cand.size() > want) cand.resize(static_cast<size_t>(want));
    return cand;
}

void check_args()
{
    char msg[320];
    TpState ok{false, 1, false, 300, 64, 3};
    int32_t gi[4], gj[4], counts[16];
    int64_t key[8], found = 0, D[300];
    uint8_t mask[300];
    memset(mask, 1, sizeof mask);
    expect(tp_check_args(ok, 0, -1, nullptr, 4, gi, gj, counts, key, &found, msg, sizeof msg) == 0, "in order, no mask");
    expect(tp_check_args(ok, 2, 0, mask, 1 << 20, gi, gj, counts, key, &found, msg, sizeof msg) == 0, "in order, mask, largest n");
    expect(tp_check_shift_args(ok, 1, 2, D, msg, sizeof msg) == 0, "rank_shift in order");
    TpState st = ok;
    st.multi = true;
    expect_msg(tp_check_args(st, 0, -1, nullptr, 4, gi, gj, counts, key, &found, msg, sizeof msg), 1, msg, "reo_top_pairs is not available on a reo_create_multi context");
    expect_msg(tp_check_shift_args(st, 0, -1, D, msg, sizeof msg), 1, msg, "reo_rank_shift is not available on a reo_create_multi context");
    st = ok; st.world = 4;
    expect_msg(tp_check_args(st, 0, -1, nullptr, 4, gi, gj, counts, key, &found, msg, sizeof msg), 2, msg, "sharded context (reo_set_shard: 4 shards");
    st = ok; st.has_mask = true;
    expect_msg(tp_check_args(st, 0, -1, nullptr, 4, gi, gj, counts, key, &found, msg, sizeof msg), 3, msg, "reo_top_pairs compares on the bit planes of the whole matrix");
    char same[320];
    mp_query_refusal("reo_top_pairs", same, sizeof same);
    expect(strcmp(msg, same) == 0, "the sentence of the other plane readers");
    st = ok; st.G = 65536;
    expect_msg(tp_check_args(st, 0, -1, nullptr, 4, gi, gj, counts, key, &found, msg, sizeof msg), 4, msg, "G = 65536, at most 65535 genes");
    st = ok; st.S = 70000;
    expect_msg(tp_check_args(st, 0, -1, nullptr, 4, gi, gj, counts, key, &found, msg, sizeof msg), 5, msg, "S = 70000, at most 65535 samples");
    st = ok; st.G = 65535; st.S = 65535;
    expect(tp_check_args(st, 0, -1, nullptr, 4, gi, gj, counts, key, &found, msg, sizeof msg) == 0, "the largest problem");
    expect_msg(tp_check_args(ok, 3, -1, nullptr, 4, gi, gj, counts, key, &found, msg, sizeof msg), 6, msg, "a = 3 is outside the groups [0, 3)");
    expect_msg(tp_check_args(ok, -1, 0, nullptr, 4, gi, gj, counts, key, &found, msg, sizeof msg), 6, msg, "a = -1 is outside");
    expect_msg(tp_check_args(ok, 0, 3, nullptr, 4, gi, gj, counts, key, &found, msg, sizeof msg), 7, msg, "b = 3 is outside the groups [0, 3) and not -1");
    expect_msg(tp_check_args(ok, 0, -2, nullptr, 4, gi, gj, counts, key, &found, msg, sizeof msg), 7, msg, "b = -2 is outside");
    expect_msg(tp_check_args(ok, 1, 1, nullptr, 4, gi, gj, counts, key, &found, msg, sizeof msg), 8, msg, "b == a == 1");
    expect_msg(tp_check_args(ok, 0, -1, nullptr, 0, gi, gj, counts, key, &found, msg, sizeof msg), 9, msg, "n_want = 0, between 1 and 2^20");
    expect_msg(tp_check_args(ok, 0, -1, nullptr, (1 << 20) + 1, gi, gj, counts, key, &found, msg, sizeof msg), 9, msg, "n_want = 1048577");
    expect_msg(tp_check_args(ok, 0, -1, nullptr, -5, gi, gj, counts, key, &found, msg, sizeof msg), 9, msg, "n_want = -5");
    expect_msg(tp_check_args(ok, 0, -1, nullptr, 4, nullptr, gj, counts, key, &found, msg, sizeof msg), 10, msg, "must not be null");
    expect_msg(tp_check_args(ok, 0, -1, nullptr, 4, gi, gj, counts, nullptr, &found, msg, sizeof msg), 10, msg, "must not be null");
    expect_msg(tp_check_args(ok, 0, -1, nullptr, 4, gi, gj, counts, key, nullptr, msg, sizeof msg), 10, msg, "must not be null");
    mask[299] = 2;
    expect_msg(tp_check_args(ok, 0, -1, mask, 4, gi, gj, counts, key, &found, msg, sizeof msg), 11, msg, "gene_mask[299] = 2, a byte of the mask is 0 or 1");
    mask[299] = 0; mask[0] = 255;
    expect_msg(tp_check_args(ok, 0, -1, mask, 4, gi, gj, counts, key, &found, msg, sizeof msg), 11, msg, "gene_mask[0] = 255");
    expect_msg(tp_check_shift_args(ok, 0, -1, nullptr, msg, sizeof msg), 9, msg, "reo_rank_shift: D must not be null");
    expect_msg(tp_check_shift_args(ok, 2, 2, D, msg, sizeof msg), 8, msg, "reo_rank_shift: b == a == 2");
}

void check_keys()
{
    // the fields come back out of the key
    const uint64_t n = 0x7FFFFFFEull, g = 0xFEDCBA987654ull;
    const TpKey k = tp_pack(n, g, 65533, 65534, 65535);
    expect((k.hi >> 16) == n && (k.hi & 0xFFFF) == (g >> 32) && (k.lo >> 32) == (g & 0xFFFFFFFFull), "fields of the key");
    expect(static_cast<uint32_t>(k.lo) == 0xFFFFFFFFu - (65533u * 65535u + 65534u), "index field");
    expect(tp_shr(k, 80).lo == n && tp_shr(k, 80).hi == 0, "|N| sits at bit 80");
    expect((tp_shr(k, 32).lo & 0xFFFFFFFFFFFFull) == g, "Gamma sits at bit 32");
    expect(tp_shr(k, 120).lo == 0 && tp_shr(k, 111).lo == 0 && tp_shr(k, 110).lo == 1, "111 bits");
    // the ten digits put the key together again, and prefix / digit split it at every digit
    TpKey again{0, 0};
    for (int s = kTpKeyBits - kTpDigitBits; s >= 0; s -= kTpDigitBits) {
        expect(tp_cmp(tp_top(k, s), again) == 0, "the prefix in front of a digit", s);
        again = tp_extend(again, tp_digit(k, s));
    }
    expect(tp_cmp(again, k) == 0, "ten digits are the key");
    // shifts across the seam, against unsigned __int128
    for (int t = 0; t < 2000; ++t) {
        const TpKey r{rnd() >> 17, rnd()};
        const unsigned __int128 v = (static_cast<unsigned __int128>(r.hi) << 64) | r.lo;
        const int s = static_cast<int>(rnd() % 128);
        const TpKey got = tp_shr(r, s);
        const unsigned __int128 w = v >> s;
        expect(got.hi == static_cast<uint64_t>(w >> 64) && got.lo == static_cast<uint64_t>(w), "tp_shr", s);
    }
    for (int s : {0, 1, 63, 64, 65, 127}) {
        const TpKey r{0x0000123456789ABCull, 0xFEDCBA9876543210ull};
        const unsigned __int128 w = ((static_cast<unsigned __int128>(r.hi) << 64) | r.lo) >> s;
        expect(tp_shr(r, s).hi == static_cast<uint64_t>(w >> 64) && tp_shr(r, s).lo == static_cast<uint64_t>(w), "tp_shr at the seam", s);
    }
    // the order of keys is the order of the definition
    const int G = 500;
    for (int t = 0; t < 4000; ++t) {
        uint64_t f[2][4];
        for (auto &row : f) { row[0] = rnd() % 5; row[1] = rnd() % 3 ? rnd() % 4 : (rnd() >> 16); row[2] = rnd() % (G - 1); row[3] = row[2] + 1 + rnd() % (G - 1 - row[2]); }
        const TpKey x = tp_pack(f[0][0], f[0][1], static_cast<int>(f[0][2]), static_cast<int>(f[0][3]), G);
        const TpKey y = tp_pack(f[1][0], f[1][1], static_cast<int>(f[1][2]), static_cast<int>(f[1][3]), G);
        int want = 0;   // +1: x first
        if (f[0][0] != f[1][0]) want = f[0][0] > f[1][0] ? 1 : -1;
        else if (f[0][1] != f[1][1]) want = f[0][1] > f[1][1] ? 1 : -1;
        else if (f[0][2] != f[1][2]) want = f[0][2] < f[1][2] ? 1 : -1;
        else if (f[0][3] != f[1][3]) want = f[0][3] < f[1][3] ? 1 : -1;
        expect(tp_cmp(x, y) == want && tp_before(x, y) == (want > 0), "key order", t);
    }
    // N, Gamma, D
    expect(tp_num(5, 0, 0, 0, 5, 7) == 2 * 5 * 7 && tp_num(0, 0, 7, 0, 5, 7) == -2 * 5 * 7, "|N| reaches 2 S_A S_B");
    expect(tp_num(3, 1, 2, 4, 5, 7) == (2 * 3 + 1 - 5) * 7 - (2 * 2 + 4 - 7) * 5, "N from the counts");
    expect(tp_num(3, 1, 2, 4, 5, 7) == -tp_num(5 - 3 - 1, 1, 7 - 2 - 4, 4, 5, 7), "N is antisymmetric");
    expect(tp_num(0, 5, 0, 7, 5, 7) == 0, "all tied: 0");
    expect(tp_num(32768, 0, 0, 0, 32768, 32767) == 2ll * 32768 * 32767 && tp_num(0, 0, 32767, 0, 32768, 32767) == -2ll * 32768 * 32767, "the largest sides");
    expect(tp_gamma(-7, 9) == 16 && tp_gamma(9, -7) == 16 && tp_gamma(3, 3) == 0, "Gamma");
    expect(tp_gamma(-(int64_t(1) << 47), int64_t(1) << 47) == uint64_t(1) << 48, "Gamma at its bound");
    expect(tp_shift(10, 4, 3, 5) == 10 * 5 - 4 * 3, "D from the sums");
    // the bound mask and the digits it proves zero
    TpKey m = tp_bound_mask(288, 0);
    expect(tp_shr(m, 80).lo == 511 && (tp_shr(m, 32).lo & 0xFFFFFFFFFFFFull) == 0 && static_cast<uint32_t>(m.lo) == 0xFFFFFFFFu, "mask fields");
    int live = 0;
    for (int s = kTpKeyBits - kTpDigitBits; s >= 0; s -= kTpDigitBits) live += tp_digit(m, s) != 0;
    expect(live == 5, "five digits can differ at |N| <= 288, Gamma = 0", live);
    m = tp_bound_mask(0x7FFFFFFFull, (uint64_t(1) << 48) - 1);
    expect(tp_digit(m, 108) == 7 && tp_digit(m, 96) == 4095 && tp_digit(m, 0) == 4095, "the full mask");
    expect(tp_ones_below(0) == 0 && tp_ones_below(1) == 1 && tp_ones_below(4) == 7 && tp_ones_below(7) == 7 && tp_ones_below(8) == 15, "ones below");
    // capacity
    expect(tp_capacity(50, 0) == (1 << 18) && tp_capacity(100000, 0) == 400000 && tp_capacity(1 << 20, -3) == (4 << 20), "capacity");
    expect(tp_capacity(50, 50) == 50 && tp_capacity(50, 7) == 50 && tp_capacity(50, 1000) == 1000 && tp_capacity(50, 1 << 20) == (1 << 18), "REO_TOP_PAIRS_CAP only lowers, never below n");
}

void check_tiles()
{
    for (int G : {1, 2, 63, 64, 65, 300}) {
        std::vector<int> hit(static_cast<size_t>(G) * G, 0);
        const int ctiles = (G + 63) / 64, rtiles = (G + kTpRows - 1) / kTpRows, gx = (ctiles + kTpWaves - 1) / kTpWaves;
        long live_waves = 0, waves = 0;
        for (int by = 0; by < rtiles; ++by)
            for (int bx = 0; bx < gx; ++bx) {
                const int i0 = by * kTpRows;
                for (int wave = 0; wave < kTpWaves; ++wave) {
                    ++waves;
                    const int ctile = bx * kTpWaves + wave;
                    if (!tp_group_live(bx, i0)) { expect(!tp_tile_live(ctile, i0, G), "a dead workgroup has no live wave", bx, by); continue; }
                    if (!tp_tile_live(ctile, i0, G)) continue;
                    ++live_waves;
                    for (int r = 0; r < kTpRows; ++r) {
                        const int i = i0 + r;
                        if (i >= G) break;
                        for (int lane = 0; lane < 64; ++lane) {
                            const int j = ctile * 64 + lane;
                            if (tp_lane_live(i, j, G)) ++hit[static_cast<size_t>(i) * G + j];
                        }
                    }
                }
            }
        bool once = true;
        for (int i = 0; i < G; ++i)
            for (int j = 0; j < G; ++j) once = once && hit[static_cast<size_t>(i) * G + j] == (i < j ? 1 : 0);
        expect(once, "every pair i < j exactly once, nothing else", G);
        printf("tiles %d %ld %ld\n", G, live_waves, waves);
    }
}

void check_pick()
{
    std::vector<uint64_t> bins(kTpHistWords, 0);
    uint64_t above = 99, share = 99;
    expect(tp_pick_digit(bins.data(), 0, 1, &above, &share) == -1 && above == 0 && share == 0, "an empty histogram");
    expect(tp_pick_digit(bins.data(), 7, 8, &above, &share) == -1 && above == 7 && share == 0, "an empty histogram behind seven keys above");
    bins[0] = 10;
    expect(tp_pick_digit(bins.data(), 0, 1, &above, &share) == 0 && above == 0 && share == 10, "the n-th key in the first bin");
    expect(tp_pick_digit(bins.data(), 0, 10, &above, &share) == 0 && above == 0 && share == 10, "the last key of the first bin");
    expect(tp_pick_digit(bins.data(), 0, 11, &above, &share) == -1 && above == 10 && share == 0, "one key too few");
    bins[kTpBins - 1] = 3;
    expect(tp_pick_digit(bins.data(), 0, 3, &above, &share) == kTpBins - 1 && above == 0 && share == 3, "the n-th key in the last bin");
    expect(tp_pick_digit(bins.data(), 0, 4, &above, &share) == 0 && above == 3 && share == 10, "past the last bin");
    expect(tp_pick_digit(bins.data(), 5, 6, &above, &share) == kTpBins - 1 && above == 5 && share == 3, "behind five keys above the prefix");
    bins[2000] = 1;
    expect(tp_pick_digit(bins.data(), 0, 4, &above, &share) == 2000 && above == 3 && share == 1, "a middle bin");
    bins[kTpAbove] = 1000; bins[kTpBelow] = 1000;   // (the extra counters are not bins)
    expect(tp_pick_digit(bins.data(), 0, 14, &above, &share) == 0 && above == 4 && share == 10, "the extra counters are not read");
    expect(tp_pick_digit(bins.data(), 0, 15, &above, &share) == -1 && above == 14, "fewer keys than wanted");
}

void check_select()
{
    // 20 000 keys of G = 200 with five |N| and Gamma that is mostly small: whole bins of equal digits, deep refinement at small capacities
    const int G = 200;
    std::vector<TpKey> keys;
    uint64_t n_max = 0, g_max = 0;
    for (int i = 0; i < G; ++i)
        for (int j = i + 1; j < G; ++j) {
            const uint64_t n = rnd() % 5 * 100, g = rnd() % 4 ? rnd() % 3 : (rnd() >> 20);
            keys.push_back(tp_pack(n, g, i, j, G));
            n_max = n > n_max ? n : n_max; g_max = g > g_max ? g : g_max;
        }
    std::vector<size_t> full(keys.size());
    for (size_t e = 0; e < full.size(); ++e) full[e] = e;
    std::sort(full.begin(), full.end(), [&](size_t x, size_t y) { return tp_before(keys[x], keys[y]); });
    int passes_default = 0;
    for (uint64_t want : {uint64_t(1), uint64_t(50), uint64_t(4000), uint64_t(19900), uint64_t(25000)})
        for (uint64_t cap : {static_cast<uint64_t>(tp_capacity(static_cast<int64_t>(want), 0)), want, want + 3, want * 4}) {
            TpSelect sel;
            const std::vector<size_t> got = select_host(keys, n_max, g_max, want, cap, &sel);
            const size_t n = want < keys.size() ? static_cast<size_t>(want) : keys.size();
            bool same = got.size() == n;
            for (size_t e = 0; same && e < n; ++e) same = got[e] == full[e];
            expect(same, "tp_select + sort is the head of the full sort", static_cast<long>(want), static_cast<long>(cap));
            expect(sel.passes >= 1 && sel.passes <= kTpKeyBits / kTpDigitBits, "passes", sel.passes);
            if (want == 50 && cap > 1000) passes_default = sel.passes;
            if (want == 50 && cap == 50) expect(sel.passes > passes_default, "a tight buffer refines deeper", sel.passes, passes_default);
        }
    // no keys at all, and one key
    std::vector<TpKey> none;
    TpSelect sel;
    expect(select_host(none, 10, 10, 5, 100, &sel).empty() && sel.n_cand == 0 && sel.passes == 1, "no eligible pair");
    std::vector<TpKey> one{tp_pack(3, 4, 0, 1, 2)};
    expect(select_host(one, 3, 4, 5, 5, &sel).size() == 1, "one pair, five wanted");
    // a histogram that contradicts the passes before it is reported
    int calls = 0;
    const auto liar = [&](const TpKey &, int, uint64_t *bins) { bins[kTpAbove] = calls++ ? 5 : 0; bins[1] = 100; return 0; };
    expect(tp_select(liar, tp_bound_mask(n_max, g_max), 10, 10, &sel) == -1, "a pass that contradicts the one before");
    const auto failing = [&](const TpKey &, int, uint64_t *) { return 7; };
    expect(tp_select(failing, tp_bound_mask(n_max, g_max), 10, 10, &sel) == 7, "the histogram's own error is passed on");
}

int select_mode()
{
    long long G, want, cap, n_max, g_max, n_pairs;
    if (scanf("%lld %lld %lld %lld %lld %lld", &G, &want, &cap, &n_max, &g_max, &n_pairs) != 6 || G < 1 || G > kTpMaxGenes || want < 1 || n_pairs < 0) {
        fprintf(stderr, "select: bad header\n");
        return 2;
    }
    std::vector<TpKey> keys;
    std::vector<std::pair<int, int>> pairs;
    for (long long e = 0; e < n_pairs; ++e) {
        long long n, g, i, j;
        if (scanf("%lld %lld %lld %lld", &n, &g, &i, &j) != 4 || i < 0 || i >= j || j >= G || n < 0 || n > n_max || g < 0 || g > g_max) {
            fprintf(stderr, "select: bad pair %lld\n", e);
            return 2;
        }
        keys.push_back(tp_pack(static_cast<uint64_t>(n), static_cast<uint64_t>(g), static_cast<int>(i), static_cast<int>(j), static_cast<int>(G)));
        pairs.emplace_back(static_cast<int>(i), static_cast<int>(j));
    }
    TpSelect sel;
    const std::vector<size_t> got = select_host(keys, static_cast<uint64_t>(n_max), static_cast<uint64_t>(g_max), static_cast<uint64_t>(want),
                                                static_cast<uint64_t>(tp_capacity(want, cap)), &sel);
    printf("passes %d\ncand %llu\n", sel.passes, static_cast<unsigned long long>(sel.n_cand));
    for (size_t e : got) printf("%d %d\n", pairs[e].first, pairs[e].second);
    return g_fail ? 1 : 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "select")) return select_mode();
    check_args();
    check_keys();
    check_tiles();
    check_pick();
    check_select();
    printf("ok %ld\n", g_checks);
    return g_fail ? 1 : 0;
}
