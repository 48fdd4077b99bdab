// Host driver of csrc/contrast.h for the CPU tests (tests/test_contrasts_cpu.py): compiled stand-alone with AddressSanitizer and UBSan.
// Every argument check of reo_build_pairs_contrast with its message, and the derived sides -- blocks, sizes, thresholds -- for interleaved
// labels, groups of 1, 31, 32 and 33 samples and 70 groups, against sums made here from the labels.  Prints one line per failed check's
// message ("msg <number> <text>"), one line per derived case and "ok <checks>" at the end; any mismatch: a message on stderr and exit 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "contrast.h"

using namespace reo;

static long g_checks = 0;

#define EXPECT(cond)                                                              \
    do {                                                                          \
        ++g_checks;                                                               \
        if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); exit(1); } \
    } while (0)

static ContrastState good_state(int32_t ngroups)
{
    ContrastState st{};
    st.ngroups = ngroups; st.thr_set = true; st.multi_device = false; st.S = 100; st.share_counts = true; st.planes_fit = true;
    st.planes_bytes = 123456789012ll;
    return st;
}

static void refusal(int want, bool have_ctx, const ContrastState &st, int32_t ctrl, int32_t treat, const char *needle)
{
    char msg[320];
    memset(msg, 0x7f, sizeof msg);
    const int got = contrast_check_args(have_ctx, st, ctrl, treat, msg, sizeof msg);
    EXPECT(got == want);
    EXPECT(strlen(msg) < sizeof msg);
    EXPECT(strncmp(msg, "reo_build_pairs_contrast: ", 26) == 0);   // every message names the function
    EXPECT(strstr(msg, needle) != nullptr);
    printf("msg %d %s\n", got, msg);
    // a short buffer is never overrun (the sanitizer watches the bytes behind it)
    std::vector<char> tiny(8, 0x7f);
    EXPECT(contrast_check_args(have_ctx, st, ctrl, treat, tiny.data(), tiny.size()) == want);
    EXPECT(strlen(tiny.data()) == 7);
}

static void check_refusals()
{
    ContrastState st = good_state(3);
    char msg[320] = "untouched";
    EXPECT(contrast_check_args(true, st, 0, 1, msg, sizeof msg) == 0);
    EXPECT(contrast_check_args(true, st, 2, 0, msg, sizeof msg) == 0);
    EXPECT(strcmp(msg, "untouched") == 0);
    refusal(1, false, ContrastState{}, 0, 1, "null context");
    refusal(2, true, st, -1, 1, "ctrl = -1 is outside [0, 3)");
    refusal(2, true, st, 3, 1, "ctrl = 3 is outside [0, 3)");
    refusal(3, true, st, 0, 3, "treat = 3 is outside [0, 3)");
    refusal(3, true, st, 0, -7, "treat = -7 is outside [0, 3)");
    refusal(4, true, st, 2, 2, "ctrl = treat = 2");
    ContrastState nogroups = good_state(0);
    refusal(2, true, nogroups, 0, 1, "outside [0, 0)");
    ContrastState t = st; t.thr_set = false;
    refusal(5, true, t, 0, 1, "thresholds not set");
    t = st; t.multi_device = true;
    refusal(6, true, t, 0, 1, "reo_create_multi");
    t = st; t.S = 65600;
    refusal(7, true, t, 0, 1, "more than 65535 samples (65600");
    t.S = 65535;
    EXPECT(contrast_check_args(true, t, 0, 1, msg, sizeof msg) == 0);
    t = st; t.share_counts = false;
    refusal(8, true, t, 0, 1, "REO_SHARE_GROUP_COUNTS=0");
    t = st; t.planes_fit = false;
    refusal(9, true, t, 0, 1, "do not fit the free device memory (123456789012 bytes needed for 3 groups)");
    // the order of the checks: the arguments before the state, the state before the planes
    t = st; t.thr_set = false; t.multi_device = true; t.S = 70000; t.share_counts = false; t.planes_fit = false;
    EXPECT(contrast_check_args(true, t, 5, 5, msg, sizeof msg) == 2);
    EXPECT(contrast_check_args(true, t, 1, 5, msg, sizeof msg) == 3);
    EXPECT(contrast_check_args(true, t, 1, 1, msg, sizeof msg) == 4);
    EXPECT(contrast_check_args(true, t, 1, 0, msg, sizeof msg) == 5);
    t.thr_set = true;
    EXPECT(contrast_check_args(true, t, 1, 0, msg, sizeof msg) == 6);
    t.multi_device = false;
    EXPECT(contrast_check_args(true, t, 1, 0, msg, sizeof msg) == 7);
    t.S = 10;
    EXPECT(contrast_check_args(true, t, 1, 0, msg, sizeof msg) == 8);
    t.share_counts = true;
    EXPECT(contrast_check_args(true, t, 1, 0, msg, sizeof msg) == 9);
    // two groups need no planes: whatever their state, the call is a reo_build_pairs
    ContrastState two = good_state(2);
    two.S = 70000; two.share_counts = false; two.planes_fit = false;
    EXPECT(contrast_check_args(true, two, 0, 1, msg, sizeof msg) == 0);
    EXPECT(contrast_check_args(true, two, 1, 0, msg, sizeof msg) == 0);
    EXPECT(contrast_check_args(true, two, 1, 1, msg, sizeof msg) == 4);
    two.multi_device = true;
    EXPECT(contrast_check_args(true, two, 0, 1, msg, sizeof msg) == 6);
}

// The offsets a context derives from labels (the groups contiguous in label order, each padded to whole blocks of 32 slots), and a
// threshold matrix whose entries name their place: row 0 of group g = 1000 + g, row 1 = 2000 + g.
struct Groups {
    std::vector<int32_t> goff, goff32, thr;
};

static Groups groups_of(const std::vector<int32_t> &label, int ngroups)
{
    Groups g;
    std::vector<int32_t> cnt(ngroups, 0);
    for (int32_t l : label) cnt[l]++;
    g.goff.assign(ngroups + 1, 0);
    g.goff32.assign(ngroups + 1, 0);
    for (int k = 0; k < ngroups; ++k) {
        g.goff[k + 1] = g.goff[k] + cnt[k];
        g.goff32[k + 1] = g.goff32[k] + (cnt[k] + 31) / 32 * 32;
    }
    g.thr.assign(2 * ngroups, 0);
    for (int k = 0; k < ngroups; ++k) { g.thr[2 * k] = 1000 + k; g.thr[2 * k + 1] = 2000 + k; }
    return g;
}

static void check_sides(const char *name, const std::vector<int32_t> &label, int ngroups)
{
    const Groups g = groups_of(label, ngroups);
    std::vector<int32_t> cnt(ngroups, 0);
    for (int32_t l : label) cnt[l]++;
    long blocks = 0;
    for (int a = 0; a < ngroups; ++a)
        for (int b = 0; b < ngroups; ++b) {
            if (a == b) continue;
            const ContrastSides s = contrast_sides(g.goff.data(), g.goff32.data(), g.thr.data(), a, b);
            EXPECT(s.nc == cnt[a] && s.nt == cnt[b]);
            EXPECT(s.m1 == 1000 + a && s.m2 == 1000 + b);          // row 0 of each group's own column, never row 1
            EXPECT(s.ce - s.cb == (cnt[a] + 31) / 32 && s.te - s.tb == (cnt[b] + 31) / 32);
            int cb = 0, tb = 0;
            for (int k = 0; k < a; ++k) cb += (cnt[k] + 31) / 32;
            for (int k = 0; k < b; ++k) tb += (cnt[k] + 31) / 32;
            EXPECT(s.cb == cb && s.tb == tb);
            EXPECT(s.ce <= g.goff32[ngroups] / 32 && s.te <= g.goff32[ngroups] / 32);
            EXPECT(s.ce <= s.tb || s.te <= s.cb);                  // the two sides never share a block
            // the mirrored contrast swaps the sides
            const ContrastSides m = contrast_sides(g.goff.data(), g.goff32.data(), g.thr.data(), b, a);
            EXPECT(m.cb == s.tb && m.ce == s.te && m.tb == s.cb && m.te == s.ce && m.nc == s.nt && m.nt == s.nc && m.m1 == s.m2 && m.m2 == s.m1);
            blocks += (s.ce - s.cb) + (s.te - s.tb);
        }
    printf("sides %s %d %zu %ld\n", name, ngroups, label.size(), blocks);
}

int main()
{
    check_refusals();
    {   // interleaved labels: 0 1 2 0 1 2 ... plus a tail of group 1
        std::vector<int32_t> l;
        for (int s = 0; s < 40; ++s) l.push_back(s % 3);
        for (int s = 0; s < 5; ++s) l.push_back(1);
        check_sides("interleaved", l, 3);
    }
    {   // groups of 1, 31, 32 and 33 samples, interleaved
        std::vector<int32_t> l;
        const int n[4] = {1, 31, 32, 33};
        for (int s = 0; s < 33; ++s)
            for (int k = 3; k >= 0; --k)
                if (s < n[k]) l.push_back(k);
        check_sides("block_edges", l, 4);
        const Groups g = groups_of(l, 4);
        const ContrastSides s = contrast_sides(g.goff.data(), g.goff32.data(), g.thr.data(), 3, 0);
        EXPECT(s.cb == 3 && s.ce == 5 && s.tb == 0 && s.te == 1 && s.nc == 33 && s.nt == 1);
        const ContrastSides u = contrast_sides(g.goff.data(), g.goff32.data(), g.thr.data(), 1, 2);
        EXPECT(u.cb == 1 && u.ce == 2 && u.tb == 2 && u.te == 3 && u.nc == 31 && u.nt == 32);
    }
    {   // 70 groups of 1 .. 70 samples
        std::vector<int32_t> l;
        for (int k = 0; k < 70; ++k)
            for (int s = 0; s <= k; ++s) l.push_back(k);
        check_sides("seventy", l, 70);
        ContrastState st = good_state(70);
        char msg[320];
        EXPECT(contrast_check_args(true, st, 69, 0, msg, sizeof msg) == 0);
        EXPECT(contrast_check_args(true, st, 70, 0, msg, sizeof msg) == 2);
    }
    printf("ok %ld\n", g_checks);
    return 0;
}
