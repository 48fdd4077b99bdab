// Driver of test_filter_maps_under_sanitizers (tests/test_cells_cpu.py): csrc/filter_maps.h -- the counts -> kept flags -> source
// lists step of reo_filter_matrix, its verdicts, and the bit rule for `x > 0` -- on vectors at their exact sizes.  Plain host C++.
//   g++ -std=c++17 -fsanitize=address,undefined -I rankcompv3.jl_amd/csrc -o driver tests/filter_maps_driver.cpp && ./driver
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "filter_maps.h"

static int g_checks = 0, g_bad = 0;
#define CHECK(cond) do { ++g_checks; if (!(cond)) { ++g_bad; std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); } } while (0)

struct Out {
    reo::FilterMaps m;
    std::vector<uint8_t> pk, gk;
};

// counts and masks live in heap blocks of exactly S + G, S and G elements, so that the sanitizer sees a read or write one past them
static Out run(const std::vector<int32_t> &col, const std::vector<int32_t> &gene, int64_t min_profiles, int64_t min_features, bool masks = true)
{
    const int64_t S = static_cast<int64_t>(col.size()), G = static_cast<int64_t>(gene.size());
    std::unique_ptr<int32_t[]> counts(new int32_t[S + G]);
    for (int64_t s = 0; s < S; ++s) counts[s] = col[s];
    for (int64_t g = 0; g < G; ++g) counts[S + g] = gene[g];
    std::unique_ptr<uint8_t[]> pk(new uint8_t[S]), gk(new uint8_t[G]);
    std::memset(pk.get(), 7, S); std::memset(gk.get(), 7, G);
    Out o;
    o.m = reo::filter_maps(counts.get(), S, G, min_profiles, min_features, masks ? pk.get() : nullptr, masks ? gk.get() : nullptr);
    o.pk.assign(pk.get(), pk.get() + S); o.gk.assign(gk.get(), gk.get() + G);
    return o;
}

static std::string str(const std::vector<int32_t> &v) { std::string s; for (int32_t x : v) s += std::to_string(x) + ","; return s; }
static std::string str(const std::vector<uint8_t> &v) { std::string s; for (uint8_t x : v) s += std::to_string(x); return s; }

template <class F, class W>
static W bits_of(F x) { W b; static_assert(sizeof(F) == sizeof(W), "width"); std::memcpy(&b, &x, sizeof(W)); return b; }

int main()
{
    {   // all kept: the identity, no lists
        Out o = run({3, 1, 2}, {1, 1, 5, 9}, 0, 0);
        CHECK(o.m.identity && !o.m.too_small && o.m.S_kept == 3 && o.m.G_kept == 4);
        CHECK(o.m.src_col.empty() && o.m.src_gene.empty());
        CHECK(str(o.pk) == "111" && str(o.gk) == "1111");
        std::printf("all_kept %s %s\n", str(o.pk).c_str(), str(o.gk).c_str());
    }
    {   // none kept
        Out o = run({0, 0, 0}, {0, 0}, 0, 0);
        CHECK(!o.m.identity && o.m.too_small && o.m.S_kept == 0 && o.m.G_kept == 0);
        CHECK(str(o.pk) == "000" && str(o.gk) == "00" && o.m.src_col.empty() && o.m.src_gene.empty());
        std::printf("none_kept %s %s\n", str(o.pk).c_str(), str(o.gk).c_str());
    }
    {   // G' = 1
        Out o = run({4, 4, 4}, {0, 3, 0}, 0, 0);
        CHECK(o.m.too_small && o.m.G_kept == 1 && o.m.S_kept == 3 && str(o.gk) == "010");
        std::printf("one_gene %lld %lld\n", (long long)o.m.G_kept, (long long)o.m.S_kept);
    }
    {   // S' = 1
        Out o = run({0, 2, 0}, {1, 1, 1}, 0, 0);
        CHECK(o.m.too_small && o.m.S_kept == 1 && o.m.G_kept == 3 && str(o.pk) == "010");
        std::printf("one_profile %lld %lld\n", (long long)o.m.G_kept, (long long)o.m.S_kept);
    }
    {   // G' = 2 and S' = 2 are enough
        Out o = run({5, 0, 5}, {2, 0, 2}, 0, 0);
        CHECK(!o.m.too_small && !o.m.identity && str(o.m.src_col) == "0,2," && str(o.m.src_gene) == "0,2,");
    }
    {   // counts equal to the threshold are dropped (strict >), one above stays
        Out o = run({3, 4, 3, 5, 2}, {2, 3, 1, 2, 7}, 3, 2);
        CHECK(str(o.pk) == "01010" && str(o.gk) == "01001");
        CHECK(!o.m.too_small && str(o.m.src_col) == "1,3," && str(o.m.src_gene) == "1,4,");
        std::printf("at_threshold %s %s\n", str(o.pk).c_str(), str(o.gk).c_str());
    }
    {   // first and last element dropped, order preserved
        Out o = run({0, 9, 9, 9, 0}, {0, 1, 2, 3, 0}, 0, 0);
        CHECK(str(o.pk) == "01110" && str(o.gk) == "01110");
        CHECK(str(o.m.src_col) == "1,2,3," && str(o.m.src_gene) == "1,2,3,");
        CHECK(static_cast<int64_t>(o.m.src_col.size()) == o.m.S_kept && static_cast<int64_t>(o.m.src_gene.size()) == o.m.G_kept);
        std::printf("ends_dropped %s %s\n", str(o.m.src_col).c_str(), str(o.m.src_gene).c_str());
    }
    {   // only the first / only the last dropped
        Out a = run({0, 1, 1}, {1, 1, 0}, 0, 0);
        CHECK(str(a.m.src_col) == "1,2," && str(a.m.src_gene) == "0,1,");
    }
    {   // negative thresholds keep zero counts; thresholds beyond int32 keep nothing; null masks are not written
        Out a = run({0, 0}, {0, 0}, -1, -1);
        CHECK(a.m.identity && str(a.pk) == "11");
        Out b = run({2147483647, 2147483647}, {2147483647, 5}, int64_t(1) << 40, 0);
        CHECK(b.m.too_small && b.m.S_kept == 0 && b.m.G_kept == 2);
        Out c = run({1, 0, 1}, {1, 1, 1}, 0, 0, false);
        CHECK(str(c.pk) == "777" && str(c.gk) == "777" && str(c.m.src_col) == "0,2,");
    }
    {   // the minimum shape, and a long vector whose last element alone is dropped
        Out a = run({1, 1}, {1, 1}, 0, 0);
        CHECK(a.m.identity);
        std::vector<int32_t> col(4099, 2), gene(257, 2);
        col.back() = 0; gene.front() = 0;
        Out b = run(col, gene, 1, 1);
        CHECK(b.m.S_kept == 4098 && b.m.G_kept == 256 && b.m.src_col.back() == 4097 && b.m.src_gene.front() == 1);
    }
    {   // `x > 0` on the bits: what the device kernels evaluate
        using reo::positive_bits;
        const double d[] = {1.0, 5e-324, std::numeric_limits<double>::infinity(), 0.0, -0.0, -1.0, -std::numeric_limits<double>::infinity(),
                            std::nan(""), -std::nan(""), 2.2250738585072014e-308, 1e300};
        for (double x : d) CHECK(positive_bits<int64_t>(bits_of<double, int64_t>(x), reo::kPosLimitF64) == (x > 0));
        const float f[] = {1.0f, 1e-45f, std::numeric_limits<float>::infinity(), 0.0f, -0.0f, -1.0f, -std::numeric_limits<float>::infinity(),
                           std::nanf(""), -std::nanf(""), 1.17549435e-38f, 3e38f};
        for (float x : f) CHECK(positive_bits<int32_t>(bits_of<float, int32_t>(x), reo::kPosLimitF32) == (x > 0));
        const int64_t q[] = {1, 0, -1, INT64_MAX, INT64_MIN, int64_t(0x7FF0000000000001LL)};
        for (int64_t x : q) CHECK(positive_bits<int64_t>(x, reo::kPosLimitI64) == (x > 0));
        CHECK(positive_bits<int64_t>(int64_t(0x7FF0000000000001LL), reo::kPosLimitF64) == false);   // a signalling NaN's bits
        CHECK(positive_bits<int32_t>(0x7FC00000, reo::kPosLimitF32) == false);
    }
    if (g_bad) { std::printf("failed %d of %d\n", g_bad, g_checks); return 1; }
    std::printf("ok %d\n", g_checks);
    return 0;
}
