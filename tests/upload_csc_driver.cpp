// Host-only driver for csrc/upload_csc.h (tests/test_csc_cpu.py builds it with -fsanitize=address,undefined and runs it).
// Containers, staging images and value runs are allocated at their exact sizes, so a read or write one element out of place is the
// sanitizer's to report.  A run's row image must equal the row indices themselves and its verdict must be the expected one whatever
// the number of thread shares; the value readers' images are compared with a plain conversion.  Prints one line per verdict and
// "ok <cases> <fnv1a64 digest>".
#include <algorithm>
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "upload_csc.h"

namespace {

uint64_t g_digest = 0xcbf29ce484222325ULL;
long g_cases = 0, g_fail = 0;

void mix(const void *p, size_t n)
{
    const unsigned char *b = static_cast<const unsigned char *>(p);
    for (size_t i = 0; i < n; ++i) { g_digest ^= b[i]; g_digest *= 0x100000001b3ULL; }
}

void fail(const char *what, long a, long b, long c)
{
    if (g_fail++ < 20) fprintf(stderr, "FAIL %s (%ld %ld %ld)\n", what, a, b, c);
}

uint64_t g_rng = 0x9E3779B97F4A7C15ULL;
uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }

struct Csc {
    int64_t G = 0;
    std::vector<int64_t> colptr;   // exact size: S + 1
    std::vector<int32_t> rowidx;   // exact size: nnz
};

// a container of S columns with the given numbers of entries, rows strictly increasing and spread over [0, G)
Csc make(int64_t G, const std::vector<int64_t> &counts)
{
    Csc m;
    m.G = G;
    m.colptr.push_back(0);
    for (int64_t n : counts) {
        // n distinct rows: every (G / n)-th one, shifted; the last column entry reaches row G - 1 when the column is full
        const int64_t step = n ? G / n : 0, off = n && step > 1 ? static_cast<int64_t>(rnd() % static_cast<uint64_t>(step)) : 0;
        for (int64_t k = 0; k < n; ++k) m.rowidx.push_back(static_cast<int32_t>(k * step + off));
        m.colptr.push_back(m.colptr.back() + n);
    }
    return m;
}

// the run of columns [c0, c0 + nc) read in `shares` pieces as the host pool would: the worst verdict, and the image
template <class R>
reo::CscVerdict read_run(const Csc &m, int64_t c0, int64_t nc, int shares, std::vector<R> &image)
{
    const int64_t n = m.colptr[c0 + nc] - m.colptr[c0];
    image.assign(static_cast<size_t>(n), R(0));   // exactly the run's entries
    const int64_t per = (n + shares - 1) / shares;
    int verdict = reo::kCscOk;
    for (int t = 0; t < shares; ++t) {
        const int64_t a = std::min<int64_t>(n, t * per), b = std::min<int64_t>(n, a + per);
        const reo::CscVerdict v = reo::read_rows<R>(m.colptr.data(), c0, nc, m.rowidx.data(), m.G, a, b, image.data());
        if (v != reo::kCscOk && verdict == reo::kCscOk) verdict = v;
    }
    return static_cast<reo::CscVerdict>(verdict);
}

template <class R>
void good_run(const Csc &m, int64_t c0, int64_t nc, const char *what)
{
    const int64_t e0 = m.colptr[c0], n = m.colptr[c0 + nc] - e0;
    for (int shares : {1, 3, 7}) {
        std::vector<R> image;
        ++g_cases;
        if (read_run<R>(m, c0, nc, shares, image) != reo::kCscOk) { fail(what, c0, nc, shares); continue; }
        for (int64_t q = 0; q < n; ++q)
            if (static_cast<int64_t>(image[q]) != m.rowidx[e0 + q]) { fail("row image", c0, q, shares); break; }
        mix(image.data(), image.size() * sizeof(R));
    }
    int64_t at = -1;
    ++g_cases;
    if (reo::check_colptr_run(m.colptr.data(), c0, nc, m.G, m.colptr.back(), &at) != reo::kCscOk) fail("colptr of a good run", c0, nc, at);
}

// a faulty container: every number of shares finds it (the shares that hold the fault, whichever they are)
void verdict_case(const char *name, const Csc &m, reo::CscVerdict want)
{
    const int64_t S = static_cast<int64_t>(m.colptr.size()) - 1;
    for (int shares : {1, 3, 7}) {
        std::vector<int32_t> image;
        const reo::CscVerdict v = read_run<int32_t>(m, 0, S, shares, image);
        ++g_cases;
        if (v != want) fail(name, v, want, shares);
        printf("rows %s %d\n", name, static_cast<int>(v));
        mix(&v, sizeof v);
    }
    if (m.G <= 65536) {
        std::vector<uint16_t> image;
        const reo::CscVerdict v = read_run<uint16_t>(m, 0, S, 3, image);
        ++g_cases;
        if (v != want) fail(name, v, want, 16);
    }
}

template <class V, class N>
void value_case(const char *type, int which, V special)
{
    // the special value at the head, in the middle and at the end of a run of 257 values that all fit, read in 1 and 3 shares
    for (int place = 0; place < 3; ++place) {
        for (int shares : {1, 3}) {
            std::vector<V> val(257);
            for (size_t i = 0; i < val.size(); ++i) val[i] = static_cast<V>(static_cast<int64_t>(rnd() % 200) - 100);
            const size_t at = place == 0 ? 0 : (place == 1 ? 128 : 256);
            val[at] = special;
            std::vector<N> image(val.size());
            bool ok = true;
            const int64_t n = static_cast<int64_t>(val.size()), per = (n + shares - 1) / shares;
            for (int t = 0; t < shares; ++t) {
                const int64_t a = std::min<int64_t>(n, t * per), b = std::min<int64_t>(n, a + per);
                ok &= reo::narrow_values<N>(val.data(), a, b, image.data());
            }
            // the yardstick: the value converts to N and back to the same bits (and is no -0.0 turned into an integer's +0)
            bool want;
            {
                const V v = special;
                N q = N(0);
                bool in = true;
                if constexpr (std::is_floating_point<V>::value && std::is_integral<N>::value)
                    in = v >= static_cast<V>(std::numeric_limits<N>::min()) && v <= static_cast<V>(std::numeric_limits<N>::max());
                if constexpr (std::is_floating_point<V>::value && std::is_same<N, float>::value)
                    in = std::isinf(v) || !(std::fabs(v) > static_cast<V>(std::numeric_limits<float>::max()));
                if constexpr (std::is_integral<V>::value)
                    in = v >= static_cast<V>(std::numeric_limits<N>::min()) && v <= static_cast<V>(std::numeric_limits<N>::max());
                if (in) q = static_cast<N>(v);
                const V back = static_cast<V>(q);
                want = in && v == v && std::memcmp(&back, &v, sizeof v) == 0;   // (NaN equals nothing: never narrowed)
            }
            ++g_cases;
            if (ok != want) fail("value verdict", which, place, shares);
            if (ok)
                for (size_t i = 0; i < val.size(); ++i)
                    if (static_cast<V>(image[i]) != val[i] && !(val[i] != val[i])) { fail("value image", which, static_cast<long>(i), shares); break; }
            if (ok) mix(image.data(), image.size() * sizeof(N));
            printf("%s %d %s\n", type, which, ok ? "fits" : "wider");
            mix(&ok, sizeof ok);
        }
    }
}

}  // namespace

int main()
{
    // ---- good runs: 16- and 32-bit row images, empty and full columns, every way of cutting the entries into shares
    for (int64_t G : {int64_t(2), int64_t(65536), int64_t(65537)}) {
        const int64_t few = std::min<int64_t>(G, 5);
        // an empty first and an empty last column, a full column in the middle, columns of 1 entry, runs of empty columns
        const Csc m = make(G, {0, few, 1, 0, 0, G, 1, few, 0, 2, 0});
        const int64_t S = static_cast<int64_t>(m.colptr.size()) - 1;
        auto both = [&](int64_t c0, int64_t nc, const char *what) {
            if (G <= 65536) good_run<uint16_t>(m, c0, nc, what);
            good_run<int32_t>(m, c0, nc, what);
        };
        both(0, S, "whole matrix");
        both(0, 1, "0 entries");                 // a run without entries
        both(3, 2, "0 entries, two columns");
        both(5, 1, "one full column");
        both(4, 3, "full column between others");
        both(S - 1, 1, "empty last column");
        both(1, S - 2, "inner columns");
    }
    {   // many short columns over many shares
        std::vector<int64_t> counts;
        for (int k = 0; k < 300; ++k) counts.push_back(static_cast<int64_t>(rnd() % 4));
        const Csc m = make(700, counts);
        good_run<uint16_t>(m, 0, 300, "many columns");
        good_run<uint16_t>(m, 37, 200, "many columns, inner run");
    }
    // ---- verdicts
    {
        Csc m = make(10, {3, 4, 2});
        m.rowidx[4] = 10;                                    // a row index equal to G
        verdict_case("index_equal_G", m, reo::kCscRowRange);
        m = make(10, {3, 4, 2});
        m.rowidx[8] = -1;                                    // a negative one
        verdict_case("negative_index", m, reo::kCscRowRange);
        m = make(10, {3, 4, 2});
        m.rowidx[5] = m.rowidx[4];                           // an equal pair inside a column
        verdict_case("equal_pair", m, reo::kCscRowOrder);
        m = make(10, {3, 4, 2});
        std::swap(m.rowidx[5], m.rowidx[6]);                 // a descending pair inside a column
        verdict_case("descending_pair", m, reo::kCscRowOrder);
        m = make(10, {3, 4, 2});
        m.rowidx = {1, 5, 9, 0, 2, 3, 4, 3, 8};              // descending across both column boundaries: legal
        verdict_case("descending_across_columns", m, reo::kCscOk);
        m = make(65537, {2, 2});
        m.rowidx = {0, 65536, 65535, 65536};                 // the last row of a matrix with 32-bit indices
        verdict_case("row_65536_of_65537", m, reo::kCscOk);
        m.rowidx[3] = 65537;
        verdict_case("row_65537_of_65537", m, reo::kCscRowRange);
    }
    {   // colptr runs
        struct { const char *name; std::vector<int64_t> colptr; int64_t G, nnz; int want; } cases[] = {
            {"good", {0, 2, 2, 5}, 4, 5, reo::kCscOk},
            {"decreasing", {0, 3, 2, 5}, 4, 5, reo::kCscColptr},
            {"beyond_nnz", {0, 2, 6, 5}, 4, 5, reo::kCscColptr},
            {"negative_start", {-1, 2, 2, 5}, 4, 5, reo::kCscColptr},
            {"column_longer_than_G", {0, 5, 5, 5}, 4, 5, reo::kCscColptr},
        };
        for (auto &k : cases) {
            int64_t at = -1;
            const int v = reo::check_colptr_run(k.colptr.data(), 0, static_cast<int64_t>(k.colptr.size()) - 1, k.G, k.nnz, &at);
            ++g_cases;
            if (v != k.want) fail(k.name, v, k.want, at);
            printf("colptr %s %d\n", k.name, v);
            mix(&v, sizeof v);
        }
    }
    // ---- the value ladders
    const int64_t i_specials[] = {32767, 32768, -32768, -32769, 2147483647LL, 2147483648LL, -2147483648LL, -2147483649LL, int64_t(1) << 53};
    for (int64_t v : i_specials) { value_case<int64_t, int16_t>("i64", 0, v); value_case<int64_t, int32_t>("i64", 1, v); }
    const double inf = std::numeric_limits<double>::infinity();
    const double f_specials[] = {32767.0, 32768.0, -32768.0, -32769.0, 2147483647.0, 2147483648.0, -2147483648.0, -2147483649.0,
                                 -0.0, std::numeric_limits<double>::quiet_NaN(), inf, -inf, 9007199254740992.0, 0.1, 16777217.0, 0.5, 1e300};
    for (double v : f_specials) { value_case<double, int16_t>("f64", 0, v); value_case<double, int32_t>("f64", 1, v); value_case<double, float>("f64", 2, v); }
    if (g_fail) { fprintf(stderr, "%ld failures\n", g_fail); return 1; }
    printf("ok %ld %016" PRIx64 "\n", g_cases, g_digest);
    return 0;
}
