// Host-only driver for csrc/upload_rows.h (tests/test_rowmajor_cpu.py builds it with -fsanitize=address,undefined and runs it).
// The yardstick is a local copy of the COLUMN readers of csrc/transform.hip (narrow_columns / narrow_columns_f64): for the same
// values the row readers must leave the transposed image and return the same verdict.  Source and staging are allocated at their
// exact sizes, so a read or write one element out of place is the sanitizer's to report.  Prints "ok <cases> <fnv1a64 digest>".
#include <algorithm>
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <type_traits>
#include <vector>

#include "upload_rows.h"

namespace {

// ---- the column readers, as transform.hip has them ----
template <class N>
bool narrow_columns(const int64_t *src, int64_t ld, int64_t G, int col0, int col1, N *dst)
{
    int64_t bad = 0;
    for (int cidx = col0; cidx < col1 && !bad; ++cidx) {
        const int64_t *s = src + static_cast<int64_t>(cidx) * ld;
        N *d = dst + static_cast<int64_t>(cidx) * G;
        for (int64_t i = 0; i < G; ++i) { const int64_t v = s[i]; const N w = static_cast<N>(v); d[i] = w; bad |= v ^ static_cast<int64_t>(w); }
    }
    return bad == 0;
}

template <class N>
bool narrow_columns_f64(const double *src, int64_t ld, int64_t G, int col0, int col1, N *dst)
{
    bool ok = true;
    for (int cidx = col0; cidx < col1 && ok; ++cidx) {
        const double *s = src + static_cast<int64_t>(cidx) * ld;
        N *d = dst + static_cast<int64_t>(cidx) * G;
        if constexpr (std::is_same<N, float>::value) {
            for (int64_t i = 0; i < G; ++i) { const double v = s[i]; const float q = static_cast<float>(v); d[i] = q; ok &= static_cast<double>(q) == v; }
        } else {
            constexpr double lo = static_cast<double>(std::numeric_limits<N>::min()), hi = static_cast<double>(std::numeric_limits<N>::max());
            for (int64_t i = 0; i < G; ++i) {
                const double v = s[i];
                const bool in = v >= lo && v <= hi;
                const N q = in ? static_cast<N>(v) : N(0);
                d[i] = q;
                ok &= in && static_cast<double>(q) == v && !(v == 0.0 && std::signbit(v));
            }
        }
    }
    return ok;
}

uint64_t g_digest = 0xcbf29ce484222325ULL;
long g_cases = 0, g_fail = 0;

void mix(const void *p, size_t n)
{
    const unsigned char *b = static_cast<const unsigned char *>(p);
    for (size_t i = 0; i < n; ++i) { g_digest ^= b[i]; g_digest *= 0x100000001b3ULL; }
}

void fail(const char *what, long a, long b, long c, long d)
{
    if (g_fail++ < 20) fprintf(stderr, "FAIL %s (%ld %ld %ld %ld)\n", what, a, b, c, d);
}

template <class S> bool read_rows_as(int which, const S *src, int64_t ld, int64_t r0, int64_t r1, int64_t c0, int nc, void *dst);
template <> bool read_rows_as<int64_t>(int which, const int64_t *src, int64_t ld, int64_t r0, int64_t r1, int64_t c0, int nc, void *dst)
{
    return which == 0 ? reo::narrow_rows<int16_t>(src, ld, r0, r1, c0, nc, static_cast<int16_t *>(dst))
                      : reo::narrow_rows<int32_t>(src, ld, r0, r1, c0, nc, static_cast<int32_t *>(dst));
}
template <> bool read_rows_as<double>(int which, const double *src, int64_t ld, int64_t r0, int64_t r1, int64_t c0, int nc, void *dst)
{
    return which == 0 ? reo::narrow_rows_f64<int16_t>(src, ld, r0, r1, c0, nc, static_cast<int16_t *>(dst))
         : which == 1 ? reo::narrow_rows_f64<int32_t>(src, ld, r0, r1, c0, nc, static_cast<int32_t *>(dst))
                      : reo::narrow_rows_f64<float>(src, ld, r0, r1, c0, nc, static_cast<float *>(dst));
}
template <class S> bool read_cols_as(int which, const S *src, int64_t ld, int64_t G, int nc, void *dst);
template <> bool read_cols_as<int64_t>(int which, const int64_t *src, int64_t ld, int64_t G, int nc, void *dst)
{
    return which == 0 ? narrow_columns<int16_t>(src, ld, G, 0, nc, static_cast<int16_t *>(dst)) : narrow_columns<int32_t>(src, ld, G, 0, nc, static_cast<int32_t *>(dst));
}
template <> bool read_cols_as<double>(int which, const double *src, int64_t ld, int64_t G, int nc, void *dst)
{
    return which == 0 ? narrow_columns_f64<int16_t>(src, ld, G, 0, nc, static_cast<int16_t *>(dst))
         : which == 1 ? narrow_columns_f64<int32_t>(src, ld, G, 0, nc, static_cast<int32_t *>(dst))
                      : narrow_columns_f64<float>(src, ld, G, 0, nc, static_cast<float *>(dst));
}

// One case: the row-major source rm (G x S, pitch ld), its chunk [c0, c0 + nc) read by `threads` row shares, against the column
// reader on the column-major copy of the same chunk.  The images are compared only when everything fits (a reader that meets a value
// that does not fit stops where it is: the chunk is redone wider).  Returns the verdict.
template <class S>
bool one_case(int which, const std::vector<S> &rm, int64_t G, int64_t Sn, int64_t ld, int64_t c0, int nc, int threads)
{
    const size_t width = which == 0 ? 2 : 4;
    const size_t nel = static_cast<size_t>(G) * nc;
    std::vector<S> cm(nel);                                   // the chunk, column-major, ld = G: what the column reader is given
    for (int64_t g = 0; g < G; ++g)
        for (int j = 0; j < nc; ++j) cm[static_cast<size_t>(j) * G + g] = rm[static_cast<size_t>(g * ld + c0 + j)];
    std::vector<unsigned char> img_c(nel * width), img_r(nel * width, 0xAB);
    const bool ok_c = read_cols_as<S>(which, cm.data(), G, G, nc, img_c.data());
    bool ok_r = true;
    const int64_t rper = (G + threads - 1) / threads;
    for (int t = 0; t < threads; ++t) {                       // the split of the host pool (transform.hip): by gene rows
        const int64_t a = std::min<int64_t>(G, t * rper), b = std::min<int64_t>(G, a + rper);
        if (a < b) ok_r &= read_rows_as<S>(which, rm.data(), ld, a, b, c0, nc, img_r.data());
    }
    ++g_cases;
    if (ok_c != ok_r) fail("verdict", which, G, c0, nc);
    if (ok_c && ok_r) {
        for (int64_t g = 0; g < G; ++g)
            for (int j = 0; j < nc; ++j)
                if (memcmp(&img_r[(static_cast<size_t>(g) * nc + j) * width], &img_c[(static_cast<size_t>(j) * G + g) * width], width) != 0) { fail("image", which, G, c0 + j, g); g = G; break; }
        mix(img_r.data(), img_r.size());
    }
    const unsigned char v = ok_r ? 1 : 0;
    mix(&v, 1);
    (void)Sn;
    return ok_r;
}

template <class S>
void sweep(int nforms)
{
    const int64_t Sn = 101, ld = Sn + 7;
    for (int64_t G : {1, 2, 63, 257}) {
        std::vector<S> rm(static_cast<size_t>((G - 1) * ld + Sn));   // exactly: the last row has no pitch behind it
        uint64_t ctr = 0x9E3779B97F4A7C15ULL;
        for (auto &v : rm) { ctr = ctr * 6364136223846793005ULL + 1442695040888963407ULL; v = static_cast<S>(static_cast<int64_t>(ctr >> 50) - 8192); }   // fits 16 bits
        for (int nc : {1, 37, 64})
            for (int64_t c0 : {int64_t(0), Sn - nc})                 // both ends of the row
                for (int threads : {1, 3, 7})
                    for (int which = 0; which < nforms; ++which)
                        if (!one_case<S>(which, rm, G, Sn, ld, c0, nc, threads)) fail("sweep value did not fit", which, G, c0, nc);
        // pack_rows and the probe's gather on the same source
        for (int nc : {1, 37, 64}) {
            const int64_t c0 = Sn - nc;
            std::vector<S> img(static_cast<size_t>(G) * nc);
            for (int t = 0; t < 3; ++t) {
                const int64_t rper = (G + 2) / 3, a = std::min<int64_t>(G, t * rper), b = std::min<int64_t>(G, a + rper);
                if (a < b) reo::pack_rows(rm.data(), ld, a, b, c0, nc, img.data());
            }
            for (int64_t g = 0; g < G; ++g)
                for (int j = 0; j < nc; ++j) if (memcmp(&img[static_cast<size_t>(g) * nc + j], &rm[static_cast<size_t>(g * ld + c0 + j)], sizeof(S)) != 0) fail("pack", G, nc, g, j);
            std::vector<S> head(static_cast<size_t>(G));
            reo::gather_column_head(rm.data(), ld, c0, G, head.data());
            for (int64_t g = 0; g < G; ++g) if (memcmp(&head[static_cast<size_t>(g)], &rm[static_cast<size_t>(g * ld + c0)], sizeof(S)) != 0) fail("gather", G, nc, g, 0);
            mix(img.data(), img.size() * sizeof(S));
            ++g_cases;
        }
    }
}

// one special value at one place of a small matrix of zeros..5: the verdicts of all forms, both readers
template <class S>
void verdicts(const std::vector<S> &specials, int nforms)
{
    const int64_t G = 5, Sn = 9, ld = 12;
    for (const S sp : specials)
        for (int64_t at : {int64_t(0), int64_t(2 * ld + 4), (G - 1) * ld + Sn - 1}) {
            std::vector<S> rm(static_cast<size_t>((G - 1) * ld + Sn));
            for (size_t i = 0; i < rm.size(); ++i) rm[i] = static_cast<S>(static_cast<int64_t>(i % 6));
            rm[static_cast<size_t>(at)] = sp;
            for (int which = 0; which < nforms; ++which)
                for (int threads : {1, 3}) {
                    const bool ok = one_case<S>(which, rm, G, Sn, ld, 0, static_cast<int>(Sn), threads);
                    printf("%s %d %s\n", std::is_same<S, double>::value ? "f64" : "i64", which, ok ? "fits" : "wider");
                }
        }
}

}  // namespace

int main()
{
    sweep<int64_t>(2);
    sweep<double>(3);
    verdicts<int64_t>({32767, 32768, -32768, -32769, 2147483647LL, 2147483648LL, -2147483648LL, -2147483649LL, int64_t(1) << 53}, 2);
    const double inf = std::numeric_limits<double>::infinity();
    verdicts<double>({32767.0, 32768.0, -32768.0, -32769.0, 2147483647.0, 2147483648.0, -2147483648.0, -2147483649.0, -0.0,
                      std::numeric_limits<double>::quiet_NaN(), inf, -inf, 9007199254740992.0 /* 2^53 */, 0.1 /* more mantissa than float32 holds */,
                      16777217.0 /* 2^24 + 1: an integer that float32 does not hold */, 0.5},
                     3);
    if (g_fail) { fprintf(stderr, "%ld failures\n", g_fail); return 1; }
    printf("ok %ld %016" PRIx64 "\n", g_cases, g_digest);
    return 0;
}
