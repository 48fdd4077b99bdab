// Row readers of the upload: one chunk of sample columns of a ROW-MAJOR host matrix (genes x samples, pitch ld >= S) into a staging
// image.  A chunk of nc columns of such a matrix is G contiguous row segments of nc elements; the readers take them as they are and
// leave the image row-major and packed, [G][nc] -- the transposition into the resident column-major matrix happens on the device
// (transform.hip, t_widen_transpose).  Counterparts of narrow_columns / narrow_columns_f64 of transform.hip: the same conversions and
// the same "everything fits" verdict for the same values, so the form ladder of a chunk does not depend on the layout it arrived in.
// No HIP in here: plain C++17, so that the host-only driver tests/upload_rows_driver.cpp runs it under the sanitizers.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <type_traits>

namespace reo {

// gene rows [r0, r1), columns [c0, c0 + nc) of an Int64 source as N (int16_t / int32_t); dst is the WHOLE chunk's image (row r lands
// at dst + r * nc): the host pool splits a chunk by gene rows, so every thread writes one contiguous piece of it.
// false: some value does not fit N (a row that does not fit ends this thread's share: the chunk is redone wider)
template <class N>
inline bool narrow_rows(const int64_t *src, int64_t ld, int64_t r0, int64_t r1, int64_t c0, int nc, N *dst)
{
    int64_t bad = 0;
    for (int64_t r = r0; r < r1 && !bad; ++r) {
        const int64_t *s = src + r * ld + c0;
        N *d = dst + r * static_cast<int64_t>(nc);
        for (int i = 0; i < nc; ++i) { const int64_t v = s[i]; const N w = static_cast<N>(v); d[i] = w; bad |= v ^ static_cast<int64_t>(w); }
    }
    return bad == 0;
}

// the same for a Float64 source as N (int16_t / int32_t / float): a chunk is narrowed only if EVERY value converts back to the same
// bits, so -0.0, NaN and anything with more mantissa (or range) than the narrow type keep it on the wider form
template <class N>
inline bool narrow_rows_f64(const double *src, int64_t ld, int64_t r0, int64_t r1, int64_t c0, int nc, N *dst)
{
    bool ok = true;
    for (int64_t r = r0; r < r1 && ok; ++r) {
        const double *s = src + r * ld + c0;
        N *d = dst + r * static_cast<int64_t>(nc);
        if constexpr (std::is_same<N, float>::value) {
            for (int i = 0; i < nc; ++i) { const double v = s[i]; const float q = static_cast<float>(v); d[i] = q; ok &= static_cast<double>(q) == v; }
        } else {
            constexpr double lo = static_cast<double>(std::numeric_limits<N>::min()), hi = static_cast<double>(std::numeric_limits<N>::max());
            for (int i = 0; i < nc; ++i) {
                const double v = s[i];
                const bool in = v >= lo && v <= hi;            // (false for NaN; the conversion below is undefined outside the range)
                const N q = in ? static_cast<N>(v) : N(0);
                d[i] = q;
                ok &= in && static_cast<double>(q) == v && !(v == 0.0 && std::signbit(v));
            }
        }
    }
    return ok;
}

// the same rows as they are (the RAW form of a chunk, and every chunk of a 32-bit host type): row segments packed into the image
template <class E>
inline void pack_rows(const E *src, int64_t ld, int64_t r0, int64_t r1, int64_t c0, int nc, E *dst)
{
    for (int64_t r = r0; r < r1; ++r)
        std::memcpy(dst + r * static_cast<int64_t>(nc), src + r * ld + c0, static_cast<size_t>(nc) * sizeof(E));
}

// the head of one column (rows [0, n) of column c0) as a dense vector: what the form probe of a chunk looks at, in either layout
template <class E>
inline void gather_column_head(const E *src, int64_t ld, int64_t c0, int64_t n, E *dst)
{
    for (int64_t r = 0; r < n; ++r) dst[r] = src[r * ld + c0];
}

}  // namespace reo
