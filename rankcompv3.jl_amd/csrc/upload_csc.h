// Host readers of the CSC upload (reo_set_matrix_csc_*): one run of columns of a sparse genes x samples matrix -- the contiguous entry
// range colptr[c0] .. colptr[c0 + nc] -- checked and narrowed into a staging image of row indices and one of values.  The columns become
// dense on the device (transform.hip, t_csc_columns).  The host pool shares a run out by ENTRIES, so a thread's share begins and ends
// anywhere inside a column; every reader takes the entry range [a, b) of the run and writes image positions [a, b), relative to the run's
// first entry.  The value ladders are those of the dense upload (narrow_columns / narrow_columns_f64 of transform.hip, a value run being
// one "column"): the same conversions and the same "everything fits" verdict for the same values.
// No HIP in here: plain C++17, so that the host-only driver tests/upload_csc_driver.cpp runs it under the sanitizers.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <type_traits>

namespace reo {

// what reo_set_matrix_csc_<type> was handed: colptr [S + 1], rowidx and val [nnz = colptr[S]]
template <class V>
struct CscSrc {
    const int64_t *colptr;
    const int32_t *rowidx;
    const V *val;
    int64_t nnz;
};

enum CscVerdict { kCscOk = 0, kCscRowRange = 1, kCscRowOrder = 2, kCscColptr = 3 };

// colptr[c0 .. c0 + nc] is non-decreasing and stays inside [0, nnz], and no column holds more than G entries (more cannot be strictly
// increasing row indices): what has to hold before the run is cut into pieces and its entries are read.  *at: the offending column.
inline CscVerdict check_colptr_run(const int64_t *colptr, int64_t c0, int64_t nc, int64_t G, int64_t nnz, int64_t *at)
{
    if (colptr[c0] < 0 || colptr[c0] > nnz) { *at = c0; return kCscColptr; }
    for (int64_t k = c0; k < c0 + nc; ++k)
        if (colptr[k + 1] < colptr[k] || colptr[k + 1] > nnz || colptr[k + 1] - colptr[k] > G) { *at = k; return kCscColptr; }
    return kCscOk;
}

// Row indices of entries [a, b) of the run of columns [c0, c0 + nc) (entry q of the run is entry colptr[c0] + q of the matrix): every
// index inside [0, G) and strictly increasing inside its column -- sorted, no duplicates; the first entry of a column is compared with
// nothing, so a descending pair across a column boundary is legal.  The entry in front of a share (a - 1, another thread's) is looked at
// when it lies in the same column.  dst[q] = the index as R (uint16_t when G <= 65 536, else int32_t); a null dst only checks.  The verdict of the first fault.
template <class R>
inline CscVerdict read_rows(const int64_t *colptr, int64_t c0, int64_t nc, const int32_t *rowidx, int64_t G, int64_t a, int64_t b, R *dst)
{
    if (a >= b) return kCscOk;
    const int64_t e0 = colptr[c0];
    // the column of entry a: the last one that begins at or in front of it (empty columns in between begin there too and hold nothing)
    int64_t col = std::upper_bound(colptr + c0, colptr + c0 + nc + 1, e0 + a) - (colptr + c0) - 1 + c0;
    const int32_t *r = rowidx + e0;
    int64_t q = a;
    while (q < b) {
        const int64_t begin = colptr[col] - e0, end = std::min(b, colptr[col + 1] - e0);   // (begin <= q < end)
        int64_t prev = q > begin ? static_cast<int64_t>(r[q - 1]) : -1;
        for (; q < end; ++q) {
            const int64_t v = r[q];
            if (v < 0 || v >= G) return kCscRowRange;
            if (v <= prev) return kCscRowOrder;
            prev = v;
            if (dst) dst[q] = static_cast<R>(v);
        }
        while (q < b && colptr[col + 1] - e0 <= q) ++col;   // the next column that holds entry q
    }
    return kCscOk;
}

// Int64 values [a, b) of a run as N (int16_t / int32_t).  false: some value does not fit N (the run is redone wider)
template <class N>
inline bool narrow_values(const int64_t *val, int64_t a, int64_t b, N *dst)
{
    int64_t bad = 0;
    for (int64_t i = a; i < b; ++i) { const int64_t v = val[i]; const N w = static_cast<N>(v); dst[i] = w; bad |= v ^ static_cast<int64_t>(w); }
    return bad == 0;
}

// Float64 values [a, b) of a run as N (int16_t / int32_t / float): narrowed only if EVERY value converts back to the same bits, so -0.0
// (as an integer), NaN and anything with more mantissa or range than the narrow type keep the run on the wider form
template <class N>
inline bool narrow_values(const double *val, int64_t a, int64_t b, N *dst)
{
    bool ok = true;
    if constexpr (std::is_same<N, float>::value) {
        for (int64_t i = a; i < b; ++i) {
            const double v = val[i];
            // (a finite value beyond Float32's range is not converted: the conversion is undefined there)
            const bool in = !(std::fabs(v) > static_cast<double>(std::numeric_limits<float>::max())) || std::isinf(v);
            const float q = in ? static_cast<float>(v) : 0.0f;
            dst[i] = q;
            ok &= in && static_cast<double>(q) == v;
        }
    } else {
        constexpr double lo = static_cast<double>(std::numeric_limits<N>::min()), hi = static_cast<double>(std::numeric_limits<N>::max());
        for (int64_t i = a; i < b; ++i) {
            const double v = val[i];
            const bool in = v >= lo && v <= hi;            // (false for NaN; the conversion below is undefined outside the range)
            const N q = in ? static_cast<N>(v) : N(0);
            dst[i] = q;
            ok &= in && static_cast<double>(q) == v && !(v == 0.0 && std::signbit(v));
        }
    }
    return ok;
}

}  // namespace reo
