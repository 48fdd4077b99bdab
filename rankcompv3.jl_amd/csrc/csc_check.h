// The checks of a CSC container whose arrays live on the device (reo_set_matrix_csc_dev_*, reo_set_matrix_pseudobulk_csc_dev_*): what the host
// readers of upload_csc.h decide for a host container, stated per column and per entry so that a kernel can evaluate them with one
// workgroup per column (csc_device.hip, csc_validate) -- and a host driver can evaluate the very same functions under the sanitizers
// (tests/csc_check_driver.cpp).  I is the type of BOTH index arrays, int32_t or int64_t.
// The order of the checks is the contract: a column's two colptr words are checked first, and only when they describe a range inside
// [0, nnz] of at most G entries is any row index of that column read; a row index is only ever compared, no address is formed from it.
// No HIP header in here: plain C++17 (the kernel's unit defines the function attributes).
#pragma once

#include <cstdint>

#include "upload_csc.h"

#if defined(__HIPCC__)
#define REO_CSC_FN __host__ __device__ inline
#else
#define REO_CSC_FN inline
#endif

namespace reo {

// The verdict of a whole container is ONE 64-bit word, the minimum over everything that was found:
//   bit 63      0 for a colptr fault, 1 for a row fault -- a colptr fault anywhere wins, as check_colptr_run runs in front of read_rows
//   bits 22-62  the column
//   bits 2-21   the entry's place inside its column (0 for a colptr fault; a checked column has at most G <= 2^18 entries)
//   bits 0-1    the CscVerdict
// so the minimum names the lowest offending column, and inside it the first offending entry with the class read_rows gives it.
constexpr uint64_t kCscClean = ~0ULL;

REO_CSC_FN uint64_t csc_pack(CscVerdict v, int64_t column, int64_t place)
{
    return (v == kCscColptr ? 0ULL : 1ULL << 63) | (static_cast<uint64_t>(column) << 22) | (static_cast<uint64_t>(place) << 2) | static_cast<uint64_t>(v);
}
REO_CSC_FN CscVerdict csc_class(uint64_t word) { return word == kCscClean ? kCscOk : static_cast<CscVerdict>(word & 3ULL); }
REO_CSC_FN int64_t csc_column(uint64_t word) { return static_cast<int64_t>((word & ~(1ULL << 63)) >> 22); }

// Column k of S: colptr[k] and colptr[k + 1] lie in [0, nnz], do not decrease and are at most G apart; the first column begins at 0 and
// the last one ends at nnz.  Reads colptr[k] and colptr[k + 1], nothing else.  On kCscOk [*a, *b) are the column's entries.
template <class I>
REO_CSC_FN CscVerdict csc_check_column(const I *colptr, int64_t k, int64_t S, int64_t G, int64_t nnz, int64_t *a, int64_t *b)
{
    const int64_t lo = static_cast<int64_t>(colptr[k]), hi = static_cast<int64_t>(colptr[k + 1]);
    *a = lo; *b = hi;
    if (lo < 0 || lo > nnz || hi < 0 || hi > nnz || hi < lo || hi - lo > G) return kCscColptr;
    if ((k == 0 && lo != 0) || (k == S - 1 && hi != nnz)) return kCscColptr;
    return kCscOk;
}

// Entry q of a checked column [a, b): its row index is inside [0, G), and above the row index in front of it when that belongs to the
// same column.  Reads rows[q] and, for q > a, rows[q - 1].  Range before order, as read_rows decides for the first faulty entry.
template <class I>
REO_CSC_FN CscVerdict csc_check_entry(const I *rows, int64_t q, int64_t a, int64_t G)
{
    const int64_t v = static_cast<int64_t>(rows[q]);
    if (v < 0 || v >= G) return kCscRowRange;
    if (q > a && static_cast<int64_t>(rows[q - 1]) >= v) return kCscRowOrder;
    return kCscOk;
}

// One column as a `stride` of workers sees it, worker `lane` of them: the word of the first fault this worker meets (kCscClean: none).
// The kernel calls it with (threadIdx.x, blockDim.x), the host driver with every lane in turn.
template <class I>
REO_CSC_FN uint64_t csc_check_share(const I *colptr, const I *rows, int64_t k, int64_t S, int64_t G, int64_t nnz, int lane, int stride)
{
    int64_t a, b;
    if (csc_check_column(colptr, k, S, G, nnz, &a, &b) != kCscOk) return csc_pack(kCscColptr, k, 0);
    for (int64_t q = a + lane; q < b; q += stride) {   // (consecutive workers, consecutive entries)
        const CscVerdict v = csc_check_entry(rows, q, a, G);
        if (v != kCscOk) return csc_pack(v, k, q - a);
    }
    return kCscClean;
}

}  // namespace reo
