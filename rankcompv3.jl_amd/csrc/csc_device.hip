// Sparse matrices that already live on the device (include/reo_hip.h, SPARSE ON THE DEVICE): the check of the caller's index arrays.
// The host entries let host threads read every colptr word and every row index before a kernel sees them (upload_csc.h); here the arrays
// are in HBM, so the same decisions are taken by a kernel -- one launch, one stream over nnz x index bytes -- and NOTHING that indexes
// with them (t_csc_columns searches and scatters by the row indices, pb_csc uses them as LDS addresses) is queued before the verdict
// has come back to the host.  The predicates are those of csc_check.h, shared with the host driver of the CPU tests.
#include <algorithm>
#include <cstdint>

#include "reo_internal.h"
#include "csc_check.h"

namespace reo {

namespace {

// One workgroup per column (striding the columns when there are more than the grid holds); its threads stride the column's entries, so
// a wave reads consecutive indices.  The verdict word (csc_check.h) is the minimum over every fault found: per wave one shuffle
// reduction, then one 64-bit atomic minimum from the waves that found something -- a clean container issues no atomic at all.
template <class I>
__global__ __launch_bounds__(256) void csc_validate(const I *__restrict__ colptr, const I *__restrict__ rows, int64_t S, int64_t G, int64_t nnz,
                                                    unsigned long long *__restrict__ verdict)
{
    unsigned long long worst = kCscClean;
    for (int64_t k = blockIdx.x; k < S; k += gridDim.x) {
        const unsigned long long w = csc_check_share<I>(colptr, rows, k, S, G, nnz, static_cast<int>(threadIdx.x), 256);
        worst = w < worst ? w : worst;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long b = __shfl_xor(worst, o, 64); worst = b < worst ? b : worst; }
    if ((threadIdx.x & 63) == 0 && worst != kCscClean) atomicMin(verdict, worst);
}

// a 32-bit column pointer as the 64-bit one the consuming kernels read (S + 1 values)
__global__ __launch_bounds__(256) void csc_widen_colptr(const int32_t *__restrict__ src, int64_t *__restrict__ dst, int64_t n)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

}  // namespace

// Arguments and container of a device CSC matrix of S columns.  REO_OK: every colptr word and row index has been checked, the context's
// stream is idle, and *colptr64 is the column pointer as int64 on the device -- the caller's own array, or c->csc_colptr for 32-bit
// indices.  REO_EINVAL names the fault and, for a fault of the container, the lowest offending column.
int32_t csc_device_check(reo_ctx *c, int64_t G, int64_t S, int64_t nnz, const void *d_colptr, const void *d_rowidx, int32_t index_bits,
                         const void *d_val, const int64_t **colptr64)
{
    if (index_bits != 32 && index_bits != 64) { set_error("index_bits is %d: the index arrays are int32 (32) or int64 (64)", index_bits); return REO_EINVAL; }
    if (!d_colptr) { set_error("colptr is null"); return REO_EINVAL; }
    if (nnz < 0 || nnz > G * S || (index_bits == 32 && nnz > INT32_MAX)) {
        set_error("nnz = %lld is not a number of entries of a %lld x %lld matrix with %d-bit indices", (long long)nnz, (long long)G, (long long)S, index_bits);
        return REO_EINVAL;
    }
    if (nnz > 0 && (!d_rowidx || !d_val)) { set_error("%s is null with nnz = %lld entries", !d_rowidx ? "rowidx" : "val", (long long)nnz); return REO_EINVAL; }
    DevBuf<unsigned long long> word;
    int32_t rc = word.ensure(1);
    if (rc) return rc;
    const unsigned grid = static_cast<unsigned>(std::min<int64_t>(S, int64_t(1) << 20));
    unsigned long long verdict = 0;
    hipError_t e = hipMemsetAsync(word.p, 0xFF, sizeof(unsigned long long), c->stream);   // kCscClean
    if (e == hipSuccess) {
        if (index_bits == 32) csc_validate<int32_t><<<grid, 256, 0, c->stream>>>(static_cast<const int32_t *>(d_colptr), static_cast<const int32_t *>(d_rowidx), S, G, nnz, word.p);
        else csc_validate<int64_t><<<grid, 256, 0, c->stream>>>(static_cast<const int64_t *>(d_colptr), static_cast<const int64_t *>(d_rowidx), S, G, nnz, word.p);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&verdict, word.p, sizeof verdict, hipMemcpyDeviceToHost, c->stream);
    const hipError_t es = hipStreamSynchronize(c->stream);   // (on every path: nothing of this call is in flight when `word` goes)
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) { set_error("checking the device CSC arrays failed: %s", hipGetErrorString(e)); return e == hipErrorOutOfMemory ? REO_ENOMEM : REO_EHIP; }
    const long long at = static_cast<long long>(csc_column(verdict));
    switch (csc_class(verdict)) {
    case kCscOk: break;
    case kCscColptr:
        set_error("colptr is not a column pointer at column %lld: it must start at 0, be non-decreasing, stay inside [0, nnz = %lld], end at nnz and "
                  "give no column more than G = %lld entries", at, (long long)nnz, (long long)G);
        return REO_EINVAL;
    case kCscRowRange:
        set_error("a row index in column %lld is outside [0,%lld)", at, (long long)G);
        return REO_EINVAL;
    default:
        set_error("the row indices of column %lld are not strictly increasing (unsorted or duplicate entries)", at);
        return REO_EINVAL;
    }
    if (index_bits == 64) { *colptr64 = static_cast<const int64_t *>(d_colptr); return REO_OK; }
    if ((rc = c->csc_colptr.ensure(static_cast<size_t>(S) + 1))) return rc;
    csc_widen_colptr<<<static_cast<unsigned>((S + 1 + 255) / 256), 256, 0, c->stream>>>(static_cast<const int32_t *>(d_colptr), c->csc_colptr.p, S + 1);
    REO_HIP_CHECK(hipGetLastError());
    *colptr64 = c->csc_colptr.p;
    return REO_OK;
}

}  // namespace reo
