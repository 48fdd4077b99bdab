// The index rules of the pair kernel's ITEM QUEUES (kernels.hip, k1w_pairs_slots): the slot form is launched with as many one-wave
// workgroups ("workers") as the device holds at three waves per SIMD, and every worker takes items of the list (k1_items.h) until none
// is left.  The list is dealt over eight queues, one per XCD label: item 8 m + x of the list is entry m of queue x, which is what
// workgroup 8 m + x of the one-item-per-workgroup launch ran, so a queue walks its XCD's chunk groups in the list's order.  A queue is
// nothing but a counter: entry m is taken by the worker whose fetch-add returned m.  A worker of label x (blockIdx.x & 7) empties
// queue x first and then the queues x + 1, x + 2, ... (mod 8): placement is a matter of speed only, every entry is taken once whoever
// takes it.  Plain C++ without a context: the kernel and a CPU test (tests/k1_queue_driver.cpp) use the same functions.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define REO_QUEUE_HD __host__ __device__ inline
#else
#define REO_QUEUE_HD inline
#endif

namespace reo {

constexpr int kQueues = 8;              // XCD labels
constexpr int kQueueStride = 32;        // words between two counters: each on its own 128-byte line
constexpr int kQueueWords = kQueues * kQueueStride;

// entries of queue x when the list holds n items: the indices x, x + 8, x + 16, ... below n
REO_QUEUE_HD uint32_t queue_len(uint32_t n, int x) { return (n + static_cast<uint32_t>(kQueues - 1 - x)) / kQueues; }

// the list index of entry m of queue x (m < queue_len(n, x))
REO_QUEUE_HD uint32_t queue_index(int x, uint32_t m) { return m * kQueues + static_cast<uint32_t>(x); }

// the s-th queue that a worker of label x draws from: its own (s = 0), then the following ones
REO_QUEUE_HD int queue_steal(int x, int s) { return (x + s) & (kQueues - 1); }

// workers of a launch: one per wave slot of the device (n_cus x 4 SIMDs x 3 waves), no more than items; `wanted` > 0 overrides (tests)
REO_QUEUE_HD uint32_t queue_workers(uint32_t n, int n_cus, int wanted)
{
    const uint32_t w = wanted > 0 ? static_cast<uint32_t>(wanted) : static_cast<uint32_t>(n_cus) * 4u * 3u;
    return w < n ? w : n;
}

}  // namespace reo
