// Driver of tests/test_slot_queue_cpu.py: the index rules of the pair kernel's item queues (csrc/k1_queue.h).  Plain host C++ with its
// own main, built with -fsanitize=address,undefined.  W workers draw from the eight counters exactly as a wave of k1w_pairs_slots does
// -- its own label's queue first, the following ones when that is dry -- in a randomly interleaved order, one draw at a time.  Every
// list index 0 .. n-1 has to be taken exactly once and none beyond; the queue lengths sum to n.  Prints one "ok n W" line per case; any
// failed check ends it with 1.
//   g++ -std=c++17 -fsanitize=address,undefined -I rankcompv3.jl_amd/csrc -o driver tests/k1_queue_driver.cpp && ./driver
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "k1_queue.h"

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

static int run_case(uint32_t n, int W, uint32_t seed)
{
    using namespace reo;
    std::mt19937 rng(seed);
    // the queues partition the list
    uint32_t sum = 0;
    for (int x = 0; x < kQueues; ++x) {
        const uint32_t len = queue_len(n, x);
        sum += len;
        uint32_t by_hand = 0;
        for (uint32_t i = static_cast<uint32_t>(x); i < n; i += kQueues) ++by_hand;
        CHECK(len == by_hand);
        if (len) CHECK(queue_index(x, len - 1) < n && queue_index(x, len - 1) + kQueues >= n);
        for (int s = 0; s < kQueues; ++s) CHECK(queue_steal(x, s) >= 0 && queue_steal(x, s) < kQueues);
        CHECK(queue_steal(x, 0) == x);
    }
    CHECK(sum == n);
    // the device buffer: eight counters, each on its own line, zero before the launch
    std::vector<uint32_t> counters(kQueueWords, 0u);
    std::vector<uint8_t> taken(n, 0);   // exactly n long: an index beyond the list is a heap overflow under the sanitizer
    struct Worker { int x, s; bool done; };
    std::vector<Worker> workers(static_cast<size_t>(W));
    for (int w = 0; w < W; ++w) workers[w] = {w & (kQueues - 1), 0, false};
    std::vector<int> live(static_cast<size_t>(W));
    for (int w = 0; w < W; ++w) live[w] = w;
    size_t items = 0, draws = 0;
    while (!live.empty()) {
        const size_t at = rng() % live.size();
        Worker &k = workers[live[at]];
        // one draw of the kernel's loop: fetch-add on the queue's counter, an item or the next queue
        const int q = queue_steal(k.x, k.s);
        const uint32_t m = counters[static_cast<size_t>(q) * kQueueStride]++;
        ++draws;
        if (m < queue_len(n, q)) {
            const uint32_t idx = queue_index(q, m);
            CHECK(idx < n);
            CHECK(!taken[idx]);
            taken[idx] = 1;
            ++items;
        } else if (++k.s == kQueues) {
            k.done = true;
            live[at] = live.back();
            live.pop_back();
        }
    }
    CHECK(items == n);
    for (uint32_t i = 0; i < n; ++i) CHECK(taken[i] == 1);
    CHECK(draws == static_cast<size_t>(n) + static_cast<size_t>(W) * kQueues);   // every worker finds every queue dry once
    for (size_t w = 0; w < counters.size(); ++w)
        if (w % kQueueStride) CHECK(counters[w] == 0);   // nothing but the counters is written
    // the launch's worker count: never more than items, the override wins
    CHECK(queue_workers(n, 256, 0) == (n < 3072u ? n : 3072u));
    CHECK(queue_workers(n, 256, W) == (n < static_cast<uint32_t>(W) ? n : static_cast<uint32_t>(W)));
    printf("ok %u %d draws %zu\n", n, W, draws);
    return 0;
}

int main()
{
    static_assert(reo::kQueueStride * sizeof(uint32_t) == 128, "a counter per 128-byte line");
    const uint32_t ns[] = {0, 1, 7, 8, 9, 1000, 51946};
    const int ws[] = {1, 8, 13, 3072};
    uint32_t seed = 2026;
    for (uint32_t n : ns)
        for (int W : ws)
            if (run_case(n, W, seed++)) return 1;
    return 0;
}
