// Internal declarations shared by the translation units of libreo_hip.so.
// Public C ABI: include/reo_hip.h.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <functional>
#include <string>
#include <type_traits>
#include <vector>

#include "reo_hip.h"

namespace reo {

constexpr int kTileJ = 256;   // lanes per workgroup along j (4 waves x 64 lanes)
constexpr int kTileI = 32;    // gene rows per pair tile (one mirror word)
constexpr int kPlanes = 4;    // cL cH tL tH
constexpr int kUnitH = 32;    // i-tiles per K1 work unit
constexpr int kRJ = 4;        // genes j per lane in the tie-free pair kernel
constexpr int kRJTies = 2;    // genes j per lane in the tie-rich pair kernel (two band edges per pair)
constexpr int kMaxGenes = 262143;  // 18 position planes (above 65 535 genes: 32-bit transform rows, k1w_pairs<17/18>, light passes in the two-launch form)
constexpr int kGenePad = 1024;  // Gp is a multiple of this (= kTileJ * kRJ: every lane's genes exist)
constexpr int kRaw = 8;       // raw tally counters per gene (see k2_tally)
constexpr int kDeltaMax = 128;   // at most this many changed reference genes: update the tallies incrementally
constexpr int kSortChunk = 1024; // genes per bitonic sort in the ranking stage

// Device-resident loop state of the iteration driver (src/RankCompV3.jl:396-425),
// so that passes can be enqueued back to back without a host round trip.
struct IterState {
    int32_t done;      // convergence reached (:419-422): later launches return at once
    int32_t passes;    // executed passes of the while loop
    int32_t nref;      // sum(ref_gene_vec) of the current pass
    int32_t i_iter;    // :397,423
    int32_t ticket;    // finished workgroups of the kernel that ends a pass
    int32_t nn_acc;    // running sum(inds)
    int32_t delta_cnt[2];  // genes whose mask bit changes for the pass of that parity (see delta_genes in kernels.hip)
    int32_t need_full; // the next pass must run on the sorting path (tallies need a table scan, or no quantile windows)
    int32_t raw_pass;  // the tally counters hold the tallies of this pass (-1: none)
    int32_t nref_prev; // nref of the last executed pass (for recomputing its outputs)
    int32_t last_full; // the last executed pass ran on the sorting path: every output column is in place
    int32_t fault;     // 0, or why the passes cannot be trusted (codes below); api.hip answers REO_EHIP
    int32_t kstar;     // the BH cut (number of genes with padj <= padj_deg) of the last executed pass (-1: unknown)
    int32_t kcut_acc;  // running count for kstar (sorting path)
    // cycle watch of the light passes (kernels.hip, "cycle watch"): Brent's search for a pass whose mask equals an earlier one
    int32_t cyc_period; // 0: watching; p > 0: the mask in front of pass `passes` equals the one p passes earlier; -1: not watching
    int32_t cyc_pow;    // passes until the snapshot is renewed (0: no snapshot yet, or a sorting pass has stepped the mask since)
    int32_t cyc_lam;    // mask steps since the snapshot
    int32_t cyc_sel;    // which of the two snapshot buffers holds it
    int32_t cyc_ndiff;  // genes whose mask bit differs from the snapshot's
    int32_t pad[4];
};
constexpr int kFaultBarrier = 1;   // the persistent light kernel gave up at a grid barrier (bounded spin expired)
constexpr int kFaultTallies = 2;   // a gene's tallies broke their invariant: not a class table (kernels.hip, tallies_from)

// Light passes as two launches per pass (kernels.hip, kl_head / kl_rank): the loop state of one batch of launches as an
// append-only log, so that no kernel reads a word that another workgroup of the same launch writes.  rec[b] = the state
// in front of light pass b of the batch (rec of slot nlight: behind the last one), written by workgroup 0 of launch b,
// read by the launches after it.
constexpr int kLightBatch = 128; // most light passes per batch of launches (the first batch of a call: 32)
struct LightRec {
    int32_t active;     // pass `t` is to run as a light pass
    int32_t t;          // passes executed so far = index of the next pass
    int32_t nref, nref_prev, done, need_full, raw_pass;  // as in IterState
    int32_t ran;        // a light pass of this batch has been completed
    int32_t dcnt;       // genes whose mask bit changed in front of pass t
    int32_t kstar;      // the BH cut of the mask step that made this record (-1: none, the record comes from a sorting pass)
    int32_t cper, cpow, clam, csel;  // cycle watch, as IterState::cyc_*
};                      // (no padding array inside: copying one through registers made the compiler keep it in LDS, indexed by a
                        //  thread id that it computed from the dispatch packet -- a 3 us read of host memory at kernel start)
// Counters of one light pass.  A launch cannot end before its atomics have been performed, and atomics on one address
// are performed one after the other (about 12 ns each): 316 waves adding to one word kept kl_rank alive for 3 us after
// its last instruction.  Sums that need no return value are therefore spread over kSpread cache lines (by workgroup)
// and added up by their readers.
constexpr int kHistParts = 8;   // partial histograms of the BH ranks, one per XCD (kernels.hip, kl_rank)
constexpr int kSpread = 8;
constexpr int kListCap = 16;   // genes near the BH cut that one workgroup of kl_rank can list
constexpr int kListWgs = 1024;  // workgroups of 256 genes that the lists and the block moments are sized for (262 144 genes)
static_assert(kMaxGenes <= kListWgs * 256, "the light passes' lists and block moments (clist, part) hold kListWgs workgroups of 256 genes");
constexpr int kPartPer = kListWgs / 256;  // block moments per thread when every workgroup combines all of them
constexpr int kListStride = kListWgs + kListWgs * kListCap * 2;  // int32 per parity: counts by workgroup, then (word, gene) pairs
constexpr int kOneListCap = 16;   // one-launch form (kl_one): genes that one workgroup can list per pass ...
constexpr int kOneListMax = 512;  // ... and that a mask step takes in all (more: the pass goes to the sorting path)
constexpr int kOneStride = 256 + 256 * kOneListCap * 4;  // int32 per parity: counts by workgroup, then entries of 16 bytes (gene | bit << 31, 0, delta1)
struct LightCnt {
    int32_t cnt_a, cnt_b;            // members of the two quantile windows (slot allocation: returned values)
    int32_t pad[30];
    int32_t below_a[kSpread][32];    // values below window A   ([k][0] used: one cache line per part)
    int32_t below_b[kSpread][32];
    int32_t sig[kSpread][32];        // genes with a finite BH rank
    int32_t nsure[kSpread][32];      // one-launch form: genes outside the lists whose BH rank is surely within the cut's band
    int32_t nlow[kSpread][32];       // two-launch form: genes whose BH rank lies below the histogram's first bin (kernels.hip, hist_first)
};
// everything the launches after pass b of a batch need of it: rec = the state in FRONT of pass b; the rest is made by
// pass b itself.  Zeroed by the host in front of the batch.
struct LightSlot {
    LightRec rec;
    int32_t bfail;      // pass b lost a quantile window: it is redone on the sorting path
    int32_t cdiff;      // cycle watch: mask bits that differ from the snapshot after launch b's mask step (workgroup 0 keeps it)
    int32_t cfound;     // ... and, when none does, the period (the launch after this one stops the batch)
    int32_t pad0[5];
    double wnext[4];    // quantile windows for the pass after pass b
    double se_base;     // one-launch form: the se that launch b bracketed its genes' p-values around (the se of the pass before)
    double eta;         // ... and the half width of the bracket, relative
    double pad1[15];
    LightCnt lc;
};
struct LightState { LightSlot slot[kLightBatch + 2]; };
static_assert(sizeof(LightSlot) % 128 == 0, "LightSlot layout");

void set_error(const char *fmt, ...);

#define REO_HIP_CHECK(expr)                                                              \
    do {                                                                                 \
        hipError_t e_ = (expr);                                                          \
        if (e_ != hipSuccess) {                                                          \
            ::reo::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),      \
                             __FILE__, __LINE__);                                        \
            return e_ == hipErrorOutOfMemory ? REO_ENOMEM : REO_EHIP;                    \
        }                                                                                \
    } while (0)

// Process-wide cache of device (and pinned host) blocks (api.hip).  The drop-in call makes a context, runs and destroys it
// (julia/RankCompV3HIP.jl): about forty hipMalloc / hipFree pairs per call cost 6 ms at config 3 -- as much as the whole step.  A
// released block goes to a free list instead (up to REO_DEVICE_CACHE_MB, default 16384; 0 switches the cache off) and the next
// request of that size on that device takes it from there; reo_trim_memory() gives everything back.  hipFree waits for the device
// before it unmaps; a cached block must be just as idle before someone else gets it, so release() waits for the device unless the
// caller says it has waited already (reo_destroy: after its streams, once for all of its buffers).
hipError_t pool_alloc(void **p, size_t bytes, bool pinned);
void pool_free(void *p, size_t bytes, bool pinned);
extern thread_local bool tl_release_synced;   // the releasing thread has waited for everything that used the blocks it releases
// Streams and events of destroyed contexts wait in the same kind of store (a context per call made and destroyed ~6 streams and ~40
// events: 1.2 ms of an 8 ms call).  kind: streams 0 normal / 1 high priority; events 0 without timing / 1 with.  A handle goes back only
// from reo_destroy, behind the waits for every stream of the context.
hipError_t handle_stream(hipStream_t *s, int kind);
hipError_t handle_event(hipEvent_t *e, int kind);
void release_stream(hipStream_t s, int kind);
void release_event(hipEvent_t e, int kind);

template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }  // locals are freed on every return path; context members with the context
    int32_t ensure(size_t count)
    {
        if (count <= n && p) return REO_OK;
        release();
        REO_HIP_CHECK(pool_alloc(reinterpret_cast<void **>(&p), count * sizeof(T), false));
        n = count;
        return REO_OK;
    }
    void release()
    {
        if (p) {
            if (!tl_release_synced) (void)hipDeviceSynchronize();   // (what hipFree did implicitly)
            pool_free(p, n * sizeof(T), false);
        }
        p = nullptr;
        n = 0;
    }
};

struct StageTimer {
    hipEvent_t a = nullptr, b = nullptr;
};

}  // namespace reo

struct reo_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    uint64_t seed = 0;
    int rank = 0, world = 1;
    reo_allreduce_fn ar = nullptr;
    void *ar_user = nullptr;
    reo_allgather_fn ag = nullptr;
    void *ag_user = nullptr;

    // problem
    int64_t G = 0, S = 0, ld = 0;
    int dtype = 0;  // of the resident matrix: 0 none, 1 f64, 2 i64, 3 f32 (Int32 input is widened to Int64: 2)
    const void *dX = nullptr;
    reo::DevBuf<unsigned char> dX_owned;
    std::vector<int32_t> group_id;
    int ngroups = 0;
    std::vector<int32_t> thr;  // 2 x ngroups
    bool thr_set = false;

    // rank/band transform output (samples re-ordered so groups are contiguous)
    int Gp = 0, Wp = 0;  // padded gene count, 32-bit words per bit row
    std::vector<int32_t> goff;   // ngroups+1 offsets into the sorted sample order
    std::vector<int32_t> goff32; // the same with every group padded to whole blocks of 32 sample slots
    // bit planes over 32-sample blocks (transform.hip, t_slice); nblk = goff32.back() / 32
    reo::DevBuf<uint4> pos;     // [nblk][4][Gp]  planes 4q..4q+3 of the position of gene g in its sample's sorted order
    reo::DevBuf<uint4> lo;      // [nblk][Gp][4]  16 plane words of the first position of the tie band (plane k in word (k+15)%16)
    reo::DevBuf<uint4> hi;      // [nblk][Gp][4]  the same for one past the last position of the tie band
    reo::DevBuf<uint16_t> t_pos16, t_lo16, t_hi16;  // [S32][Gp] the three numbers before slicing (scratch)
    reo::DevBuf<uint32_t> t_pos32, t_lo32, t_hi32;  // the same for more than 65 535 genes (32-bit positions; transform.hip, t_slice_big)
    reo::DevBuf<uint32_t> t_vin32, t_vout32;        // by-slot scratch of the bucket ranking (!GENL); gene indices of the A/B build's segmented sort, 32-bit
    reo::DevBuf<int32_t> goff_dev;  // group offsets in blocks
    // transform scratch (grow-only, freed with the context)
    reo::DevBuf<uint64_t> t_kin, t_kout;
    reo::DevBuf<uint16_t> t_vin, t_vout;
    reo::DevBuf<unsigned char> t_temp;
    reo::DevBuf<int32_t> t_order, t_flags, t_slots;
    reo::DevBuf<uint32_t> unit_map;  // K1 work units: panel << 16 | i-range
    std::vector<uint32_t> unit_map_host;          // what unit_map holds (launch_k1 uploads only a different list)
    std::vector<int32_t> t_order_host, t_slots_host, goff_blocks_host;  // what t_order / t_slots / goff_dev hold (transform: uploaded when they change)
    const int32_t *t_meta_ptr[3] = {nullptr, nullptr, nullptr};
    int32_t *host_flags = nullptr;       // pinned: the transform's flags on their way to the host
    hipEvent_t ev_flags = nullptr;       // ... and the point of the stream at which they have arrived
    bool table_prezeroed = false;        // the transform has already queued the clearing of the class table (behind its flags copy)
    const uint32_t *unit_map_uploaded = nullptr;  // ... and into which allocation
    size_t k1_items_n = 0;           // wave form of K1: items of the launch being made (one work item per workgroup: side << 31 | wave chunk << 16 | i-tile; lists: k1_wave_items)
    bool transformed = false;
    // pipelined upload of a host matrix (transform.hip, eager_upload): chunks on an upload stream, ranked as they arrive
    int eager_mode = 2;                  // REO_EAGER_UPLOAD: 0 off, 1 transform only, 2 (default) the pair kernel's sides as well
    int eager_chunk = 0;                 // REO_EAGER_CHUNK: columns per chunk (0: about 8 MB)
    int eager_gate = 1;                  // REO_EAGER_GATE=0: the host reads the transform's flags before it launches a side (A/B)
    hipStream_t up = nullptr, rk = nullptr;   // the upload stream; the stream that widens, ranks and slices the chunks (high priority)
    hipEvent_t ev_up[8] = {nullptr};     // chunk k has arrived (ring)
    hipEvent_t ev_rk[4] = {nullptr, nullptr, nullptr, nullptr};   // fork from / join into the context's stream; a side's planes are in place (two sides)
    reo::DevBuf<int32_t> e_lists;        // [S] columns, [S + padding] slots, in column order
    // narrowed upload of Int64 matrices: host threads convert a chunk to 16- or 32-bit numbers in a pinned staging slot, a kernel widens it
    int upload_threads = 12;             // REO_UPLOAD_THREADS (0: the caller's array goes over the link as it is)
    unsigned char *stage_h[3] = {nullptr, nullptr, nullptr};   // pinned staging slots (from the block cache)
    size_t stage_cap = 0;                // bytes of each
    reo::DevBuf<unsigned char> stage_d[3];
    hipEvent_t ev_stage[3] = {nullptr, nullptr, nullptr}, ev_widen[3] = {nullptr, nullptr, nullptr};
    int64_t narrowed_bytes = 0;          // bytes the last pipelined upload put on the link (reo_get_info 19)
    int rowmajor_upload = 0;             // the last host matrix was read row-major in place (reo_set_matrix_rm_*; reo_get_info 21)
    int csc_upload = 0;                  // the last host matrix came as CSC (reo_set_matrix_csc_*; reo_get_info 22) ...
    int64_t csc_nnz = 0;                 // ... with this many stored entries (reo_get_info 23)
    reo::DevBuf<int64_t> csc_colptr;     // its column pointer, which t_csc_columns reads (transform.hip, CscUploader)
    int csc_device = 0;                  // the matrix came from CSC arrays on the device (reo_set_matrix_csc_dev_*; reo_get_info 27)
    bool eager_k1 = false;               // reo_set_matrix has already launched the pair kernel of comparison 0 on this data, groups and thresholds
    int has_ties = 0;
    int transform_in_lds = 0;  // the last transform sorted each sample inside one workgroup's LDS (transform.hip)

    // class table: [G][4 planes][Wp] 32-bit words
    reo::DevBuf<uint32_t> table;
    int built_k = -1;
    int built_treat = -1;               // reo_get_info 29: the treat group of the resident table (reo_build_pairs_contrast), -1: every other sample
    bool table_complete = false;        // world > 1: the shards' parts have been summed (api.hip, exchange_table)
    void *comm = nullptr;               // ncclComm_t of the in-library RCCL path (comm.hip), or null
    int spin_wait = 0;                  // REO_SPIN_WAIT=1: poll the stream on the hot path instead of the blocking wait (api.hip, stream_wait; measured: 0.04 ms per step)
    int check_hook_table = 1;           // REO_CHECK_HOOK_TABLE=0: skip the consistency scan of a table delivered by a caller's hook (timing tools)
    bool comm_dead = false;             // the communicator was aborted after a failure: every later build answers REO_ECOMM
    bool in_multi = false;              // this context is the leader or a peer of a reo_create_multi context (its exchange is multi_build_pairs', not launch_k1's)
    bool multi_one_device = false;      // reo_create_multi under REO_MULTI_ONE_DEVICE=1 (test seam: shards share one device, no RCCL)
    std::vector<reo_ctx *> peers;       // reo_create_multi: the contexts of devices 1.. owned by this (leader) context
    // one-vs-rest with > 2 groups: per-group pair counts shared by the comparisons (kernels.hip, k1_group_counts)
    reo::DevBuf<uint16_t> gcounts;      // [ngroups + 1][Gp/32][4][Gp][8]
    bool gc_valid = false;
    int k1_wave = 1;                    // REO_K1_WAVE=0: the workgroup form of the pair kernel (round 2) instead of the wave form
    int k1_order = 0;                   // REO_K1_ORDER=1 (experiment): the wave form's items i-tile-fastest inside a chunk instead of chunk-fastest inside an i-tile
    int k1_half = 1;                    // REO_K1_HALF=0: no half-height items in the last round of the wave form's launch
    // slot order of the pair kernel (kernels.hip, k1_slots; index rules: k1_slots.h): tie-free data of two groups on one shard is counted
    // with the genes ordered by level, and the table's rows and columns come back in gene order before launch_k1 returns
    int k1_slots = 1;                   // REO_K1_SLOTS=0: the identity order for everything (A/B, tests)
    int last_k1_slots = 0;              // reo_get_info 25: the last build of the class table used the slot order
    int k1_unslot = -1;                 // REO_K1_UNSLOT: the column un-permute behind a slot build -- unset: the word form of unslot_form (k1_slots.h); 0: the bit form
                                        // (k1_unslot_columns; A/B, tests); 8 or 4: that word form wherever its LDS fits (tests)
    int k1_slot_sides = 0;              // REO_K1_SLOT_SIDES: 1 one slot order for both sides everywhere, 2 an order per side wherever slot order runs with a word
                                        // un-permute (A/B, tests); unset: per side from 16 sample blocks on (k1_slots.h, slot_sides_wanted)
    int last_k1_slot_sides = 0;         // reo_get_info 30: 0 no slot build, 1 the common order, 2 an order per side
    int last_k1_unslot = 0;             // reo_get_info 28: the un-permute of the last build (0: no slot build; 1: the bit form; 8 or 4: the word forms)
    int k1_unslot_attr = 0;             // word forms whose kernel has been given its LDS size (bit 0: wide, bit 1: narrow; bits 2, 3: their pair forms)
    const uint32_t *k1_slot_items = nullptr;   // ... and its item list (one of k1_wave_items), for the count of separated items (reo_get_info 26)
    size_t k1_slot_items_n = 0;
    int k1_slot_gp = 0;                 // ... and the padded gene count its maps and ranges are laid out for
    reo::DevBuf<uint32_t> k1_slot_part; // [kSlotSplits][2][Gp] the sides' position ranges of every gene over a slice of the samples (min | max << 16)
    reo::DevBuf<uint32_t> k1_slot_maps; // [2][Gp] ranges per side, [2][Gp] keys, [2][Gp] g2s, [2][Gp] s2g, [2][Gp / 32] tile ranges, [2][Gp / 256] chunk ranges, [2] a count
    reo::DevBuf<uint4> pos_s, lo_s;     // the pos and lo planes in slot order (the layouts of pos and lo)
    int k1_slot_slice = 1;              // REO_K1_SLOT_SLICE=0: a slot build makes the gene-order planes and gathers them (k1_slot_gather; A/B, tests) instead of
                                        // slicing the 16-bit position rows straight into slot order (k1_slot_slice)
    int last_k1_slot_slice = 0;         // reo_get_info 32: the last build's operands came from k1_slot_slice
    // The gene-order planes (pos, lo, hi) on demand: a transform of tie-free data whose next build can be a slot build leaves them unmade,
    // and whoever reads them calls ensure_planes first (transform.hip), which slices the 16-bit rows -- they live until the next transform.
    bool planes_ready = false;          // pos, lo and hi hold the planes of the current transform (or their slicing is queued in front of every reader)
    int planes_on_demand = 0;           // reo_get_info 33: how many times the current transform's planes were made by ensure_planes
    // item queues of the slot form (kernels.hip, k1w_pairs_slots; index rules: k1_queue.h): resident waves take items from eight counters
    int k1_queue = 1;                   // REO_K1_QUEUE=0: one workgroup per item, as the identity order's kernels (A/B, tests)
    int k1_workers = 0;                 // REO_K1_WORKERS=n (tests): workgroups of the launch instead of CUs x 4 SIMDs x 3 waves
    reo::DevBuf<uint32_t> k1_queue_ctr; // [kQueueWords] the counters, each on its own 128-byte line; cleared on the stream before every launch
    int n_cus = 256;                    // compute units of the device (the wave form's item slots = CUs x 4 SIMDs x waves per SIMD)
    int share_counts = 1;               // REO_SHARE_GROUP_COUNTS=0 recounts per comparison instead
    int last_k1_shared = 0;             // reo_get_info: how the last class table was built
    int64_t tiles_owned = 0, tiles_total = 0;
    int k1_cj = 0, k1_q = 0;  // K1 geometry of the last build: genes j per workgroup, j-chunks per panel
    // gather form of the exchange (kernels.hip, x_pack / x_expand_*): every work unit of the last build (panel << 16 | i-range,
    // owner = index % world), pack and gather buffers
    std::vector<uint32_t> units_all_host, units_all_dev;   // ... and what the device copy holds
    const uint32_t *units_all_uploaded = nullptr;
    reo::DevBuf<uint32_t> units_all, xsend, xrecv;
    // pipelined exchange (several shards, wave form of the pair kernel): the shard's units are counted in waves, and wave w is
    // packed, gathered and unpacked on a second stream while wave w + 1 is being counted (kernels.hip, launch_k1)
    int x_waves = 4;                    // REO_EXCHANGE_WAVES (1: the whole exchange behind the pair kernel, as in round 3)
    bool x_pipelined = false;           // the last launch_k1 has already exchanged the table
    hipStream_t k1s[2] = {nullptr, nullptr}, xs = nullptr;
    hipEvent_t ev_fork = nullptr, ev_k1[8] = {nullptr}, ev_k1_join[2] = {nullptr, nullptr}, ev_x = nullptr;
    struct ItemList { reo::DevBuf<uint32_t> buf; size_t n = 0; uint64_t key[5] = {0, 0, 0, 0, 0}; };
    ItemList k1_wave_items[8];          // the item lists of the waves (kept until the geometry changes)
    reo::DevBuf<uint32_t> k1_park[2];   // range items of the pipelined upload: parked counts of a side, [items][kParkSlot] (kernels.hip)
    reo::DevBuf<int32_t> k1_park_ge[2]; // ... and which slots hold n_ge of their own
    int64_t eager_range_launches = 0;   // launches of the pair kernel that the last pipelined upload made over RANGES of a side's blocks (reo_get_info 20)
    int eager_ranges = -1;              // REO_EAGER_RANGES: ranges of sample blocks per side in the pipelined upload (1: whole sides, as in round 5; -1: by shape)
    reo::DevBuf<int32_t> check_flag;    // [1] verdict of k_check_table (kernels.hip, launch_check_table)

    // iteration state
    reo::DevBuf<uint32_t> refbits[2];   // [Wp]
    reo::DevBuf<uint8_t> refbytes[2];   // [Gp]
    // reo_get_ref_mask / reo_pair_list: which of the two slots holds the reference set that the last reo_identify_degs counted its returned
    // tallies over -- the mask of its last executed pass t, slot t & 1 (pass t writes the NEXT set into the other slot) -- or -1 and why not
    int ref_slot = -1;
    const char *ref_gone = "reo_identify_degs has not run on this context";
    // reo_sample_counts: the caller's column of every sample slot (-1: padding), uploaded when the groups have changed
    reo::DevBuf<int32_t> sc_slot2col;   // [32 * sample blocks]
    std::vector<int32_t> sc_slot2col_host;      // what it holds ...
    const int32_t *sc_slot2col_uploaded = nullptr;   // ... and in which allocation
    // reo_sample_tests: the log-factorial table lf[0 .. 2 (G - 1)] (sample_tests.h), uploaded once and rebuilt when G changes
    reo::DevBuf<double> st_lf;
    int64_t st_lf_G = -1;               // the G it was built for (-1: none)
    // missing values (reo_set_valid_mask, reo_build_pairs_masked; maskedpairs.hip, masked_pairs.h)
    reo::DevBuf<uint8_t> vmask;         // [S][G] the validity bytes, column-major in the caller's column order (nonzero = observed)
    bool vmask_set = false;
    int64_t vmask_G = 0, vmask_S = 0;   // the shape it was set for: a matrix of another shape drops it (api.hip, mask_in_force)
    reo::DevBuf<uint32_t> vwords;       // [sample blocks][Gp] one validity word per block of 32 sample slots and gene, in slot order
    bool vwords_valid = false;          // ... made from vmask under the current groups (set_groups and a new mask clear it)
    reo::DevBuf<int32_t> mp_thr;        // m(0 .. n1) then m(0 .. n2): the thresholds of every number of jointly observed samples per side
    std::vector<int32_t> mp_thr_host;   // what it holds ...
    int32_t mp_thr_n[2] = {-1, -1};     // ... for these side sizes ...
    double mp_thr_pval = -1.0;          // ... and this pval_reo
    const int32_t *mp_thr_uploaded = nullptr;   // ... and in which allocation
    int built_masked = 0;               // reo_get_info 31: the resident class table came from reo_build_pairs_masked
    // label-permutation null (reo_perm_null; permpairs.hip, perm_null.h)
    int64_t perm_batch = 0;             // reo_get_info 34: tables per batch of the last reo_perm_null
    int64_t perm_kernel_us = 0;         // reo_get_info 35: microseconds its launches of k_pairs_permuted took in all (HIP events)
    // top-scoring pairs (reo_top_pairs; toppairs.hip, top_pairs.h)
    int64_t top_hist_us = 0;            // reo_get_info 36: microseconds the histogram passes of the last reo_top_pairs took in all (HIP events)
    int64_t top_emit_us = 0;            // reo_get_info 37: microseconds of its emit pass
    int64_t top_null_batch = 0;         // reo_get_info 38: permutations per launch of the last reo_top_pairs_null
    int64_t top_null_us = 0;            // reo_get_info 39: microseconds its launches of k_top_pairs_null took in all (HIP events)
    int64_t top_loo_words_us = 0;       // reo_get_info 40: microseconds k_loo_words of the last reo_top_pairs_loo took (HIP events)
    int64_t top_loo_select_us = 0;      // reo_get_info 41: microseconds of its k_loo_select
    int64_t top_partners_count_us = 0;  // reo_get_info 42: microseconds the launches of k_top_partners_count of the last reo_top_partners took in all (HIP events)
    int64_t top_partners_select_us = 0; // reo_get_info 43: microseconds of its launches of k_top_partners_select
    int64_t top_partners_null_batch = 0; // reo_get_info 44: permutations per launch of the last reo_top_partners_null
    int64_t top_partners_null_us = 0;    // reo_get_info 45: microseconds its launches of k_top_partners_null took in all (HIP events)
    reo::DevBuf<int32_t> raw;           // [G][8]
    reo::DevBuf<uint32_t> delta_list;   // [2][Gp] changed genes (gene << 1 | added) per pass parity
    reo::DevBuf<int32_t> cont;          // [G][9]
    reo::DevBuf<double> result;         // [15][G]
    reo::DevBuf<double> sorted_d;       // [G]
    reo::DevBuf<double> sorted_p;       // [G]
    reo::DevBuf<uint32_t> rank_s, rank_a;  // [G]
    reo::DevBuf<double> scal;           // [8] device scalars (se, ...)
    reo::DevBuf<double> blockmin;       // [<= 64]
    reo::DevBuf<double> chunk_v;        // [nchunk][kSortChunk] chunk-sorted delta1
    reo::DevBuf<uint16_t> chunk_i;      // [nchunk][kSortChunk] gene offsets inside the chunk
    reo::DevBuf<double> part;           // [<= 256][3] slice moments per block
    reo::DevBuf<reo::IterState> state;  // [1]
    reo::DevBuf<int32_t> trace;         // [n_iter][2]
    reo::DevBuf<int32_t> modes;         // [K2 launches] 1 = the launch scanned the whole table, 0 = incremental update or skipped
    reo::DevBuf<double> cand;           // [2 parities][2 windows][64] light passes: values inside the quantile windows
    reo::DevBuf<unsigned> gridbar;      // [1] arrival counter of the persistent light kernel's grid barrier
    reo::DevBuf<reo::LightState> lstate;  // [1] batch log of the two-launch light passes
    reo::DevBuf<int32_t> clist;         // [2][256 + 256 * kListCap * 2] genes near the BH cut, by workgroup (kernels.hip, kl_rank)
    int light_band = 32;                // REO_LIGHT_BAND (tests)
    bool cycle_watch = true;            // REO_CYCLE=0 switches the cycle watch of the light passes off (every pass is then executed)
    reo::DevBuf<uint8_t> snap;          // [2][Gp] cycle watch: mask snapshots
    int it_cycle_period = 0, it_cycle_at = 0, it_cycle_skipped = 0;  // the last reo_identify_degs: period found (0: none), in front of which pass, passes skipped
    int hist_below = 256;               // REO_HIST_BELOW (tests): ranks under the last cut that keep a histogram bin (kernels.hip, hist_first)
    int xcc_local = 0;                  // the per-XCD histogram atomics may stay in the XCD's L2 (checked once per context: kernels.hip, xcc_selftest)
    int light_window = 24, light_min_g = 4096;  // set from kernels.hip's constants in reo_create (REO_LIGHT_WINDOW, REO_LIGHT_MIN_G)
    int light_mode = 1;                 // 0 sorting passes only, 1 light passes as two launches each (the default), 2 as one persistent launch,
                                        // 3 as ONE launch each (round 4: measured slower, 24.0 against 23.1 us per pass; opt-in) (REO_LIGHT)
    reo::DevBuf<int32_t> olist;         // [2][kOneStride] one-launch form: the genes near the BH cut with their delta1, by workgroup (kernels.hip, kl_one)
    reo::DevBuf<int32_t> hist, mrank;   // [2][G padded to whole 32768-bin rounds], [Gp] light passes: histogram of the BH ranks (by launch parity), the ranks
    // parameters of the running reo_identify_degs call (kernels.hip, iter_args)
    double it_pval_deg = 1.0, it_padj_deg = 0.05;
    int it_n_iter = 0, it_n_conv = 0, it_a0 = 0, it_b0 = 0;
    int k2_idx = 0;                     // K2 launches of the running call
    int it_light_form = 1;              // the form of light pass the running call uses (light_mode, or 1 above 65 535 genes)
    bool it_no_light = false;           // the running call has given up on light passes (two light batches in a row completed no pass)
    reo::IterState *host_state = nullptr;  // pinned
    bool state_mirror_wanted = true;       // REO_STATE_MIRROR=0 (read once, in reo_create, like every other switch)
    bool debug_passes = false, debug_stamps = false, k1_stamps = false;  // REO_DEBUG_PASSES, REO_DEBUG_STAMPS, REO_K1_STAMPS (diagnostics)
    bool state_mirror = false;             // the kernels write what the host reads of IterState straight into host_state (REO_STATE_MIRROR=0: a copy per batch)
    uint8_t *host_ref = nullptr;           // pinned: the caller's reference mask on its way to the device (reo_identify_degs)
    size_t host_ref_cap = 0;

    // timing
    bool profiling = false;
    double t_ms[REO_NTIMINGS] = {0};
    std::vector<std::pair<int, reo::StageTimer>> pending;  // (slot, events)
    std::vector<reo::StageTimer> pool;
    std::vector<size_t> open;  // indices into pending of timers not yet closed (tic/toc nest)
    std::vector<int32_t> k2_modes;  // per pass of the last identify_degs call: 1 = full table scan in K2
    size_t k2_seen = 0;
};

namespace reo {

// transform.hip
int32_t run_transform(reo_ctx *c);
// the gene-order planes of the current transform, made now (t_slice over the whole matrix on c->stream) if the transform left them unmade
int32_t ensure_planes(reo_ctx *c);
// host matrix -> HBM in chunks, ranked (and paired) as they arrive (host_i32: the host array is Int32, the resident matrix Int64)
// how a host matrix lies: column-major (hld = leading dimension), row-major (genes x samples, hld = its pitch), or CSC (hX points at the
// reo::CscSrc<element type> of upload_csc.h, hld unused)
enum { kLayoutColMajor = 0, kLayoutRowMajor = 1, kLayoutCsc = 2 };
int32_t eager_upload(reo_ctx *c, const void *hX, int64_t hld, bool with_k1, bool host_i32 = false, int layout = kLayoutColMajor);
int32_t upload_columns(reo_ctx *c, const void *hX, int64_t hld, int64_t G, int64_t ncols, void *dX, int dtype, int layout = kLayoutColMajor);  // a host matrix into a device matrix (ld = G), chunked, Int64 narrowed
int32_t widen_device_i32(reo_ctx *c, const void *dX32, int64_t ld, int64_t G, int64_t S, void *dX64);  // a device Int32 matrix into a dense Int64 one, on c->stream
int32_t densify_device_csc(reo_ctx *c, int64_t G, int64_t S, const int64_t *colptr, const void *rows, int32_t index_bits, const void *vals,
                           int dtype, void *dX);  // a checked device CSC matrix into a dense one (ld = G), on c->stream
int32_t ensure_upload_streams(reo_ctx *c);                                      // c->up, c->rk and their events (created on first use)
int32_t ensure_staging(reo_ctx *c, size_t slot_bytes);                          // three pinned + device staging slots of at least that size, their events
void host_parallel(int nthreads, int ntasks, const std::function<void(int)> &fn);   // fn(0 .. ntasks - 1) on the process-wide pool of host threads (and the caller)

// kernels.hip
// range: the launch covers sample blocks [b0, b1) of its ONE side (counted from the side's first block); the counts wait in the context's park
// buffer between the ranges of a side and the launch of the last range classifies (kernels.hip, K1Args::park).  prepare: only make
// (and upload) the unit map and the item list of `sides` -- the pipelined upload does that before it queues any wait on the stream.
struct K1Range { int b0, b1; bool first, last; };
// treat: -1 = comparison k against every other sample; a group id = the contrast of group k against that group alone, classified from
// the shared per-group count planes (more than two groups; contrast.h) -- whole table only.
int32_t launch_k1(reo_ctx *c, int k, int sides = 3, bool keep_table = false, const int32_t *gate = nullptr, const K1Range *range = nullptr,
                  bool prepare = false, int treat = -1);  // sides: bit 0 = the comparison's own group, bit 1 = the rest (wave form; eager_upload)
// whether the shared per-group count planes of the context's problem are resident or fit the free device memory, and their size
int32_t k1_planes_fit(reo_ctx *c, bool *fit, size_t *need_bytes);
int64_t exchange_unit_words(const reo_ctx *c);   // uint32 per packed work unit
int32_t exchange_units_per_rank(const reo_ctx *c);
int32_t launch_pack_units(reo_ctx *c, int m0 = 0, int mcnt = -1, uint32_t *send = nullptr, hipStream_t st = nullptr);    // this shard's units (all, or slots m0 .. m0 + mcnt - 1) -> c->xsend / send
int32_t launch_expand_units(reo_ctx *c, int m0 = 0, int mcnt = -1, const uint32_t *recv = nullptr, hipStream_t st = nullptr);  // every shard's pack -> the table: the others' words and their mirrors
int32_t launch_slot_separated(reo_ctx *c, int64_t *half_tiles);   // half-height tiles of the last build whose count loop was skipped (0 without slot order; waits for the stream)
int32_t launch_counts(reo_ctx *c, int64_t i0, int64_t i1, int64_t j0, int64_t j1, uint16_t *d_gt, uint16_t *d_eq);
int32_t launch_check_table(reo_ctx *c, int *bad);  // consistency of an exchanged class table (kernels.hip, k_check_table)
int32_t launch_decode(reo_ctx *c, int64_t i0, int64_t i1, int64_t j0, int64_t j1, uint8_t *d_code);
int32_t launch_pack_ref(reo_ctx *c, const uint8_t *d_bytes, uint32_t *d_bits);
int32_t launch_cycle_skip(reo_ctx *c, int skip, int period);  // cycle watch: move the loop state `skip` passes on (whole periods), fill their trace, end the watch
int32_t launch_iter_init(reo_ctx *c, const uint8_t *host_ref, const IterState *host_state);  // mask + loop state from pinned host memory, clears
int32_t launch_tally(reo_ctx *c, int nref);
int32_t launch_full_pass(reo_ctx *c, bool replay);
int32_t launch_light_persistent(reo_ctx *c);
int32_t launch_light_batch(reo_ctx *c, int nlight);
int32_t xcc_selftest(reo_ctx *c, int *ok);
int32_t light_min_genes();
int32_t light_window();
int32_t launch_mccullagh(reo_ctx *c, const int32_t *d_cont, int64_t n, double *d_out);

// What the launchers of the plane-reading kernels share (band_chain.h).
int plane_bits(int64_t G);   // kernels.hip: position planes that the count loops read
// The guard in front of a kernel that reads the planes of the 16-plane layout: they exist, for at most max_genes genes, and are sliced.
inline int32_t need_planes(reo_ctx *c, const char *what, int64_t max_genes)
{
    if (c->pos.p && c->lo.p && c->hi.p && c->goff_dev.p && !c->goff32.empty() && c->ngroups >= 1 && c->G <= max_genes) return ensure_planes(c);
    set_error("%s: no bit planes", what);
    return REO_EINVAL;
}
// f(std::integral_constant<int, NB>) with NB = plane_bits(G) of the 16-plane layout, 12, 15 or 16: one kernel instantiation per number of
// planes that the chain reads, so that its trip count is a constant without a guard per plane.
template <typename F>
void with_plane_bits(int64_t G, F &&f)
{
    switch (plane_bits(G)) {
    case 12: f(std::integral_constant<int, 12>{}); break;
    case 15: f(std::integral_constant<int, 15>{}); break;
    default: f(std::integral_constant<int, 16>{}); break;
    }
}
// The grid of the tiled kernels: a wave owns 64 of `cols` columns and `tile_rows` of `rows` rows, `waves` waves a workgroup.
inline dim3 tile_grid(int64_t cols, int64_t rows, int tile_rows, int waves, int z = 1)
{
    const unsigned ctiles = static_cast<unsigned>((cols + 63) / 64);
    return dim3((ctiles + waves - 1) / waves, static_cast<unsigned>((rows + tile_rows - 1) / tile_rows), static_cast<unsigned>(z));
}

// pairlist.hip: the kernels of reo_pair_list (shared arithmetic and host checks: pair_list.h).  d_maskbits: [Wp] the partner mask as bits
// (k_pack_ref's layout, a refbits slot); d_genes: [n_genes] query rows, checked by the caller to lie in [0, G)
int32_t launch_pair_count(reo_ctx *c, const int32_t *d_genes, int64_t n_genes, const uint32_t *d_maskbits, uint32_t class_mask, int32_t *d_count);
int32_t launch_pair_fill(reo_ctx *c, const int32_t *d_genes, int64_t n_genes, const uint32_t *d_maskbits, uint32_t class_mask, const int64_t *d_rowptr,
                         int32_t *d_partner, uint8_t *d_code, int64_t capacity, int32_t *d_flag);

// samplecounts.hip: the kernel of reo_sample_counts (shared arithmetic and host checks: sample_counts.h).  d_genes: [n_queries] query rows,
// checked by the caller to lie in [0, G); d_maskbits as above; d_slot2col: [32 * sample blocks] the caller's column of every sample slot, -1
// for padding; d_gt / d_eq: [n_queries][S] (d_eq null: the tied counts are not computed); d_sel: [n_queries]
int32_t launch_sample_counts(reo_ctx *c, const int32_t *d_genes, int64_t n_queries, const uint32_t *d_maskbits, uint32_t class_mask,
                             const int32_t *d_slot2col, int32_t *d_sel, int32_t *d_gt, int32_t *d_eq);

// sampletests.hip: the kernel of reo_sample_tests (shared arithmetic and host checks: sample_tests.h).  The six counts are what two
// launch_sample_counts calls (class masks 0x1C0 and 0x007, tied counts included) left on the device: d_sel_*: [n_queries], the rest
// [n_queries][S]; d_lf: the log-factorial table of lf_entries >= 2 (G - 1) + 1 doubles; d_rev_up / d_rev_down / d_tied: [n_queries][S] or
// null; d_p_up / d_p_down: [n_queries][S]; d_flag: [1], set when a thread met counts that G genes cannot produce
int32_t launch_sample_fisher(reo_ctx *c, int64_t n_queries, const int32_t *d_sel_a, const int32_t *d_sel_b, const int32_t *d_gt_a,
                             const int32_t *d_eq_a, const int32_t *d_gt_b, const int32_t *d_eq_b, const double *d_lf, int64_t lf_entries,
                             int32_t *d_rev_up, int32_t *d_rev_down, int32_t *d_tied, double *d_p_up, double *d_p_down, int32_t *d_flag);

// samplecalls.hip: the three kernels of reo_sample_calls (shared arithmetic and host checks: sample_calls.h).  d_words: the resident cell
// words, [S][call_padded_rows(n_genes)].  launch_call_rank turns the tails of one batch (d_p_up / d_p_down: [nq][S], rows q0 .. q0 + nq - 1
// of the call) into words; launch_call_cut finds every column's cut (d_kstar) and counts the rows within it and the calls of either
// sign (d_cut, d_n_up, d_n_down: [S] each); launch_call_emit stores the calls, d_calls: [n_genes][S]
int32_t launch_call_rank(reo_ctx *c, int64_t n_genes, int64_t q0, int64_t nq, const double *d_p_up, const double *d_p_down, double pval_deg,
                         double padj_deg, uint32_t *d_words);
int32_t launch_call_cut(reo_ctx *c, int64_t n_genes, const uint32_t *d_words, int32_t *d_kstar, int32_t *d_cut, int32_t *d_n_up, int32_t *d_n_down);
int32_t launch_call_emit(reo_ctx *c, int64_t n_genes, const uint32_t *d_words, const int32_t *d_kstar, int8_t *d_calls);

// pairsupport.hip: the kernel of reo_pair_support (work items, batches and host checks: pair_support.h).  d_items: [n_items] work items of the
// batch; d_partner: [entries of the batch] partners, checked by the caller to lie in [0, G) and off the diagonal; d_slot2col as above (read
// only with d_outcome); d_gt / d_eq: [entries][ngroups] (d_eq null: no tied counts); d_outcome: [entries][S] bytes or null
struct PsItem;
int32_t launch_pair_support(reo_ctx *c, const PsItem *d_items, int64_t n_items, const int32_t *d_partner, const int32_t *d_slot2col,
                            int32_t *d_gt, int32_t *d_eq, uint8_t *d_outcome);

// toppairs.hip: the kernels of reo_rank_shift / reo_top_pairs (the key, the pass loop and the host checks: top_pairs.h).  d_gside: [ngroups]
// the side of every group (0: A, 1: B, 2: neither); d_D: [Gp] the rank shifts, which launch_rank_shift fills (0 for genes >= G);
// d_maskbits: [Wp] the gene mask as bits, or null for every gene.  launch_top_hist adds the histogram of one pass (prefix, digit at bit
// `shift`) into d_hist ([kTpHistWords], cleared by the caller); launch_top_emit appends every pair with key >> shift >= cut to d_cand
// ([capacity] records) and counts them all in d_cand_n ([1], cleared by the caller)
struct TpKey;
struct TpRec;
int32_t launch_rank_shift(reo_ctx *c, const int32_t *d_gside, int s_a, int s_b, int64_t *d_D, int64_t *d_sums = nullptr);   // d_sums: [2][Gp] sum_A, sum_B of lo + hi, or null
int32_t launch_top_hist(reo_ctx *c, const int32_t *d_gside, int s_a, int s_b, const int64_t *d_D, const uint32_t *d_maskbits, const TpKey &prefix,
                        int shift, unsigned long long *d_hist);
int32_t launch_top_emit(reo_ctx *c, const int32_t *d_gside, int s_a, int s_b, const int64_t *d_D, const uint32_t *d_maskbits, const TpKey &cut,
                        int shift, TpRec *d_cand, int64_t capacity, uint32_t *d_cand_n);

// toppairsnull.hip: the kernels of reo_top_pairs_null (the key, the word packing and the host checks: top_pairs_null.h).
// launch_top_null_words: the label rows d_side ([n_perm][S] bytes 0 / 1 / 2, checked by the caller, n_perm <= kTnBatchCap) and d_slot2col
// into the A-words d_aw (pn_word_count(n_perm, blocks) words, cleared here) and the live words d_live ([blocks]: the slots of the two
// sides).  launch_top_pairs_null: for permutations 0 .. np - 1 of those words the largest key into d_keys ([kTnBatchCap], atomicMax) and
// the pairs with |N| >= cuts[t] into d_reach ([kTnBatchCap][kTnMaxCuts], atomicAdd); the caller has cleared both; cuts: HOST, n_cuts values
int32_t launch_top_null_words(reo_ctx *c, const uint8_t *d_side, int64_t n_perm, const int32_t *d_slot2col, uint32_t *d_aw, uint32_t *d_live);
int32_t launch_top_pairs_null(reo_ctx *c, const uint32_t *d_aw, const uint32_t *d_live, int np, int s_a, int s_b, const uint32_t *d_maskbits,
                              const int64_t *cuts, int n_cuts, unsigned long long *d_keys, unsigned long long *d_reach);

// toppairsloo.hip: the kernels of reo_top_pairs_loo (the fold arithmetic, the cut rule and the host checks: top_pairs_loo.h).
// launch_loo_words: for the n_cand records of d_cand (the emit pass's, on the device) and every block of 32 sample slots the gt word and
// the eq word of the pair into d_words ([blocks][n_cand]).  launch_loo_select: one workgroup per sample slot decides the fold of that slot
// from d_cand, d_words and d_sums ([2][Gp] of launch_rank_shift) and stores its kmax picks into row slot2col[slot] of d_i, d_j, d_n, d_g,
// d_o ([S][kmax], preset by the caller: rows of no fold and picks that do not exist keep what they hold)
int32_t launch_loo_words(reo_ctx *c, const TpRec *d_cand, int64_t n_cand, uint2 *d_words);
int32_t launch_loo_select(reo_ctx *c, const TpRec *d_cand, int64_t n_cand, const uint2 *d_words, const int32_t *d_gside, const int32_t *d_slot2col,
                          const int64_t *d_sums, int s_a, int s_b, int kmax, int32_t *d_i, int32_t *d_j, int64_t *d_n, int64_t *d_g, int8_t *d_o);

// toppartners.hip: the kernels of reo_top_partners (the cell, the row key, the batch rule and the host checks: top_partners.h).
// launch_top_partners_count: for the n_rows query genes d_genes[0 .. n_rows - 1] (n_rows a multiple of kTpRows, every entry a gene) and
// every column the cell of "query above column" into d_cells ([n_rows][Gp] 64-bit words).  launch_top_partners_select: one workgroup per
// row decides the first m_want partners of rows 0 .. n_rows - 1 from the cells and d_D and stores them into d_partner ([n_rows][m_want]),
// d_counts ([..][4]), d_key ([..][2]) and d_found ([n_rows]); entries beyond a row's n_found are -1 / 0
int32_t launch_top_partners_count(reo_ctx *c, const int32_t *d_gside, int s_a, int s_b, const int32_t *d_genes, int64_t n_rows,
                                  unsigned long long *d_cells);
int32_t launch_top_partners_select(reo_ctx *c, const unsigned long long *d_cells, const int32_t *d_genes, int64_t n_rows, const int64_t *d_D,
                                   const uint32_t *d_maskbits, int s_a, int s_b, int m_want, int32_t *d_partner, int32_t *d_counts, int64_t *d_key,
                                   int32_t *d_found);

// toppartnersnull.hip: the kernel of reo_top_partners_null (the key, the batch rule and the host checks: top_partners_null.h).  For
// permutations 0 .. np - 1 of the words of launch_top_null_words and the n_genes query genes d_genes (padded with gene 0 up to a multiple
// of kTnRows, every entry a gene) the largest key of every (permutation, row) into d_keys (atomicMax) and the partners with |N| >=
// d_cuts[row] into d_reach (atomicAdd; d_cuts null: nothing is counted); both are [np][padded rows] and cleared by the caller; d_cuts:
// [padded rows] words of tprn_cut_word; d_maskbits: [Wp] the partner mask as bits, or null for every gene
int32_t launch_top_partners_null(reo_ctx *c, const uint32_t *d_aw, const uint32_t *d_live, int np, int s_a, int s_b, const int32_t *d_genes,
                                 int64_t n_genes, const uint32_t *d_maskbits, const uint32_t *d_cuts, unsigned long long *d_keys, uint32_t *d_reach);

// maskedpairs.hip: the kernels of reo_set_valid_mask / reo_build_pairs_masked / reo_pair_counts_masked (shared arithmetic and host checks:
// masked_pairs.h).  launch_valid_words: c->vmask and d_slot2col ([32 * sample blocks], -1 for padding) into c->vwords (sized by the
// caller).  launch_pairs_masked: the class table of comparison k from the planes and c->vwords (the caller has cleared the table);
// d_m1 / d_m2: the thresholds m(0 .. n1) / m(0 .. n2) of the two sides.  launch_counts_masked: the rectangle layout of launch_counts, int32
int32_t launch_valid_words(reo_ctx *c, const int32_t *d_slot2col);
int32_t launch_pairs_masked(reo_ctx *c, int k, const int32_t *d_m1, int n1, const int32_t *d_m2, int n2, int min_complete1, int min_complete2);
int32_t launch_counts_masked(reo_ctx *c, int64_t i0, int64_t i1, int64_t j0, int64_t j1, int32_t *d_gt, int32_t *d_eq, int32_t *d_avail);

// permpairs.hip: the kernels of reo_perm_null / reo_perm_codes (shared arithmetic and host checks: perm_null.h).  launch_perm_words: the label
// rows d_side ([n_perm][S] bytes, checked by the caller) and d_slot2col ([32 * sample blocks], -1 for padding) into the A-words d_aw
// (pn_word_count(n_perm, blocks) words, cleared here) and the live words d_live ([blocks]).  launch_pairs_permuted: the class tables of
// permutations 0 .. np - 1 of those words into d_tables ([np][G][4][Wp]; the caller has cleared it once), sides of n1 / n2 samples held to
// m1 / m2.  launch_perm_accumulate: the pass result in c->result against d_obs ([G] observed delta1) into d_n_ge ([G]) and the
// permutation's own d_n_up, d_n_down, d_se ([1] each)
int32_t launch_perm_words(reo_ctx *c, const uint8_t *d_side, int64_t n_perm, const int32_t *d_slot2col, uint32_t *d_aw, uint32_t *d_live);
int32_t launch_pairs_permuted(reo_ctx *c, const uint32_t *d_aw, const uint32_t *d_live, int np, int n1, int n2, int m1, int m2, uint32_t *d_tables);
int32_t launch_perm_accumulate(reo_ctx *c, const double *d_obs, double pval_deg, double padj_deg, int32_t *d_n_ge, int32_t *d_n_up, int32_t *d_n_down,
                               double *d_se);

// pseudobulk.hip: the checks, upload and kernels of reo_pseudobulk_*, the G x n_out sums left in c->dX_owned (ld = G) instead of a host array
int32_t pseudobulk_resident_dense(reo_ctx *c, const void *X, bool is_int, int64_t G, int64_t C, int64_t ld, const int32_t *order,
                                  int64_t n_order, const int32_t *chunk_ptr, int32_t n_out);
int32_t pseudobulk_resident_csc(reo_ctx *c, bool is_int, int64_t G, int64_t C, const int64_t *colptr, const int32_t *rowidx, const void *val,
                                const int32_t *order, int64_t n_order, const int32_t *chunk_ptr, int32_t n_out);
// the cells on the device (reo_set_matrix_pseudobulk_*_dev_*): read where they are; dtype 1 Float64, 2 Int64, 3 Float32, 4 Int32 (summed in Float64 / Int64)
int32_t pseudobulk_device_dense(reo_ctx *c, int dtype, const void *dX, int64_t G, int64_t C, int64_t ld, const int32_t *order, int64_t n_order,
                                const int32_t *chunk_ptr, int32_t n_out);
int32_t pseudobulk_device_csc(reo_ctx *c, int dtype, int64_t G, int64_t C, int64_t nnz, const void *d_colptr, const void *d_rowidx,
                              int32_t index_bits, const void *d_val, const int32_t *order, int64_t n_order, const int32_t *chunk_ptr, int32_t n_out);
// csc_device.hip: arguments and container of a device CSC matrix, checked by a kernel before anything indexes with them (csc_check.h);
// *colptr64: the column pointer as int64 on the device (32-bit ones widened into c->csc_colptr)
int32_t csc_device_check(reo_ctx *c, int64_t G, int64_t S, int64_t nnz, const void *d_colptr, const void *d_rowidx, int32_t index_bits,
                         const void *d_val, const int64_t **colptr64);
// filter.hip: the low-expression filters and the compaction of the resident matrix (reo_filter_matrix; host half: filter_maps.h)
int32_t filter_matrix(reo_ctx *c, int64_t min_profiles, int64_t min_features, uint8_t *profile_kept, uint8_t *gene_kept,
                      int64_t *S_kept, int64_t *G_kept);

// comm.hip: in-library RCCL.  Returns REO_OK after enqueueing the sum on c->stream, 1 when no communicator is attached
int32_t comm_allgather(reo_ctx *c, const void *send, void *recv, int64_t bytes_per_rank, hipStream_t st = nullptr);
void comm_release(reo_ctx *c);
void comm_abort(reo_ctx *c);                     // abort the communicator, mark the context unusable for exchanges
int32_t comm_wait(reo_ctx *c);                   // stream wait that watches the communicator (async errors, time limit)
int32_t multi_build_pairs(reo_ctx *lead, int32_t k, int32_t (*build_local)(reo_ctx *, int32_t));

// timing helpers (api.hip)
void tic(reo_ctx *c, int slot);
void toc(reo_ctx *c);
void collect_timings(reo_ctx *c);

// query prologue (api.hip): what the entry points of queries.hip share with the rest of the C ABI
int32_t use(reo_ctx *c);                               // a context, and its device made current
int32_t no_multi(reo_ctx *c, const char *what);        // `what` refuses a reo_create_multi context
int32_t need_complete_table(reo_ctx *c);               // a class table, and every shard's part of it
int32_t ensure_transform(reo_ctx *c);                  // matrix and groups set and of one size; the bit planes made if they are not in place
int32_t wait_or_drop_table(reo_ctx *c);                // the stream wait of a call that may be the first to see a failed pair kernel
bool mask_in_force(reo_ctx *c);                        // a validity mask is set and has the resident matrix's shape (another shape drops it)
int32_t refuse_under_mask(reo_ctx *c, const char *what);   // `what` compares on the bit planes: refused while a validity mask is set
// The slot -> column map of sc_slot_map (sample_counts.h) into c->sc_slot2col (already sized by the caller), on the stream
int32_t upload_slot2col(reo_ctx *c, const std::vector<int32_t> &map);
// Every call that enqueues an asynchronous copy from or into CALLER memory (or a local) holds one of these: whatever way the call
// ends -- a failing REO_HIP_CHECK between the enqueue and the wait included -- the stream has been waited for before the caller
// gets its arrays back (include/reo_hip.h: "no host pointer is retained after return").  A call that has done its own wait
// dismisses the guard; the extra wait of an error path costs nothing that matters.
struct DrainOnExit {
    reo_ctx *c;
    bool armed = true;
    explicit DrainOnExit(reo_ctx *ctx) : c(ctx) {}
    DrainOnExit(const DrainOnExit &) = delete;
    DrainOnExit &operator=(const DrainOnExit &) = delete;
    void dismiss() { armed = false; }
    ~DrainOnExit()
    {
        if (!armed || !c || !c->stream) return;
        (void)hipStreamSynchronize(c->stream);
    }
};

}  // namespace reo
