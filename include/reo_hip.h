/*
 * reo_hip.h -- C ABI of libreo_hip.so, the MI355X (gfx950) implementation of
 * RankCompV3.jl's REO pairwise-comparison hot path.
 *
 * The reference has no FFI: the seam this library replaces is the ordinary
 * Julia call identify_degs(data, group, gene_names, pval_reo, pval_deg,
 * padj_deg, ref_gene, n_iter, n_conv) at /root/reference/src/RankCompV3.jl:
 * 339-350 (called once from reoa at :652-662).  A <=100-line Julia shim with
 * that exact signature drives the entry points below through ccall (see
 * INTEGRATION.md and julia/RankCompV3HIP.jl); the Python mirror in
 * rankcompv3.jl_amd/ binds the same symbols through ctypes.
 *
 * Conventions
 *   - every function returns 0 on success or a negative reo_status; the
 *     message of the last failure on the calling thread is reo_last_error().
 *     REO_EINVAL corresponds to the reference's DimensionMismatch /
 *     ArgumentError / BoundsError paths (src/RankCompV3.jl:355-356,411).
 *   - the caller owns every array it passes; host inputs are copied during
 *     the call and no host pointer is retained after return; outputs are
 *     caller-allocated.
 *   - a context is single-owner (not thread-safe); distinct contexts may be
 *     used from distinct threads.  Every call blocks until its outputs are in
 *     the caller's arrays and its inputs have been read.  ONE exception:
 *     on one GPU with nothing to exchange reo_build_pairs returns with the
 *     pair kernel still running (see there); all work of a context is ordered
 *     on one stream, so later calls need no synchronisation by the caller, a
 *     host timer around reo_build_pairs alone measures the launch only, and an
 *     asynchronous failure of that kernel is reported (REO_EHIP) by the next
 *     call that waits, which also drops the class table so that a retry
 *     rebuilds it.
 *   - matrices are column-major (the layout Julia hands over at :652).
 */
#ifndef REO_HIP_H
#define REO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct reo_ctx reo_ctx;

enum reo_status {
    REO_OK = 0,
    REO_EINVAL = -1, /* bad argument / shape mismatch / reference error path */
    REO_EHIP = -2,   /* HIP runtime failure (including "no GPU")           */
    REO_ECOMM = -3,  /* RCCL or the all-reduce hook failed / table not exchanged */
    REO_ENOMEM = -4  /* host or device allocation failed                   */
};

/* Library version, major*10000 + minor*100 + patch. */
int32_t reo_version(void);

/* Message of the last error on this thread (library-owned, valid until the
 * next failing call on the same thread). */
const char *reo_last_error(void);

/* Create a context on HIP device `device` (-1 = the current device).  `seed`
 * keys the tie coin stream that stands in for the reference's unseeded
 * rand(Bool) in is_greater (src/RankCompV3.jl:71-77).  Fails with REO_EHIP
 * when no gfx950 device is usable: there is no CPU fallback. */
int32_t reo_create(reo_ctx **out, int32_t device, uint64_t seed);
void reo_destroy(reo_ctx *ctx);

/* Memory of destroyed contexts is kept for the next one: a caller that makes a context per identify_degs call (the Julia shim
 * does) would otherwise spend as long in hipMalloc / hipFree as in the computation (6 of 14 ms at 20 000 x 1 000).  Released
 * device and pinned-host blocks wait in a process-wide cache, at most REO_DEVICE_CACHE_MB megabytes of them (environment,
 * default 16384; 0 = no cache, every release is a hipFree), and so do the streams and events of destroyed contexts;
 * reo_trim_memory() returns all of it to the driver now. */
int32_t reo_trim_memory(void);

/* ---- several GPUs ---------------------------------------------------------------------------------------
 * The reference is one process with shared-memory threads (src/RankCompV3.jl:368,402) and has no multi-device
 * path; this is the build's own.  The pair tiles of the G x G triangle are dealt to `world` shards; every shard
 * builds the class-table words of its tiles, ONE exchange per class table (the shards' bits are disjoint: an
 * all-gather of their own words, or an in-place sum) gives every shard the whole table, and the iteration passes
 * run with no further collective.
 *
 * (a) one process, all GPUs: reo_create_multi(&ctx, n_gpus (0 = all visible), seed) returns a context that is
 *     used exactly like a one-GPU context; it drives one device context each; inside reo_build_pairs the peers pack
 *     the table words of their own pair tiles and hand them to device 0 (grouped ncclSend / ncclRecv), which unpacks
 *     them, derives the mirror words and runs the passes.  This form is NOT pipelined (the hand-over starts when every
 *     device has finished its tiles) and the passes run on the leader only: for throughput use (b).  NOT yet run on more than one GPU (no such box in this
 *     project's pool): the orchestration is tested with the shards sharing one device (REO_MULTI_ONE_DEVICE=1).
 * (b) one process per GPU: rank 0 calls reo_comm_unique_id and hands the 128 bytes to the other ranks by any
 *     means; every rank calls reo_comm_init_rank(ctx, id, rank, world) (ncclCommInitRank + reo_set_shard).
 *     reo_build_pairs then ends with an ncclAllGather of the shards' own table words on the context's stream (see
 *     reo_set_allgather for the protocol); all ranks get identical results.  A rank that fails inside reo_build_pairs
 *     aborts its communicator (ncclCommAbort) so that its peers' collective ends with REO_ECOMM instead of waiting;
 *     the wait itself watches ncclCommGetAsyncError and gives up after REO_COMM_TIMEOUT_S seconds (default 300).  After
 *     such a failure the context needs a new communicator.  NOT yet run with more than one rank on hardware.
 * (c) bring your own collective: reo_set_shard + reo_set_allgather or reo_set_allreduce (hooks below).  */
enum { REO_UNIQUE_ID_BYTES = 128 };
int32_t reo_create_multi(reo_ctx **out, int32_t n_gpus, uint64_t seed);
int32_t reo_comm_unique_id(void *id /* REO_UNIQUE_ID_BYTES */);
int32_t reo_comm_init_rank(reo_ctx *ctx, const void *id, int32_t rank, int32_t world);

/* This context builds only the pair tiles it owns out of `world` shards.  Default (0, 1) = everything.
 * With world > 1 and neither a communicator nor a hook attached, reo_build_pairs leaves the shard's own part
 * of the table (reo_get_codes shows it; pairs of other shards read as class 4) and reo_tally /
 * reo_identify_degs refuse with REO_ECOMM. */
int32_t reo_set_shard(reo_ctx *ctx, int32_t rank, int32_t world);

/* Hook called once per reo_build_pairs when world > 1 and no communicator is attached: it must arrange for
 * `count` int32 values at device pointer `dev_buf` (the class table) to be summed in place across all shards,
 * ORDERED ON `stream` (a hipStream_t): everything the library enqueued on `stream` before the call has to
 * precede the sum, and the sum has to precede whatever is enqueued on `stream` afterwards.  A hook that enqueues
 * the collective on `stream` (RCCL ncclAllReduce(..., stream), or torch.distributed.all_reduce under
 * torch.cuda.stream(ExternalStream(stream))) needs no host synchronisation; a hook that works on the host must
 * synchronise `stream` itself before and after.  Return 0 on success.  A hook that fails must abort its own
 * communicator: the library cannot release peers that wait inside a caller's collective.  The table a hook delivers is
 * scanned for consistency (a pair in two states, bits outside the table: REO_ECOMM). */
typedef int32_t (*reo_allreduce_fn)(void *dev_buf, int64_t count, void *stream, void *user);
int32_t reo_set_allreduce(reo_ctx *ctx, reo_allreduce_fn fn, void *user);

/* The cheaper form of the same exchange, and what the in-library RCCL path does: every shard packs the table words of
 * ITS OWN pair tiles (upper triangle only, about a quarter of what an in-place sum of the whole table moves), the
 * packs are gathered, and every shard unpacks the others' words and derives the mirror words (the pair seen from the
 * other gene, src/RankCompV3.jl:386) itself.  The hook is an all-gather: `bytes_per_rank` bytes at device pointer
 * `send` of every shard have to arrive at `recv + r * bytes_per_rank` of every shard, r = the sender's shard number,
 * ordered on `stream` like the sum above (RCCL: ncclAllGather(send, recv, bytes_per_rank, ncclUint8, comm, stream)).
 * When both hooks are set this one is used.
 * CALLED SEVERAL TIMES PER BUILD, ON ANOTHER STREAM: with two groups the shard's pair tiles are counted in up to 8 waves
 * (REO_EXCHANGE_WAVES, default 4) and the hook is called once per wave -- `bytes_per_rank` differs from call to call but is the
 * same on every shard for the same call -- with `stream` = the context's EXCHANGE stream, not the stream of other calls; the
 * ordering rule above holds per call, on the stream that call names.  Every shard must make the same number of calls: the
 * number of waves follows from REO_EXCHANGE_WAVES / REO_K1_STAMPS / REO_K1_WAVE in the environment, which must therefore be
 * equal on all shards (the in-library communicator checks that in reo_comm_init_rank and answers REO_EINVAL; with a caller's
 * hook the caller has to see to it).  REO_EXCHANGE_WAVES=1: one call per build, on the context's own stream. */
typedef int32_t (*reo_allgather_fn)(const void *send, void *recv, int64_t bytes_per_rank, void *stream, void *user);
int32_t reo_set_allgather(reo_ctx *ctx, reo_allgather_fn fn, void *user);

/* Expression matrix, G genes x S samples, column-major with leading dimension
 * ld >= G: the `data` argument of identify_degs (src/RankCompV3.jl:340) as
 * Matrix(df_expr) produces it (:652), eltype Float64, Int64, Float32 or Int32.  G must be in [2, 262143] and S in [2, 1048576];
 * with more than two groups G and S may not both exceed 65535; values must be finite.  reo_set_matrix_f64 / _i64 /
 * _f32 / _i32 copy from host memory (pageable is fine) and have read all of it when they return; *_dev uses a buffer already resident in HBM (it
 * must stay valid until reo_build_pairs returns).
 * ORDER OF CALLS.  Any order of reo_set_matrix_*, reo_set_groups, reo_compute_thresholds works.  From HOST memory the cheap order is
 * groups and thresholds FIRST, the matrix last: the call then uploads the columns in chunks and pipelines them with the rest of
 * the work -- the samples of a chunk are ranked while the next chunk is crossing PCIe, and with two groups on one GPU the pair
 * kernel's items of a group (its "side" of every pair) are counted over ranges of that group's 32-sample blocks as its chunks arrive
 * (their 16-bit counts wait in device memory for the group's last range, which classifies), while the rest is still on its way.  The call still returns only when the whole matrix has been read (no host pointer is retained); the pair
 * kernel may be running then, exactly as after reo_build_pairs on one GPU, and the reo_build_pairs(ctx, 0) that follows has nothing
 * left to do (it is still the call that makes the class table current: keep it).  Results are bit-identical in every order.
 * VALUES.  +-Inf are accepted and compared as the reference's is_greater compares them (src/RankCompV3.jl:71-77): equal infinities
 * are neither tied nor greater (abs(Inf - Inf) = NaN is not < 0.1, Inf > Inf is false -- the pair (i, j), i < j, counts as "i not
 * greater" in that sample, no coin), an infinity against any other value compares as usual; log(0) = -Inf tables run unchanged.
 * A NaN is refused (REO_EINVAL, by whichever call reads the matrix: this one in the pipelined case): every comparison with a NaN
 * is false, which makes a NaN gene below every later and above every earlier gene -- row order, not an ordering.
 * A context that is used for several matrices should keep to that order each time: a matrix handed over while the groups of the LAST
 * problem are still set is ranked and paired with those, and all of it is done again when the new groups arrive (correct, but wasted).
 * REO_EAGER_UPLOAD=0 in the environment switches the pipelining off, =1 keeps it to the ranking.
 * ELEMENT TYPES.  A matrix is compared in the arithmetic of its own element type, as the reference's is_greater compares a
 * Matrix of that type.  FLOAT32 RULE: x and y are tied iff (double)fabsf(x - y) < 0.1 -- the difference is formed and rounded (to
 * nearest, subnormals kept) in Float32 and then compared with the Float64 literal 0.1; equivalently fabsf(x - y) <= 0x1.999998p-4f.
 * Float32(0.1) = 0.100000001... is not below 0.1, so a pair whose exact difference lies in [0.09999999776, 0.1) and rounds up to
 * Float32(0.1) is NOT tied, where the same values widened to Float64 would be; wherever x - y is exact in Float32 (every pair within a
 * factor two of each other) the two agree.  A caller who wants the Float64 rule widens the matrix and calls _f64.  The Float32 matrix
 * is ranked from a resident Float32 copy (4 bytes per value on the link and in HBM); no Float64 copy is made.  Int32 has Int64's rule
 * (a tie is equality): _i32 sends the 4-byte values over the link and widens them on the device into the context's own Int64 matrix,
 * _dev_i32 widens once on the context's stream (the caller's buffer has been read when it returns); results are bit-identical to
 * _i64 on the same values.  REO_TRANSFORM=segmented (the A/B build) is refused for these two types.
 * LAYOUT.  reo_set_matrix_rm_f64 / _i64 / _f32 / _i32 take the same matrix ROW-MAJOR from host memory (pageable is fine): the value of
 * gene g in sample s is X[g * ld + s], ld >= S (REO_EINVAL otherwise) -- a C-ordered numpy array, a genes x cells HDF5 dataset, a
 * column slice of a wider one.  The array is read IN PLACE, no transposed host copy is made: a chunk of sample columns is G row
 * segments, which the host threads narrow (or pack) into a staging slot as they are, and the transposition into the context's own
 * column-major matrix is fused with the widening kernel on the device.  Limits, ownership (all of it has been read on return, no host
 * pointer is kept), the NaN refusal, the +-Inf rule, the element-type rules and both upload paths (pipelined with the groups set first,
 * plain otherwise) are those of the column-major entries, and every result is BIT-IDENTICAL to reo_set_matrix_* on the transposed copy,
 * in every order of calls; chunk by chunk the link carries the same bytes (reo_get_info 19).  REO_ROWMAJOR_COPY=2d in the environment
 * sends chunks that are not narrowed as one 2-D copy from the caller's array instead of packing them through pinned memory (A/B;
 * REO_UPLOAD_THREADS=0 always does).  reo_get_info 21 says which layout the last host matrix had.
 *
 * SPARSE.  reo_set_matrix_csc_f64 / _i64 / _f32 / _i32 take the same matrix from host memory in compressed sparse column form (single-cell
 * counts are 90-95 % zeros; a scipy.sparse csc_matrix is this container as it is), arguments in the order of reo_pseudobulk_csc_*:
 * colptr has S + 1 entries, colptr[0] = 0, non-decreasing, colptr[S] = nnz; rowidx and val have nnz entries, row indices 0-based and
 * STRICTLY INCREASING inside a column (sorted, no duplicates).  A row index outside [0, G), an unsorted or repeated one and a colptr
 * that is not such a pointer are REO_EINVAL (the context then holds no matrix until the next reo_set_matrix_*; it stays usable).
 * Explicitly stored zeros are fine, a stored -0.0 stays -0.0, an absent entry is +0 of the element type; nnz = 0 is an all-zero matrix,
 * and rowidx / val may then be null.  The zeros never exist on the host or on the link: a chunk of columns is the entry range
 * colptr[c0] .. colptr[c0 + nc], which the host threads check and narrow -- row indices to 16 bits when G <= 65 536, Int64 and Float64
 * values as the dense entries narrow theirs, Float32 / Int32 values as they are (REO_UPLOAD_THREADS=0: the calling thread checks, the
 * arrays go as they are) -- and a kernel writes the chunk's columns of the context's own column-major matrix, each element once.
 * Limits, ownership (everything has been read on return, no host pointer is kept), the NaN refusal, the +-Inf rule, the element-type
 * rules and both upload paths are those of the dense entries, and every result is BIT-IDENTICAL to reo_set_matrix_<type> on the
 * densified array, in every order of calls.  reo_get_info 19 counts what this upload sent (colptr included), 22 says that the last host
 * matrix came as CSC, 23 its nnz.
 *
 * CELLS.  reo_set_matrix_pseudobulk_csc_f64 / _csc_i64 / _dense_f64 / _dense_i64 (declared beside reo_pseudobulk_* below) make the pseudo-bulk
 * profiles of a cell matrix the expression matrix without a trip through host memory, and reo_filter_matrix applies the reference's two
 * low-expression filters (src/RankCompV3.jl:618, :626) to whatever matrix the context holds and compacts it in HBM.
 * ORDER OF CALLS with them: matrix (any entry), then reo_filter_matrix, then reo_set_groups for the profiles that are LEFT, thresholds,
 * reo_build_pairs.  The filter always invalidates what was derived from the matrix; groups of the old length then fail with the
 * DimensionMismatch message until new ones are set.  A matrix that the pipelined upload has already ranked (groups set first, host
 * entry) is ranked again after filtering: correct, but wasted -- filter first. */
int32_t reo_set_matrix_f64(reo_ctx *ctx, const double *X, int64_t G, int64_t S, int64_t ld);
int32_t reo_set_matrix_i64(reo_ctx *ctx, const int64_t *X, int64_t G, int64_t S, int64_t ld);
int32_t reo_set_matrix_dev_f64(reo_ctx *ctx, const void *dX, int64_t G, int64_t S, int64_t ld);
int32_t reo_set_matrix_dev_i64(reo_ctx *ctx, const void *dX, int64_t G, int64_t S, int64_t ld);
int32_t reo_set_matrix_f32(reo_ctx *ctx, const float *X, int64_t G, int64_t S, int64_t ld);
int32_t reo_set_matrix_i32(reo_ctx *ctx, const int32_t *X, int64_t G, int64_t S, int64_t ld);
int32_t reo_set_matrix_dev_f32(reo_ctx *ctx, const void *dX, int64_t G, int64_t S, int64_t ld);
int32_t reo_set_matrix_dev_i32(reo_ctx *ctx, const void *dX, int64_t G, int64_t S, int64_t ld);
int32_t reo_set_matrix_rm_f64(reo_ctx *ctx, const double *X, int64_t G, int64_t S, int64_t ld);
int32_t reo_set_matrix_rm_i64(reo_ctx *ctx, const int64_t *X, int64_t G, int64_t S, int64_t ld);
int32_t reo_set_matrix_rm_f32(reo_ctx *ctx, const float *X, int64_t G, int64_t S, int64_t ld);
int32_t reo_set_matrix_rm_i32(reo_ctx *ctx, const int32_t *X, int64_t G, int64_t S, int64_t ld);
int32_t reo_set_matrix_csc_f64(reo_ctx *ctx, int64_t G, int64_t S, const int64_t *colptr, const int32_t *rowidx, const double *val);
int32_t reo_set_matrix_csc_i64(reo_ctx *ctx, int64_t G, int64_t S, const int64_t *colptr, const int32_t *rowidx, const int64_t *val);
int32_t reo_set_matrix_csc_f32(reo_ctx *ctx, int64_t G, int64_t S, const int64_t *colptr, const int32_t *rowidx, const float *val);
int32_t reo_set_matrix_csc_i32(reo_ctx *ctx, int64_t G, int64_t S, const int64_t *colptr, const int32_t *rowidx, const int32_t *val);

/* Group of each sample: the `group` argument (src/RankCompV3.jl:341) recoded
 * to 0-based ids in order of first appearance (unique(), :353).  Length must
 * equal S (else REO_EINVAL = the DimensionMismatch of :355); ngroups must be
 * >= 2 (:356); any number of levels that the samples allow. */
int32_t reo_set_groups(reo_ctx *ctx, const int32_t *group_id, int64_t len, int32_t ngroups);

/* Stable-REO thresholds: get_major_reo_lower_count (src/RankCompV3.jl:81-92)
 * applied as at :362.  m is 2 x ngroups column-major: m[2k] for group k,
 * m[2k+1] for the rest.  reo_compute_thresholds derives them from pval_reo,
 * reo_set_thresholds overrides them, reo_get_thresholds reads them back. */
int32_t reo_compute_thresholds(reo_ctx *ctx, double pval_reo);
int32_t reo_set_thresholds(reo_ctx *ctx, const int32_t *m);
int32_t reo_get_thresholds(reo_ctx *ctx, int32_t *m);
/* The threshold function itself (host arithmetic), for tests. */
int32_t reo_threshold(int32_t sample_size, double pval_reo);

/* REO table build for comparison k (group k vs every other sample; with two
 * groups the reference only runs k = 0, :387-389): replaces the pair loop
 * src/RankCompV3.jl:363-392.  Runs the per-sample rank/band transform and the
 * pair-compare kernel and leaves the 4-bit class table in HBM.  The input matrix has been read when the call
 * returns.  On one GPU with nothing to exchange the pair kernel may still be running then: every later call on the
 * context is ordered behind it (one stream), and an asynchronous failure of the kernel is reported by the next call
 * that waits (REO_EHIP).  With shards (several GPUs, hooks) the call returns after the exchange has finished. */
int32_t reo_build_pairs(reo_ctx *ctx, int32_t k);

/* Pairwise contrast: the class table of "group ctrl (c-side) against group treat (t-side)"; samples of every other group take no part.
 * With more than two groups reo_build_pairs answers "group k against every other sample"; a design with a control and several treatments
 * asks for treatment against control and treatment against treatment, and this call answers those from what the one-vs-rest comparisons
 * already keep: the per-group counts nre_g(i, j) of every ordered pair (reo_get_info 12, 13), tie coins included.  Nothing is counted again
 * -- the first build of a context counts every group once, whichever call it is, and each contrast is one table-sized classification.
 * For the unordered pair i < j and group g: nre_g = n_gt_g(i, j) + tie_wins(seed, i, j, g, n_eq_g(i, j)), the coin keyed by the group's own
 * id in reo_set_groups order (not by its side); ic = nre_ctrl >= m1 ? 3 : (S_ctrl - nre_ctrl >= m1 ? 1 : 2), `it` likewise from nre_treat,
 * S_treat, m2; the code is 3 (ic - 1) + (it - 1) and the ordered pair (j, i) gets 8 - code.  m1 = thr[0, ctrl] and m2 = thr[0, treat]: row 0
 * of reo_get_thresholds, each group's own size (row 1 is not used; values from reo_set_thresholds are read from the same places).  On
 * tie-free data the table equals, code for code, the reo_build_pairs table of a context that holds only the two groups' columns with ctrl
 * as its control; with ties that holds when the two group ids are 0 and 1 (the coin keys then coincide).
 * Everything behind the table -- reo_tally, reo_identify_degs, reo_get_ref_mask, reo_pair_list, reo_sample_counts, reo_pair_support,
 * reo_sample_tests (ctrl is its control group) -- works on it as on any other; reo_get_info 29 reports the treat group.  Two groups:
 * (0, 1) is reo_build_pairs(ctx, 0) and (1, 0) is reo_build_pairs(ctx, 1).  Sharded contexts (reo_set_shard with a communicator or a hook) classify their own units and exchange as
 * reo_build_pairs does.  Returns and waits as reo_build_pairs.
 * Refused with REO_EINVAL, before anything of the context is touched (the resident table and the reference mask survive): a null context;
 * ctrl or treat outside [0, ngroups); ctrl == treat; thresholds not set; a reo_create_multi context; and, with more than two groups, no
 * shared count planes -- more than 65535 samples, REO_SHARE_GROUP_COUNTS=0 in the environment, or planes that do not fit the free device
 * memory (the message gives the bytes needed).  There is no fallback that recounts. */
int32_t reo_build_pairs_contrast(reo_ctx *ctx, int32_t ctrl, int32_t treat);

/* Parity hook: deterministic per-pair per-group counts for the ordered pairs
 * (i, j), i in [i0,i1), j in [j0,j1): n_gt = #samples with x_i > x_j and not
 * tied, n_eq = #tied samples (|x_i - x_j| < 0.1, src/RankCompV3.jl:72), each
 * laid out [(i-i0)][(j-j0)][group].  Computed from the same bit planes with the
 * same borrow chain as reo_build_pairs.  Needs matrix + groups only. */
int32_t reo_pair_counts(reo_ctx *ctx, int64_t i0, int64_t i1, int64_t j0, int64_t j1,
                        uint16_t *n_gt, uint16_t *n_eq);

/* Parity hook: class codes 3*(ic-1)+(it-1) in 0..8 of the ordered pairs of a
 * block (255 on the diagonal, which the table never sets; pairs owned by
 * another shard read as class 4 = all four bits clear), row-major [(i-i0)][(j-j0)] -- the column index of the
 * reference's R BitArray minus one (src/RankCompV3.jl:383-386). */
int32_t reo_get_codes(reo_ctx *ctx, int64_t i0, int64_t i1, int64_t j0, int64_t j1, uint8_t *code);

/* Per-gene 3x3 contingency builder, src/RankCompV3.jl:403: cont is G x 9
 * row-major (n11 n12 n13 n21 ... n33), ref_mask has one byte per gene
 * (non-zero = reference gene).  Needs the complete class table: with world > 1 and no exchange done by
 * reo_build_pairs (communicator or hook) it refuses with REO_ECOMM. */
int32_t reo_tally(reo_ctx *ctx, const uint8_t *ref_mask, int32_t *cont);

/* Iteration driver + McCullagh test, src/RankCompV3.jl:396-425 (and :225-259)
 * for the comparison built by reo_build_pairs.  result is G x 15 column-major
 * Float64: [pval padj n11..n33 delta1 delta2 se z1] (:398,405,415-416,665).
 * iters_run = number of executed passes of the while loop (:400); trace is
 * n_iter x 2 int32, (#DEG, #non-DEG) per pass (the :418 log line); either may
 * be NULL.  REO_EINVAL when the reference would throw (G < 10: the slice of
 * :411 is out of bounds).
 * A loop that does not converge repeats itself sooner or later: a pass depends on its reference set alone, so once the set in
 * front of a pass equals an earlier one (checked exactly, bit for bit) the remaining passes are the last period over and over.
 * The call then skips whole periods and executes only the remainder -- iters_run, trace and result are what n_iter executed
 * passes give (reo_get_info 16-18 says what happened; REO_CYCLE=0 in the environment executes every pass). */
int32_t reo_identify_degs(reo_ctx *ctx, const uint8_t *ref0, double pval_deg, double padj_deg,
                          int32_t n_iter, int32_t n_conv, double *result,
                          int32_t *iters_run, int32_t *trace);

/* The reference set behind the returned tallies.  ref_mask (G bytes, 0 / 1) receives the mask over which the last reo_identify_degs on the
 * current class table counted the n11 .. n33 it returned -- ref_gene_vec of its last executed pass (src/RankCompV3.jl:399-424): ref0 when one
 * pass ran, otherwise the `inds` of the pass before the last -- and *nref (may be NULL) its number of genes.  The labels of `result` do NOT
 * give this set: they are the last pass's own `inds`, the set a further pass would have used.  The rule holds however the loop ended
 * (converged, n_iter exhausted on either kind of pass, whole periods skipped by the cycle watch); reo_tally(ctx, ref_mask) reproduces
 * result[:, 2:11] exactly.  The mask is read where the passes left it: reo_identify_degs does no extra work for it.
 * REO_EINVAL, with a message that says why, when there is no such mask or it is out of date: before any reo_identify_degs, after a failed
 * one or one with n_iter <= 0, and after reo_tally (it uploads its own mask into the iteration's buffers), reo_build_pairs, any
 * reo_set_matrix_*, reo_filter_matrix, reo_set_groups, reo_set_shard or a change of the thresholds.  A wrong mask is never delivered. */
int32_t reo_get_ref_mask(reo_ctx *ctx, uint8_t *ref_mask /* G bytes, 0 / 1 */, int32_t *nref /* may be NULL */);

/* Pair lists: WHICH partner genes make up a gene's tallies.  The reference has no such output (its R BitArray dies inside identify_degs,
 * src/RankCompV3.jl:363-392); the class table of reo_build_pairs holds every pair, and this call extracts rows of it on the device.
 * For query q, gene i = genes[q] (any order, repeats allowed, each entry is its own row), partner[rowptr[q] .. rowptr[q+1]) lists in ascending
 * order every gene j != i with partner_mask[j] != 0 whose ordered pair (i, j), seen from gene i, has a selected class, and code[...] holds that
 * class: 3*(ic-1)+(it-1) in 0..8, what reo_get_codes returns, the position of the pair's tally among n11 .. n33.  class_mask bit c selects
 * class c (0x1 .. 0x1FF; n13 | n31, the reversed pairs, is 0x44).  partner_mask NULL = the mask of reo_get_ref_mask, read where it lies;
 * row q then has result[i, 2 + c] entries of class c (the diagonal contributes nothing, as in :403).
 * rowptr has n_genes + 1 entries (64-bit), partner and code `capacity` entries.  partner == NULL (then code is NULL and capacity 0): count
 * only, rowptr is still filled -- call once to size the arrays, once to fill them.  With arrays and rowptr[n_genes] > capacity: REO_EINVAL,
 * the message names the needed total, rowptr is delivered and nothing is written to partner / code.
 * Two kernels on the context's stream, one wave per query row (csrc/pairlist.hip): a count pass, whose n_genes counts visit the host for
 * the prefix sums, and a fill pass; device temporaries are sized from the counted total.  Should the two passes ever disagree about a row,
 * nothing is written outside that row's range and the call answers REO_EHIP.
 * Host arrays only; totals above 2^31 entries have not been run (the offsets are 64-bit).
 * REO_EINVAL, each with its own message: no class table; a NULL genes or rowptr; n_genes < 1 (or above 2^30); a gene outside [0, G); a class_mask of 0 or with
 * bits above 8; partner without code (or the reverse) or a negative capacity; a NULL partner_mask while reo_get_ref_mask would refuse; a
 * reo_create_multi context.  An incomplete sharded table: REO_ECOMM, as reo_tally. */
int32_t reo_pair_list(reo_ctx *ctx, const int32_t *genes, int64_t n_genes,
                      const uint8_t *partner_mask /* G bytes; NULL = the mask of reo_get_ref_mask */,
                      uint32_t class_mask /* bit c selects class code c = 3*(ic-1)+(it-1), c in 0..8; 1..0x1FF */,
                      int64_t *rowptr /* n_genes + 1 */, int32_t *partner, uint8_t *code, int64_t capacity);

/* Sample counts: IN WHICH SAMPLES a gene's selected pairs put it above its partner.  The tallies say that gene i's order against the
 * reference genes reversed between the groups, the pair lists say against which genes; this call says in which samples.  The reference has
 * no such output (its R BitArray dies inside identify_degs, src/RankCompV3.jl:363-392).
 * For query q, gene i = genes[q] (any order, repeats allowed, each entry is its own row), J is exactly the partner set that reo_pair_list
 * lists for the same partner_mask / class_mask: j != i, partner_mask[j] != 0 (NULL = the mask of reo_get_ref_mask, read where it lies), the
 * class of the ordered pair (i, j) selected.  n_sel[q] = |J|, and for every sample s in the CALLER's column order -- both groups, every
 * group of a multi-group problem --
 *     n_gt[q * S + s] = #{j in J : x_i > x_j and not tied in sample s}        n_eq[q * S + s] = #{j in J : tied in sample s}
 * by the comparator of the resident matrix's element type as the rank/band transform encodes it: Float64 the 0.1 band, Float32 the Float32
 * rule above, Int64 and Int32 equality; of two equal infinities the gene with the larger index is the greater one and nothing is tied.
 * n_lt = n_sel - n_gt - n_eq is not delivered.  No tie coin is drawn: like reo_pair_counts, the call reports ties as ties.
 * n_eq == NULL: the tied counts are not computed (half of the compare work).
 * Needs the class table (reo_build_pairs) and the transform; reads the reference mask and changes nothing: reo_get_ref_mask and a following
 * reo_identify_degs behave as if the call had not happened.  Both plane layouts (up to and above 65 535 genes), every S.
 * One kernel (csrc/samplecounts.hip): a workgroup per (query, 8 blocks of 32 sample slots) compacts the selected columns of the query's
 * table row tile by tile, runs the borrow chain of the pair kernel against every listed partner and adds the 32-sample result words into
 * bit-sliced counters.  Device temporaries are bounded: the queries go in batches whose two count buffers, each batch x padded sample slots
 * x 4 bytes, stay under 32 MiB each (at least one query per batch); REO_SAMPLE_COUNTS_BATCH in the environment, read per call, lowers the
 * batch to that many queries (tests of the batch seam).
 * Host arrays only; no stage timer of its own.
 * REO_EINVAL, each with its own message: no class table; a NULL genes or n_gt; n_genes < 1 or above 2^30; a gene outside [0, G); a
 * class_mask of 0 or with bits above 8; a NULL partner_mask while reo_get_ref_mask would refuse (its reason is passed on); a
 * reo_create_multi context.  An incomplete sharded table: REO_ECOMM, as reo_tally. */
int32_t reo_sample_counts(reo_ctx *ctx, const int32_t *genes, int64_t n_genes,
                          const uint8_t *partner_mask /* G bytes; NULL = the mask of reo_get_ref_mask */,
                          uint32_t class_mask /* as reo_pair_list: 1 .. 0x1FF */,
                          int32_t *n_sel /* n_genes; may be NULL */,
                          int32_t *n_gt, int32_t *n_eq /* n_genes x S row-major, ld = S; n_eq may be NULL */);

/* Pair support: HOW STRONGLY a listed pair supports a call.  The tallies say that gene i's order against the reference genes reversed, the
 * pair lists say against which genes, the sample counts in which samples summed over the partners; this call says, for every single listed
 * pair, in how many samples of each group gene i lies above its partner -- "above it in 498 of 500 control samples and in 3 of 500 treated
 * ones" -- and, on request, the outcome in every sample.  The reference has no such output.
 * The pairs come as a CSR, exactly what reo_pair_list delivers (a caller may as well hand in pairs of its own, a published signature):
 * for entry e of row q, i = genes[q] (any order, repeats allowed), j = partner[e] (any order, repeats allowed, never i), rowptr[0] = 0,
 * rowptr[n_genes] entries in all; empty rows are fine, and a list without entries returns REO_OK without a launch.  For every group g of
 * reo_set_groups
 *     n_gt[e * ngroups + g] = #{samples of g : x_i > x_j and not tied}        n_eq[e * ngroups + g] = #{samples of g : tied}
 * the values and the per-pair layout of reo_pair_counts widened to int32 (no limit of 65 535 samples), by the comparator of the resident
 * matrix's element type as the rank/band transform encodes it: Float64 the 0.1 band, Float32 the Float32 rule above, Int64 and Int32
 * equality; of two equal infinities the gene with the larger index is the greater one and nothing is tied.  No tie coin is drawn: ties are
 * reported as ties.  n_eq == NULL: the tied counts are not computed (without `outcome`, half of the compare work).
 * outcome (may be NULL): outcome[e * S + s] = 0 (x_i < x_j), 1 (tied), 2 (x_i > x_j) for sample s in the CALLER's column order.
 * Needs the matrix, the groups and the transform (run here if need be, as by reo_pair_counts); needs no class table, no thresholds and no
 * reference mask, reads none of the iteration's buffers and writes none: reo_get_ref_mask and a following reo_identify_degs behave as if
 * the call had not happened.  Both plane layouts (up to and above 65 535 genes), every S.
 * One kernel (csrc/pairsupport.hip): the host cuts every row into work items of at most 64 consecutive entries, one wave per item and one
 * lane per entry; the wave walks the groups' blocks of 32 sample slots with the band edges of gene i wave-uniform, every lane runs the borrow
 * chain of the pair kernel against its own partner and adds the popcounts.  The outcome bytes are stored lane by lane, not coalesced:
 * meant for signatures of hundreds of pairs.  Device temporaries are bounded and sized from the list: the entries go in batches whose two
 * count buffers (batch x ngroups x 4 bytes) and outcome buffer (batch x S bytes) stay under 32 MiB each (at least one entry per batch);
 * REO_PAIR_SUPPORT_BATCH in the environment, read per call, lowers the batch to that many entries (tests of the batch seam).
 * Host arrays only; no stage timer of its own.
 * REO_EINVAL, each with its own message that names reo_pair_support, all checked on the host before anything is uploaded, and a refused
 * call writes nothing: a NULL genes, rowptr or n_gt; n_genes < 1 or above 2^30; a gene outside [0, G); rowptr[0] != 0 or a decreasing
 * rowptr; a NULL partner with rowptr[n_genes] > 0; a partner outside [0, G); a partner that equals its row's gene (the diagonal is no
 * pair, reo_pair_list never lists it); a reo_create_multi context. */
int32_t reo_pair_support(reo_ctx *ctx, const int32_t *genes, int64_t n_genes,
                         const int64_t *rowptr /* n_genes + 1 */, const int32_t *partner /* rowptr[n_genes] */,
                         int32_t *n_gt, int32_t *n_eq /* entries x ngroups, row-major; n_eq may be NULL */,
                         uint8_t *outcome /* entries x S, row-major, caller's column order; may be NULL */);

/* Top-scoring pairs: WHICH few gene pairs, out of all G (G - 1) / 2, separate two sides best?  Every other read-out starts from a gene that
 * the tallies already call; this one is the search of Geman's top-scoring pair and of Tan's k-TSP: it finds the two-gene signature that
 * reo_pair_support takes as input.  The reference has no such output.
 * Sides: A = the samples of group a, B = those of group b, or, with b = -1, every sample not in a (the two sides of reo_build_pairs with
 * k = a); S_A and S_B their sizes.  Per pair and side, by the comparator of the resident element type exactly as reo_pair_support counts:
 * gt = samples with x_i above x_j and not tied, eq = tied samples, lt = S_side - gt - eq; no tie coin is drawn.
 *     w(side) = gt - lt        N_ij = w(A) S_B - w(B) S_A   (int64, antisymmetric)        score = |N| / (2 S_A S_B)  in [0, 1]
 * On tie-free data the score is |gt_A / S_A - gt_B / S_B|, Geman's Delta; in general N / (S_A S_B) = 2 delta + eq_A / S_A - eq_B / S_B with
 * delta = gt_A / S_A - gt_B / S_B: ties count half to each side.  Equal |N| are ordered by the rank shift, as TSP does: per gene
 *     W_i(side) = sum over the side's samples of (genes that i lies above, untied) - (genes that i lies below, untied)
 *     D_i = W_i(A) S_B - W_i(B) S_A        Gamma_ij = |D_i - D_j|        (tie-free: Gamma / (2 S_A S_B) is Tan's gamma)
 * reo_rank_shift delivers D (G values, host).  The order over the unordered pairs i < j with both genes inside gene_mask (NULL: all
 * genes): |N| descending, then Gamma descending, then i ascending, then j ascending -- a total order -- and reo_top_pairs returns its first
 * n_want elements in that order: gene_i < gene_j, counts[4 e ..] = gt_A, eq_A, gt_B, eq_B of "gene_i above gene_j", key[2 e] = N (signed),
 * key[2 e + 1] = Gamma, *n_found = min(n_want, eligible pairs).  The result does not depend on the launch geometry, on the arrival order of
 * atomics or on the candidate capacity.  With G, S <= 65535: |N| < 2^31, |D| <= 2^47, Gamma <= 2^48.
 * Needs the matrix, the groups and the transform (run here if need be); no class table, no thresholds, no reference set.  Reads and writes
 * none of the iteration's buffers: the resident table, reo_get_ref_mask and a following reo_identify_degs behave as if the call had not
 * happened.  Host arrays only, allocated by the caller; no stage timer of its own.
 * Selection without a score per pair (csrc/toppairs.hip, csrc/top_pairs.h): the key (|N|, Gamma, 2^32 - 1 - (i G + j)) is one number of
 * 111 bits; a radix select over its 12-bit digits RECOUNTS all pairs in every pass -- the pair kernel's O(G^2 S) work on the resident bit
 * planes, histogrammed per workgroup in LDS --, the host reads 4098 counters back, picks the bin of the n_want-th key and extends the prefix,
 * skipping the digits that 2 S_A S_B and max D - min D prove zero.  As soon as the keys above the prefix and those that share it fit the
 * candidate buffer -- max(4 n_want, 2^18) records; REO_TOP_PAIRS_CAP in the environment, read per call, lowers it, never below n_want
 * (tests of deep refinement) -- one emit pass appends them and the host sorts by the full key.  *passes_run (may be NULL) = histogram
 * passes; reo_get_info 36 and 37 = microseconds of the histogram passes and of the emit pass of the last call (HIP events).  Device
 * temporaries: the histogram, D, the mask bits, the candidates; nothing scales with G^2.
 * REO_EINVAL, each with its own message, all checked on the host before anything is uploaded, and a refused call writes nothing: a
 * reo_create_multi context; a sharded context; a validity mask set; G or S above 65535 (the 16-plane layout only); n_want outside
 * [1, 2^20]; a or b outside the groups; b == a; a gene_mask byte other than 0 or 1; a NULL output other than passes_run. */
int32_t reo_rank_shift(reo_ctx *ctx, int32_t a, int32_t b /* -1: every other sample */, int64_t *D /* G */);
int32_t reo_top_pairs(reo_ctx *ctx, int32_t a, int32_t b, const uint8_t *gene_mask /* G bytes 0/1, or NULL */,
                      int64_t n_want, int32_t *gene_i, int32_t *gene_j,
                      int32_t *counts /* [n_want][4]: gt_A, eq_A, gt_B, eq_B of (gene_i above gene_j) */,
                      int64_t *key /* [n_want][2]: N (signed), Gamma */,
                      int64_t *n_found, int32_t *passes_run /* may be NULL */);

/* Label-permutation null of the best score: is the winning score of reo_top_pairs larger than the best score that meaningless labels
 * produce?  Geman's top-scoring-pair paper and the k-TSP applications answer that with a permutation test of the maximum; the reference has
 * no such output.
 * Sides A and B are those of reo_top_pairs(a, b), with the context's sizes S_A and S_B.  A label row has S bytes in the caller's column
 * order: 1 = side A, 0 = side B, 2 = takes no part.  A row holds exactly S_A ones and S_B zeros, and the columns that carry a 2 are, in
 * every row, exactly the samples of the groups on neither side (with b = -1 there are none); the caller supplies the rows (shuffled freely,
 * or within batches or patients: the library has no shuffling rule).  So the sizes, and with them the denominator 2 S_A S_B, are the same
 * under every permutation, and which sample slots take part is the same for all of them.
 * Per permutation p, for every pair i < j with both genes inside gene_mask (NULL: all genes): gt and eq per side exactly as reo_top_pairs
 * counts them (no tie coin), side B being "the samples that take part, minus A", and N_p(i, j) = w(A) S_B - w(B) S_A as above.  Then
 *     max_n[p] = max |N_p|,   (arg_i[p], arg_j[p]) = the pair that attains it, the smallest (i, j) among equals,
 *     n_reach[p * n_cuts + t] = the number of eligible pairs with |N_p| >= cuts[t];
 * with no eligible pair max_n[p] = -1, arg_i[p] = arg_j[p] = -1 and n_reach = 0.  The rank shift Gamma is NOT a tie-break here: it depends
 * on the labels and would need a D per permutation.  A row that repeats the observed labels gives max_n = |key[0]| of reo_top_pairs(n_want
 * = 1).  All results are exact integers, independent of the launch geometry, of the batch size and of the arrival order of atomics.
 * Needs the matrix, the groups and the transform (run here if need be); no class table, no thresholds, no reference set.  Reads and writes
 * none of the iteration's buffers.  Host arrays only, allocated by the caller.
 * One walk over the bit planes serves 16 permutations (csrc/toppairsnull.hip, csrc/top_pairs_null.h): the lt / le words of a pair and a
 * block of 32 sample slots do not depend on the labels, a permutation costs one and + popcount per counter, only the tiles with i < j are
 * walked, and per permutation one 63-bit key (|N|, 2^32 - 1 - (i G + j)) and n_cuts counters leave the device; no class table and no
 * candidates are written.  One launch handles at most 64 permutations (REO_TOP_NULL_BATCH=n in the environment, read per call, asks for at
 * most n); reo_get_info 38 = the permutations per launch of the last call, 39 = the microseconds of its kernel launches in all (HIP
 * events).  No other info entry is touched.
 * REO_EINVAL, each with its own message, all checked on the host before anything is uploaded, and a refused call writes nothing:
 * everything reo_top_pairs refuses of the context and of a, b (a reo_create_multi context; a sharded context; a validity mask set; G or S
 * above 65535; a or b outside the groups; b == a); n_perm outside [1, 2^20]; n_cuts outside [0, 8]; a negative cut; a row byte above 2; a
 * row whose 2-columns differ from the samples of neither side (the message names row and column); a row whose count of ones and zeros
 * differs from S_A and S_B (the message names the row, the counts and the sizes); a gene_mask byte other than 0 or 1; a NULL output, except
 * cuts and n_reach with n_cuts == 0. */
int32_t reo_top_pairs_null(reo_ctx *ctx, int32_t a, int32_t b /* -1: every other sample */,
                           const uint8_t *sides /* [n_perm][S], caller's column order */, int64_t n_perm,
                           const uint8_t *gene_mask /* G bytes 0/1, or NULL */,
                           const int64_t *cuts /* n_cuts values of |N|, may be NULL when n_cuts == 0 */, int32_t n_cuts,
                           int64_t *max_n /* n_perm */, int32_t *arg_i, int32_t *arg_j /* n_perm each */,
                           int64_t *n_reach /* [n_perm][n_cuts]; may be NULL when n_cuts == 0 */);

/* Leave-one-out cross-validation of the k-TSP classifier: what Geman et al. report for the top-scoring pair and what Tan et al. choose k
 * by.  The reference has no such output.
 * Sides A and B are those of reo_top_pairs(a, b).  A FOLD is one sample s of side A or of side B; its training set is both sides without s,
 * so its sizes are (S_A - 1, S_B) or (S_A, S_B - 1).  Samples of groups on neither side are no folds.  In fold s, with the sizes and
 * counts of the training set: N(s) = w(A) S_B - w(B) S_A as above, D(s) the rank shift over the training samples, Gamma(s) =
 * |D(s)_i - D(s)_j|, and the pairs i < j with both genes inside gene_mask (NULL: all genes) are ordered exactly as reo_top_pairs orders
 * them: |N(s)| descending, Gamma(s) descending, i ascending, j ascending.  The fold's selection is the greedy disjoint one of k-TSP: walk
 * that order and take a pair when neither of its genes is used yet, up to kmax pairs.  It is nested: the first k picks are the k-TSP of
 * every k <= kmax.  For pick r the held-out sample has an outcome o: +1 gene_i above gene_j, 0 tied, -1 below, under the comparator of
 * the matrix's element type (ties are reported as ties); its vote is sign(N(s)) o, positive = A-like.
 * By definition the result of fold s equals what a context gives in which s is moved into a group on neither side and reo_top_pairs(every
 * pair, a, b), the greedy disjoint selection of kmax pairs and reo_pair_support with outcomes are run.  All results are exact integers,
 * independent of the launch geometry, of buffer sizes and of the order in which the candidates are stored.
 * Row s of the outputs is the caller's column s.  gene_i, gene_j: -1 where the fold has fewer disjoint pairs, and in the rows of samples
 * that are no folds (num, rank_num and outcome are 0 there).  side[s]: 1 = A, 0 = B, 2 = neither.  stats: the cut T, the number of
 * candidates, the histogram passes spent finding T, the number of folds.
 * The route (csrc/top_pairs_loo.h has the proof, csrc/toppairsloo.hip the kernels): removing one sample moves |N| of a pair by at most
 * 2 max(S_A, S_B), so every pick of every fold lies in a band below the full-data winners.  (1) reo_top_pairs' own selection with a list
 * that doubles from 1 024 to 2^20 pairs until its greedy disjoint walk yields 2 kmax pairs, the last with |N| = v; T = max(v - 4 max(S_A,
 * S_B), 0), or 0 when they do not exist.  (2) One emit pass of the search's kernel leaves every pair with |N| >= T on the device (a second
 * one when the first buffer of 2^18 records was too small).  (3) k_loo_words compares the candidates once on the bit planes: per block of
 * 32 sample slots a gt word and an eq word.  (4) k_loo_select, one workgroup per fold, forms the fold's counts by subtracting the
 * sample's own bit, and selects kmax times.  No fold recounts all pairs.
 * More than 2^26 candidates, or more than fit in free device memory: REO_ENOMEM, with the count and the cut in the message (small sides
 * and many genes: one sample moves every score by a large step).  REO_TOP_PAIRS_LOO_CAP=n and REO_TOP_PAIRS_LOO_FIRST=n in the
 * environment lower that cap and the first buffer, REO_TOP_PAIRS_LOO_ALL=1 sets T = 0 (all three: for the tests, read per call).
 * Needs the matrix, the groups and the transform (run here if need be); no class table, no thresholds, no reference set.  Reads and writes
 * none of the iteration's buffers.  Host arrays only, allocated by the caller.  reo_get_info 40 and 41 = the microseconds of k_loo_words
 * and of k_loo_select of the last call (HIP events); no other info entry is touched.
 * REO_EINVAL, each with its own message, checked on the host before anything is uploaded, and a refused call writes nothing: everything
 * reo_top_pairs refuses of the context and of a, b (a reo_create_multi context; a sharded context; a validity mask set; G or S above
 * 65535; a or b outside the groups; b == a); kmax outside [1, 64]; a NULL output; a gene_mask byte other than 0 or 1; a side of fewer
 * than two samples (the message names the side and its size). */
int32_t reo_top_pairs_loo(reo_ctx *ctx, int32_t a, int32_t b /* -1: every other sample */, const uint8_t *gene_mask /* G bytes 0/1, or NULL */,
                          int32_t kmax, int32_t *gene_i, int32_t *gene_j /* [S][kmax] each */,
                          int64_t *num /* [S][kmax]: N(s), signed */, int64_t *rank_num /* [S][kmax]: Gamma(s) */,
                          int8_t *outcome /* [S][kmax]: -1 / 0 / +1 */, int8_t *side /* [S] */, int64_t *stats /* [4] */);

/* Top partners: the best partner genes of given genes.  reo_top_pairs answers "which pairs, out of all"; a user who holds a gene -- a DEG of
 * reo_identify_degs, the genes of a marker panel, or every gene for a gene-level ranking that needs no normalisation -- asks "which single
 * partner makes the best two-gene rule with THIS gene, and how good is that rule".  The reference has no such output.
 * Sides A and B, the four counts per side, N, D and Gamma are exactly those of reo_top_pairs(a, b).  For a query gene q = genes[r] and a
 * partner p != q with partner_mask[p] != 0 (NULL: every gene; q itself need not be inside the mask): the counts are those of "q above p",
 * N_qp is signed (N_pq = -N_qp), Gamma_qp = |D_q - D_p| with D over all genes, independent of the mask (reo_rank_shift).  Row r lists the
 * partners in the order |N| descending, Gamma descending, p ascending -- a total order; it is the subsequence of reo_top_pairs' total order
 * over all pairs that contain q (csrc/top_partners.h has the argument).  The call returns the first m_want partners of every row:
 * partner[r m_want + e] (-1 beyond n_found[r]), counts[4 (r m_want + e) ..] = gt_A, eq_A, gt_B, eq_B of "q above p", key[2 (r m_want + e)]
 * = N (signed), key[.. + 1] = Gamma (counts and key 0 beyond n_found[r]), n_found[r] = min(m_want, eligible partners).  Query genes may
 * repeat and come in any order: every row is decided on its own.  The result is exact and does not depend on the launch geometry, on the
 * batch size or on the arrival order of anything.  (partner, n_found) is the row-shaped input (genes, rowptr, partner) of reo_pair_support.
 * Needs the matrix, the groups and the transform (run here if need be); no class table, no thresholds, no reference set.  Reads and writes
 * none of the iteration's buffers: the resident table, reo_get_ref_mask and a following reo_identify_degs behave as if the call had not
 * happened.  Host arrays only, allocated by the caller; no stage timer of its own.
 * The route (csrc/toppartners.hip, csrc/top_partners.h): k_top_partners_count walks the bit planes as the search's kernel does, with the
 * query genes as its rows and every column as a partner, and stores one 8-byte cell of four unsigned 16-bit counts per (row, column);
 * k_top_partners_select, one workgroup per row, runs m_want rounds over the row's cells, each taking the best key strictly behind the
 * previous round's.  The rows go in batches whose cells and outputs stay within 256 MiB of device memory and within what is free
 * (REO_TOP_PARTNERS_BATCH=n in the environment, read per call, lowers the rows per batch: tests of the seam).  reo_get_info 42 and 43 =
 * the microseconds of the count launches and of the select launches of the last call (HIP events); no other info entry is touched.
 * REO_EINVAL, each with its own message, checked on the host before anything is uploaded, and a refused call writes nothing: everything
 * reo_top_pairs refuses of the context and of a, b (a reo_create_multi context; a sharded context; a validity mask set; G or S above
 * 65535; a or b outside the groups; b == a); n_genes outside [1, 2^20]; m_want outside [1, 1024]; n_genes * m_want above 2^26; a NULL
 * genes or output; a query gene outside [0, G) (the message names the row); a partner_mask byte other than 0 or 1. */
int32_t reo_top_partners(reo_ctx *ctx, int32_t a, int32_t b /* -1: every other sample */,
                         const int32_t *genes, int64_t n_genes /* query genes, any order, repeats allowed */,
                         const uint8_t *partner_mask /* G bytes 0/1, or NULL */, int32_t m_want,
                         int32_t *partner /* [n_genes][m_want], -1 beyond n_found */,
                         int32_t *counts /* [n_genes][m_want][4]: gt_A, eq_A, gt_B, eq_B of (query above partner), 0 beyond */,
                         int64_t *key /* [n_genes][m_want][2]: N (signed, query against partner), Gamma, 0 beyond */,
                         int32_t *n_found /* [n_genes]: min(m_want, eligible partners) */);

/* Label-permutation null of a gene's best partner score: reo_top_partners always lists a winner, and with thousands of candidate partners
 * per gene a large best score is what chance alone produces.  Is the best partner of THIS gene better than the best partner that
 * meaningless labels find for it?  The reference has no such output.
 * Sides A and B are those of reo_top_partners(a, b); the label rows are those of reo_top_pairs_null: S bytes in the caller's column order,
 * 1 = side A, 0 = side B, 2 = takes no part, exactly S_A ones and S_B zeros, a 2 exactly on the samples of the groups on neither side.  So
 * the sizes, and with them 2 S_A S_B, hold under every row.  Query genes are those of reo_top_partners: any order, repeats allowed, q
 * itself need not be inside partner_mask.
 * Per label row b and query row r with gene q = genes[r], over the eligible partners p (p != q, p < G, partner_mask[p] != 0 or the mask
 * NULL): N_b(q, p) from the four counts of "q above p" under the relabelling, ties counted as ties, no coin.  Then
 *     max_n[b n_genes + r] = max |N_b(q, p)|,   arg_p[b n_genes + r] = the smallest p that attains it,
 *     n_reach[b n_genes + r] = the number of eligible p with |N_b(q, p)| >= cuts[r]   (cuts: one per query row; NULL: not counted);
 * a row with no eligible partner gives max_n = -1, arg_p = -1 and n_reach = 0.  The rank shift Gamma is NOT a tie-break here: it depends on
 * the labels.  On a row that repeats the observed labels max_n equals |key[0]| of reo_top_partners(m_want = 1) -- the partner may differ
 * among equal |N|, where Gamma decides there.  With every gene as a query the maximum over the rows is max_n of reo_top_pairs_null, and
 * the smallest (min(q, p), max(q, p)) over the rows that attain it is its (arg_i, arg_j): two independent kernels, one answer.  The null
 * is single-step (maxT over a gene's partners), not step-down.  All results are exact integers, independent of the launch geometry, of the
 * batch size, of the arrival order of atomics and of a row's position in the call.
 * Needs the matrix, the groups and the transform (run here if need be); no class table, no thresholds, no reference set.  Reads the bit
 * planes only; the class table, the reference set and the iteration's buffers are untouched.  Host arrays only, allocated by the caller.
 * The route (csrc/toppartnersnull.hip, csrc/top_partners_null.h): the A-words and the live word of reo_top_pairs_null, and
 * k_top_partners_null, which walks the query rows against every column with one borrow chain for 16 permutations and reduces one 63-bit
 * key (|N|, 2^32 - 1 - p) and one counter per (permutation, query row).  One launch handles at most 64 permutations, fewer when the keys and
 * counters of a batch (12 bytes per permutation and query row) would not fit 256 MiB or the free memory (REO_TOP_PARTNERS_NULL_BATCH=n in
 * the environment, read per call, asks for at most n).  reo_get_info 44 = the permutations per launch of the last call, 45 = the
 * microseconds of its launches of the null kernel in all (HIP events).  No other info entry is touched.
 * REO_EINVAL, each with its own message, all checked on the host before anything is uploaded, and a refused or failed call writes
 * nothing: everything reo_top_pairs refuses of the context and of a, b (a reo_create_multi context; a sharded context; a validity mask set;
 * G or S above 65535; a or b outside the groups; b == a); n_perm outside [1, 2^20]; n_genes outside [1, 2^20]; n_perm * n_genes above
 * 2^26; a NULL sides, genes, max_n or arg_p; cuts without n_reach or n_reach without cuts; a query gene outside [0, G); a negative cut;
 * the three kinds of bad label row of reo_top_pairs_null; a partner_mask byte other than 0 or 1. */
int32_t reo_top_partners_null(reo_ctx *ctx, int32_t a, int32_t b /* -1: every other sample */,
                              const uint8_t *sides /* [n_perm][S], caller's column order */, int64_t n_perm,
                              const int32_t *genes, int64_t n_genes /* query genes, any order, repeats allowed */,
                              const uint8_t *partner_mask /* G bytes 0/1, or NULL */,
                              const int64_t *cuts /* [n_genes] or NULL */,
                              int64_t *max_n /* [n_perm][n_genes] */, int32_t *arg_p /* [n_perm][n_genes] */,
                              int32_t *n_reach /* [n_perm][n_genes]; NULL exactly when cuts is NULL */);

/* Missing values: pair classes from the samples where BOTH genes were observed.  The reference drops every gene with a missing cell
 * (dropmissing!, src/RankCompV3.jl:601) and the library refuses a NaN; with a validity mask V beside the resident matrix a pair (i, j) is
 * compared in the samples where both values exist, and its stability is judged against the threshold of that many samples.
 * For every i < j and every group g:  A_g = {s in g : V[i,s] and V[j,s]}, n_g = |A_g|;  gt_g = #{s in A_g : x_i > x_j, not tied},
 * eq_g = #{s in A_g : tied} under the comparator of the resident element type, exactly as reo_pair_counts applies it;
 * nre_g = gt_g + the keyed coins of (seed, i, j, g) for eq_g ties (the stream of reo_build_pairs).  For comparison k:
 * a = nre_k, n1 = n_k, b = sum of nre_g over g != k, n2 = sum of n_g over g != k, m(n) = reo_threshold(n, pval_reo);
 * ic = 2 if n1 < min_complete[0], else 3 if a >= m(n1), else 1 if n1 - a >= m(n1), else 2;  `it` likewise from b, n2, min_complete[1].
 * The code of (i, j) is 3(ic-1)+(it-1), that of (j, i) 8 minus it.  A side with fewer than min_complete jointly observed samples is
 * unstable, never "stable by unanimity of three samples".  With an all-ones mask and min_complete <= the side sizes the table equals that
 * of reo_compute_thresholds(pval_reo) + reo_build_pairs(k) byte for byte, ties and coins included.
 *
 * reo_set_valid_mask: G x S bytes (nonzero = observed), column-major in the caller's column order, host memory, ld >= G; the shape must be
 * the resident matrix's.  NULL clears the mask.  The bytes are kept on the device, so a later reo_set_groups needs nothing from the
 * caller; a matrix of another shape drops the mask.  The matrix cell under an invalid byte is ignored, but it must still be a number
 * the library accepts: NaN stays refused, the caller writes a filler.
 * While a mask is set, reo_sample_counts, reo_sample_tests, reo_sample_calls, reo_pair_support, reo_rank_shift, reo_top_pairs and
 * reo_build_pairs_contrast are refused
 * (REO_EINVAL, a message that names the mask): they compare on the planes of the whole matrix and would count the fillers.  With no mask
 * set, no call behaves differently.
 *
 * reo_build_pairs_masked builds the class table by the rule above and leaves the context as reo_build_pairs(k) leaves it (reo_get_info 29
 * reads -1, the table is complete); it neither reads nor changes the context's thresholds.  reo_get_info 31 reads 1 while the resident
 * table came from this call; any other build sets it back to 0.  reo_tally, reo_identify_degs, reo_get_ref_mask, reo_pair_list and
 * reo_get_codes run on the table unchanged.
 * reo_pair_counts_masked is the parity hook: n_gt, n_eq and n_avail (= n_g) of the rectangle [i0, i1) x [j0, j1) per group, int32, in the
 * layout of reo_pair_counts ([i - i0][j - j0][g]); at most 2^28 counts per array and call.
 * REO_EINVAL, each with its own message, and a refused call writes nothing: no mask, or none of the matrix's shape; min_complete < 1 or
 * NULL; pval_reo outside (0, 1] (or 1, for which no threshold exists); k outside the groups; S > 65535; G > 65535 (the 16-plane layout
 * only); a sharded context (reo_set_shard with more than one shard) or a reo_create_multi context. */
int32_t reo_set_valid_mask(reo_ctx *ctx, const uint8_t *valid, int64_t G, int64_t S, int64_t ld);
int32_t reo_build_pairs_masked(reo_ctx *ctx, int32_t k, double pval_reo, const int32_t *min_complete /* 2 */);
int32_t reo_pair_counts_masked(reo_ctx *ctx, int64_t i0, int64_t i1, int64_t j0, int64_t j1, int32_t *n_gt, int32_t *n_eq, int32_t *n_avail);

/* Label-permutation null: how many of the calls would there be if the labels meant nothing?  The reference has no such output (one
 * permutation is one whole build there).  The context holds a matrix, groups and thresholds; no validity mask may be set.  For comparison
 * k, side A of the observed data is group k (n1 samples), side B every other sample (n2 = S - n1).  A permutation is a row of S bytes in
 * the caller's column order, 1 = side A, 0 = side B, with exactly n1 ones; the caller supplies the rows (shuffled freely, or within
 * batches or patients: the library has no shuffling rule).  The sizes are kept, so the context's thresholds m1 = thr[0, k], m2 = thr[1, k]
 * hold unchanged.  For permutation p and every i < j:  a = n_gt_A + coins(seed, i, j, 0, n_eq_A),  b = n_gt_B + coins(seed, i, j, 1, n_eq_B)
 * -- the keyed coin stream of reo_build_pairs, keyed by SIDE 0 and 1, never by the context's group ids --,  ic = 3 if a >= m1, else 1 if
 * n1 - a >= m1, else 2;  `it` likewise from b, n2, m2;  the code of (i, j) is 3(ic-1)+(it-1), that of (j, i) 8 minus it.  The table of
 * permutation p therefore equals, byte for byte and ties included, the reo_build_pairs(0) table of a two-group context with the same
 * seed, thresholds and group ids 1 - row.  With a context of more than two groups the permuted tables are still two-group tables, one coin
 * stream per side.  The sample ranks do not depend on the labels: all tables of a batch come from ONE walk over the bit planes.
 *
 * reo_perm_null works in batches of P tables (as many as fit half of the free device memory, at most 64; REO_PERM_BATCH=n in the
 * environment, read at every call, asks for at most n; reo_get_info 34 reports P) and answers REO_ENOMEM with the byte count if not even
 * one table fits beside the resident one.  It needs the resident class table of comparison k (reo_build_pairs(k)), and first runs on it
 * what reo_identify_degs(ref0 = ref_mask, n_iter = 1) runs: delta1_obs[i] is that pass's delta1.  Per permuted table it runs the same
 * tally and pass, unchanged, with the same ref_mask (the null holds the reference set fixed and does not iterate), then
 *   n_ge[i] += |delta1_p(i)| >= |delta1_obs(i)| (as doubles; equality counts, 0 against 0 too),
 *   n_up[p] / n_down[p] = the genes with pval <= pval_deg && padj <= padj_deg and z1 > 0 / z1 < 0,  se_null[p] = the pass's trimmed
 *   standard deviation,  delta1_null[p * G + i] = delta1_p(i) (NULL: not delivered).
 * All arrays are host memory.  The resident class table is intact after the call (reo_get_codes gives the same bytes); the iteration's
 * buffers are used, so reo_get_ref_mask is refused afterwards exactly as after reo_tally.
 * reo_perm_codes is the parity hook: the class codes of ONE permutation's table in the layout of reo_get_codes; it needs no resident table.
 * (REO_PERM_CODES_SLOT=q in the environment, for tests: the table is built as table q of a batch of q + 1, q < 64, and read from there.)
 * REO_EINVAL, each with its own message, before anything is touched: a null argument (delta1_null excepted); a row whose number of ones
 * is not n1, or with a byte other than 0 / 1; n_perm < 1; k outside the groups; no thresholds; (reo_perm_null) no resident table of
 * comparison k built by reo_build_pairs; a validity mask set; a sharded context (more than one shard) or a reo_create_multi context;
 * S > 65535 or G > 65535 (the 16-plane layout only). */
int32_t reo_perm_null(reo_ctx *ctx, int32_t k, const uint8_t *side_a /* [n_perm][S] */, int64_t n_perm,
                      const uint8_t *ref_mask /* G bytes, required */, double pval_deg, double padj_deg,
                      double *delta1_obs /* G */, int32_t *n_ge /* G */,
                      int32_t *n_up /* n_perm */, int32_t *n_down /* n_perm */, double *se_null /* n_perm */,
                      double *delta1_null /* [n_perm][G], may be NULL */);
int32_t reo_perm_codes(reo_ctx *ctx, int32_t k, const uint8_t *side_a /* [S], one permutation */,
                       int64_t i0, int64_t i1, int64_t j0, int64_t j1, uint8_t *code);

/* Sample tests: is gene i UP OR DOWN IN ONE SAMPLE?  The tallies call a gene over the groups; this call tests one sample's orderings of
 * the gene against the pairs that are stable in the control group, with Fisher's exact test -- the individual-level question of the
 * RankComp family.  The reference has no such output.
 * For query q, gene i = genes[q] (any order, repeats allowed, each entry is its own row), the background is
 *     J = {j != i : partner_mask[j] != 0, ic(i, j) in {1, 3}}
 * where ic is the c-side class of the resident table (class code 3*(ic-1)+(it-1)); the c-side is group k of reo_build_pairs(k), or ctrl
 * of reo_build_pairs_contrast(ctrl, treat).  partner_mask NULL = the mask of reo_get_ref_mask, read where it lies.  J splits into
 *     A = {ic = 3} (class mask 0x1C0: i stably above j in the control group)   n_above_ctrl[q] = |A|
 *     B = {ic = 1} (class mask 0x007)                                          n_below_ctrl[q] = |B|
 * and for every sample s in the CALLER's column order -- every group's samples, the control's own included -- by the comparator of the
 * resident matrix's element type as reo_sample_counts applies it (ties are reported as ties, no tie coin is drawn):
 *     rev_up[q * S + s]   = #{j in B : x_i > x_j}          rev_down[q * S + s] = #{j in A : x_i < x_j}
 *     tied[q * S + s]     = #{j in J : tied}               u = #{j in J : x_i > x_j}      d = |J| - u - tied
 * Fisher's 2 x 2 table is [[n_above_ctrl, n_below_ctrl], [u, d]]; with N its total, K = n_above_ctrl + u, n = u + d and
 * X ~ Hypergeometric(N, K, n):
 *     p_up[q * S + s] = P(X >= u)          p_down[q * S + s] = P(X <= u)
 * An empty J, or n = 0 (every pair tied), gives 1 and 1.  A two-sided value, min(1, 2 min(p_up, p_down)), and any correction for multiple
 * testing are the caller's (the Python package forms both on the host).  Samples of the control group are tested against a background
 * that they helped to define: their p-values are not those of an independent sample.
 * rev_up, rev_down and tied may be NULL (they are then not stored); n_above_ctrl and n_below_ctrl may be NULL as well.
 * Arithmetic (csrc/sample_tests.h, evaluated by the kernel and by a host driver alike): pmf(u) from a table of log k!, k = 0 .. 2 (G - 1)
 * (a running sum of logl in long double, rounded once per entry, uploaded once per context and rebuilt when G changes); the tail that points
 * away from the mode floor((n+1)(K+1)/(N+2)) is summed by the ratio recurrence, integer products formed exactly, until the support ends
 * or a term falls below 2^-60 of the sum; the other tail is 1 - small + pmf(u); both are clamped to [0, 1].  Relative error against the
 * exact tails: DESIGN.md section 7 (n9).  Tails below about 2^-1022 are subnormal or 0.
 * Per batch of queries: two launches of the kernel of reo_sample_counts into device buffers that stay on the device, one launch of
 * k_sample_fisher (csrc/sampletests.hip), one thread per (query, sample).  Batches are sized so that every device buffer stays under
 * 32 MiB (at least one query per batch); REO_SAMPLE_TESTS_BATCH in the environment, read per call, lowers the batch to that many queries
 * (tests of the batch seam).  Needs the class table and the transform; reads the reference mask and changes nothing: reo_get_ref_mask and
 * a following reo_identify_degs behave as if the call had not happened.  Both plane layouts, every S.
 * Host arrays only; no stage timer of its own.
 * REO_EINVAL, each with its own message, decided before anything is uploaded, and a refused call writes nothing: a NULL genes, p_up or
 * p_down; n_genes < 1 or above 2^30; a gene outside [0, G); no class table; a NULL partner_mask while reo_get_ref_mask would refuse (its
 * reason is passed on); a reo_create_multi context.  An incomplete sharded table: REO_ECOMM, as reo_tally. */
int32_t reo_sample_tests(reo_ctx *ctx, const int32_t *genes, int64_t n_genes,
                         const uint8_t *partner_mask /* G bytes; NULL = the mask of reo_get_ref_mask */,
                         int32_t *n_above_ctrl, int32_t *n_below_ctrl /* n_genes; may be NULL */,
                         int32_t *rev_up, int32_t *rev_down, int32_t *tied /* n_genes x S row-major, ld = S; may be NULL */,
                         double *p_up, double *p_down /* n_genes x S row-major, ld = S */);

/* The calls themselves: is gene genes[q] up (+1), down (-1) or neither (0) in sample s, with the multiple-testing correction made on the
 * device -- one byte per cell comes back instead of the two tails.  Per cell p_up and p_down are exactly those of reo_sample_tests for
 * the same genes and partner_mask (same kernels, same batches' arithmetic), and
 *     pval = min(1, 2 min(p_up, p_down))
 *     padj = Benjamini-Hochberg of pval down sample column s over the n_genes rows of THIS call (a repeated gene is a row of its own):
 *            with the rows in ascending order of pval, padj_(i) = min(1, min over j >= i of pval_(j) (n_genes / j))
 *     calls[q * S + s] = +1 where pval <= pval_deg, padj <= padj_deg and p_up < p_down; -1 with the tails the other way; else 0
 *     cut[s]    = the rows of column s with padj <= padj_deg, whatever pval_deg says (the step-up rule's k*)
 *     n_up[s], n_down[s] = the rows of column s called +1 / -1
 * in the CALLER's column order.  The padj values themselves are not formed (they need the sorted order): reo_sample_tests and the
 * caller's own correction keep that route.  The decision is that of the sorted rule bit for bit: with m_i = min{r : pval_i (n / r) <=
 * padj_deg} and H(r) = #{i : m_i <= r}, k* = max{r : H(r) >= r} and padj_i <= padj_deg <=> m_i <= k* (csrc/sample_calls.h; DESIGN.md
 * section 3.4), and pval (n / r) is evaluated with the two roundings of the sorted rule's p * (n / rank).
 * Three phases (csrc/samplecalls.hip): per batch of queries the launches of reo_sample_tests into device buffers that stay there, then
 * k_call_rank packs rank, direction and the pval_deg bit of every cell into a 32-bit word, kept by sample for the whole call
 * (4 x n_genes x S bytes, n_genes rounded up to 32); k_call_cut, one workgroup per sample, finds k* from a histogram of the ranks in LDS;
 * k_call_emit stores the bytes, which come back in one copy.  Batches as reo_sample_tests; REO_SAMPLE_CALLS_BATCH in the environment,
 * read per call, lowers the batch (tests of the batch seam).  Needs the class table and the transform; reads the reference mask and
 * changes nothing: reo_get_ref_mask and a following reo_identify_degs behave as if the call had not happened.  Both plane layouts,
 * every S.  Host arrays only; no stage timer of its own.  cut, n_up and n_down may be NULL.
 * REO_EINVAL, each with its own message, decided before anything is uploaded, and a refused call writes nothing: a NULL genes or calls;
 * n_genes < 1 or above 2^29 - 2 (the rank and three more bits share the word); pval_deg or padj_deg NaN or outside [0, 1]; a gene outside
 * [0, G); no class table; a NULL partner_mask while reo_get_ref_mask would refuse (its reason is passed on); a reo_create_multi context.
 * REO_ENOMEM, with the bytes needed in the message: the call's device buffers (the resident words foremost) exceed the free device memory.
 * An incomplete sharded table: REO_ECOMM, as reo_tally.  Counts that G genes cannot produce: REO_EHIP, and no call is written. */
int32_t reo_sample_calls(reo_ctx *ctx, const int32_t *genes, int64_t n_genes,
                         const uint8_t *partner_mask /* G bytes; NULL = the mask of reo_get_ref_mask */,
                         double pval_deg, double padj_deg,
                         int8_t *calls  /* n_genes x S row-major, ld = S, caller's column order */,
                         int32_t *cut   /* S; may be NULL: k*, the number of rows with padj <= padj_deg in the column */,
                         int32_t *n_up, int32_t *n_down /* S each; may be NULL: rows called +1 / -1 in the column */);

/* McCullagh test on 3x3 tables given as 9 tallies each (n x 9 row-major),
 * evaluated by the device routine the iteration uses; out is n x 5 row-major
 * (pval, delta1, delta2, se, z1) -- src/RankCompV3.jl:225-259. */
int32_t reo_mccullagh(reo_ctx *ctx, const int32_t *cont, int64_t n, double *out);

/* Pseudo-bulk front end: pseudobulk_group (src/RankCompV3.jl:56-67, call site :608-612) for all
 * groups at once.  `order` lists the cells (0-based columns) of every output profile back to back --
 * the reference's shuffled partition, sample(1:c, c) + Iterators.partition (:62) -- and
 * chunk_ptr[o] .. chunk_ptr[o+1] delimits profile o (n_out + 1 entries, chunk_ptr[n_out] = n_order).
 * Each profile is the row-wise sum of its cells taken in that order (:63): exact for Int64,
 * bit-reproducible for Float64.  out is G x n_out column-major, caller-allocated.
 * dense: X is the G x C cell matrix, column-major (what the reference holds after CSV.read);
 * csc:   this build's container for sparse single-cell counts (colptr C+1, rowidx/val nnz).  The entries are uploaded in chunks:
 *        host threads (REO_UPLOAD_THREADS) check the row indices and narrow them (16 bits when G <= 65 536) and the Int64 values
 *        (16 / 32 bits when they fit) into pinned staging, the device widens them -- exact; 60 M entries: 28 -> 9 ms. */
int32_t reo_pseudobulk_dense_f64(reo_ctx *ctx, const double *X, int64_t G, int64_t C, int64_t ld,
                                 const int32_t *order, int64_t n_order, const int32_t *chunk_ptr,
                                 int32_t n_out, double *out);
int32_t reo_pseudobulk_dense_i64(reo_ctx *ctx, const int64_t *X, int64_t G, int64_t C, int64_t ld,
                                 const int32_t *order, int64_t n_order, const int32_t *chunk_ptr,
                                 int32_t n_out, int64_t *out);
int32_t reo_pseudobulk_csc_f64(reo_ctx *ctx, int64_t G, int64_t C, const int64_t *colptr, const int32_t *rowidx,
                               const double *val, const int32_t *order, int64_t n_order,
                               const int32_t *chunk_ptr, int32_t n_out, double *out);
int32_t reo_pseudobulk_csc_i64(reo_ctx *ctx, int64_t G, int64_t C, const int64_t *colptr, const int32_t *rowidx,
                               const int64_t *val, const int32_t *order, int64_t n_order,
                               const int32_t *chunk_ptr, int32_t n_out, int64_t *out);

/* The same sums as the context's expression matrix.  Arguments, argument checks, the chunked and narrowed upload, the kernels and so the
 * summation order (exact for Int64, bit-reproducible for Float64) are those of the reo_pseudobulk_* entry of the same name, without `out`:
 * the G x n_out result is written into the context's own matrix in HBM (Float64 or Int64, ld = G) and becomes the expression matrix as if
 * reo_set_matrix_dev_* had delivered it; nothing is copied to the host.  G and n_out must satisfy the limits of reo_set_matrix_* (G in
 * [2, 262143], n_out in [2, 1048576]).  The context is invalidated as by reo_set_matrix_*; reo_get_info 19 and 21-23 read 0.  On ANY failure
 * the context holds no matrix until the next reo_set_matrix_* (it stays usable).  Not available on a reo_create_multi context (REO_EINVAL;
 * one process per GPU works, every rank has its own context). */
int32_t reo_set_matrix_pseudobulk_dense_f64(reo_ctx *ctx, const double *X, int64_t G, int64_t C, int64_t ld,
                                            const int32_t *order, int64_t n_order, const int32_t *chunk_ptr, int32_t n_out);
int32_t reo_set_matrix_pseudobulk_dense_i64(reo_ctx *ctx, const int64_t *X, int64_t G, int64_t C, int64_t ld,
                                            const int32_t *order, int64_t n_order, const int32_t *chunk_ptr, int32_t n_out);
int32_t reo_set_matrix_pseudobulk_csc_f64(reo_ctx *ctx, int64_t G, int64_t C, const int64_t *colptr, const int32_t *rowidx,
                                          const double *val, const int32_t *order, int64_t n_order,
                                          const int32_t *chunk_ptr, int32_t n_out);
int32_t reo_set_matrix_pseudobulk_csc_i64(reo_ctx *ctx, int64_t G, int64_t C, const int64_t *colptr, const int32_t *rowidx,
                                          const int64_t *val, const int32_t *order, int64_t n_order,
                                          const int32_t *chunk_ptr, int32_t n_out);

/* SPARSE ON THE DEVICE.  The same three families for a matrix whose arrays already live in HBM on the context's device (a torch sparse_csc
 * tensor on the GPU is this container as it is): nothing crosses the link, the caller's buffers are only read and have been read when the
 * call returns (it waits for the context's stream, so nothing has to be kept alive beyond the call).  The suffix names the element type of
 * d_val / dX; d_colptr ([S + 1] or [C + 1]) and d_rowidx ([nnz]) are both int32 (index_bits = 32) or both int64 (64; torch's default); nnz,
 * the length of d_rowidx and d_val, is passed in so that nothing is read back before buffers are sized, and must equal colptr[last].
 * order and chunk_ptr stay HOST arrays, checked as in the host entries.
 *   reo_set_matrix_csc_dev_<T> is reo_set_matrix_csc_<T>: row indices strictly increasing inside a column, stored zeros and -0.0 kept as
 *     stored, the resident matrix Float64 / Int64 / Float32 (compared in Float32) / Int64 for Int32 values, in the context's own memory
 *     (ld = G), bit-identical to the host entry on the same arrays in every order of calls.
 *   reo_set_matrix_pseudobulk_csc_dev_<T> / _dense_dev_<T> are reo_set_matrix_pseudobulk_csc_* / _dense_*: cells in the given order,
 *     left-to-right sums.  Float32 and Int32 cells are widened AS THEY ARE READ and summed in Float64 / Int64, so the sums are
 *     bit-identical to the host entry on the widened values (that is this library's rule for such cells, not the reference's arithmetic
 *     for a Matrix{Float32}).
 * THE CHECK.  The index arrays are untrusted and the kernels index with them, so one kernel checks them first (one stream over the
 * index bytes): per column its two colptr words -- inside [0, nnz], non-decreasing, at most G apart, colptr[0] = 0, colptr[last] = nnz
 * -- and only then the column's row indices -- inside [0, G), strictly increasing.  The verdict returns to the host (8 bytes) before the
 * consuming kernel is queued.  A fault is REO_EINVAL and the message names its class and the lowest offending column; so are an
 * index_bits other than 32 / 64, an nnz that no such matrix has and a null d_rowidx / d_val with nnz > 0.  The arrays must not be written
 * by the caller while the call runs.
 * On ANY failure the context holds no matrix until the next reo_set_matrix_* (it stays usable).  Not available on a reo_create_multi
 * context (REO_EINVAL).  reo_get_info 27 reads 1 after reo_set_matrix_csc_dev_* (and 23 its nnz; 19, 21 and 22 read 0: nothing was
 * uploaded); after the pseudo-bulk entries 19 and 21-23 and 27 read 0, as after the host ones. */
int32_t reo_set_matrix_csc_dev_f64(reo_ctx *ctx, int64_t G, int64_t S, int64_t nnz, const void *d_colptr, const void *d_rowidx,
                                   int32_t index_bits /* 32 or 64 */, const void *d_val);
int32_t reo_set_matrix_csc_dev_i64(reo_ctx *ctx, int64_t G, int64_t S, int64_t nnz, const void *d_colptr, const void *d_rowidx,
                                   int32_t index_bits /* 32 or 64 */, const void *d_val);
int32_t reo_set_matrix_csc_dev_f32(reo_ctx *ctx, int64_t G, int64_t S, int64_t nnz, const void *d_colptr, const void *d_rowidx,
                                   int32_t index_bits /* 32 or 64 */, const void *d_val);
int32_t reo_set_matrix_csc_dev_i32(reo_ctx *ctx, int64_t G, int64_t S, int64_t nnz, const void *d_colptr, const void *d_rowidx,
                                   int32_t index_bits /* 32 or 64 */, const void *d_val);
int32_t reo_set_matrix_pseudobulk_csc_dev_f64(reo_ctx *ctx, int64_t G, int64_t C, int64_t nnz, const void *d_colptr, const void *d_rowidx,
                                              int32_t index_bits, const void *d_val, const int32_t *order, int64_t n_order,
                                              const int32_t *chunk_ptr, int32_t n_out);
int32_t reo_set_matrix_pseudobulk_csc_dev_i64(reo_ctx *ctx, int64_t G, int64_t C, int64_t nnz, const void *d_colptr, const void *d_rowidx,
                                              int32_t index_bits, const void *d_val, const int32_t *order, int64_t n_order,
                                              const int32_t *chunk_ptr, int32_t n_out);
int32_t reo_set_matrix_pseudobulk_csc_dev_f32(reo_ctx *ctx, int64_t G, int64_t C, int64_t nnz, const void *d_colptr, const void *d_rowidx,
                                              int32_t index_bits, const void *d_val, const int32_t *order, int64_t n_order,
                                              const int32_t *chunk_ptr, int32_t n_out);
int32_t reo_set_matrix_pseudobulk_csc_dev_i32(reo_ctx *ctx, int64_t G, int64_t C, int64_t nnz, const void *d_colptr, const void *d_rowidx,
                                              int32_t index_bits, const void *d_val, const int32_t *order, int64_t n_order,
                                              const int32_t *chunk_ptr, int32_t n_out);
int32_t reo_set_matrix_pseudobulk_dense_dev_f64(reo_ctx *ctx, const void *dX, int64_t G, int64_t C, int64_t ld, const int32_t *order,
                                                int64_t n_order, const int32_t *chunk_ptr, int32_t n_out);
int32_t reo_set_matrix_pseudobulk_dense_dev_i64(reo_ctx *ctx, const void *dX, int64_t G, int64_t C, int64_t ld, const int32_t *order,
                                                int64_t n_order, const int32_t *chunk_ptr, int32_t n_out);
int32_t reo_set_matrix_pseudobulk_dense_dev_f32(reo_ctx *ctx, const void *dX, int64_t G, int64_t C, int64_t ld, const int32_t *order,
                                                int64_t n_order, const int32_t *chunk_ptr, int32_t n_out);
int32_t reo_set_matrix_pseudobulk_dense_dev_i32(reo_ctx *ctx, const void *dX, int64_t G, int64_t C, int64_t ld, const int32_t *order,
                                                int64_t n_order, const int32_t *chunk_ptr, int32_t n_out);

/* The reference's low-expression filters on the resident matrix (any host entry, a _dev buffer, the pseudo-bulk entries; resident Float64,
 * Int64 or Float32), :618 then :626 of src/RankCompV3.jl:
 *   profile s is kept iff #{g : x[g,s] > 0} > min_profiles;
 *   gene g is kept iff #{KEPT s : x[g,s] > 0} > min_features (a gene expressed only in dropped profiles goes too).
 * `> 0` is the comparison of the element type: -0.0, negative values and NaN do not count, +Inf and subnormals do.
 * profile_kept (S bytes) and gene_kept (G bytes) receive the 0 / 1 masks -- the caller subsets names, groups and a reference mask with them --
 * and S_kept / G_kept the numbers S' and G'; any of the four may be NULL.  The compacted G' x S' matrix, order preserved, becomes the resident
 * matrix (reo_get_info 0 and 1 then report G' and S').  When nothing is dropped no copy is made.  A caller's _dev buffer is never written:
 * the compacted matrix lives in memory of the context's own, and the buffer may be released once the call has returned with something dropped.
 * The call always invalidates the context (see CELLS / ORDER OF CALLS above).  G' < 2 or S' < 2: REO_EINVAL with the numbers in the message
 * (masks and numbers are delivered all the same); the context then holds no matrix and stays usable.  Two counting kernels and one gather on
 * the context's stream (stage timer 7), the G + S counts visit the host in between.  Not available on a reo_create_multi context (REO_EINVAL). */
int32_t reo_filter_matrix(reo_ctx *ctx, int64_t min_profiles, int64_t min_features, uint8_t *profile_kept, uint8_t *gene_kept,
                          int64_t *S_kept, int64_t *G_kept);

/* Parity hook: the resident matrix as it stands, G x S column-major without the leading dimension, elements of 8 bytes (Float64 / Int64) or
 * 4 (Float32); reo_get_info 24 says which.  `bytes` must be exactly G * S * element size (REO_EINVAL otherwise). */
int32_t reo_get_matrix(reo_ctx *ctx, void *out, int64_t bytes);

/* Stage timers (HIP events on the library's stream), milliseconds, summed
 * since the last reo_reset_timings.  Index: 0 rank/band transform, 1 pair
 * kernel K1, 2 tally stage K2 (full scan or incremental update, sum), 3 iteration passes in total (K2 + the
 * statistics kernels K3, sum), 4 number of K2 launches (passes enqueued after
 * convergence return at once and are counted too), 5 number of K1 launches,
 * 6 exchange of the class table between shards (HIP events), 7 pseudo-bulk kernel and the kernels of reo_filter_matrix, 8 K2 stage of the passes that scanned the whole table (sum), 9 their
 * number, 10 K2 stage of the passes that updated the tallies incrementally (sum), 11 host wall time inside reo_set_matrix_f64 / _i64 /
 * _f32 / _i32 (the upload from host memory, with whatever was pipelined behind it). */
enum { REO_NTIMINGS = 12 };
int32_t reo_set_profiling(reo_ctx *ctx, int32_t on);
int32_t reo_reset_timings(reo_ctx *ctx);
int32_t reo_get_timings(reo_ctx *ctx, double *ms, int32_t n);

/* Facts about the current problem for roofline accounting and for mirroring
 * the shard ownership rule: 0 G, 1 S, 2 padded G (table row pitch in bits),
 * 3 class-table bytes, 4 data-has-ties flag, 5 pair tiles owned by this
 * shard, 6 pair tiles total, 7 gene rows per pair tile, 8 gene columns per
 * workgroup, 9 column chunks per panel, 10 tiles per work-unit column,
 * 11 padded sample slots, 12 the last class table came from the shared
 * per-group counts (more than two groups: the one-vs-rest comparisons count
 * every group once and keep the counts in HBM; REO_SHARE_GROUP_COUNTS=0 in the
 * environment recounts per comparison), 13 bytes held by those counts, 14 the last transform ranked every sample
 * inside one workgroup, 15 the iteration passes keep their rank histogram per XCD (the self-test of reo_create passed;
 * REO_XCC_LOCAL=0 switches it off), 16-18 the last reo_identify_degs: the period p of the cycle its iteration was found in
 * (0: none found), the pass in front of which the reference set equalled that of p passes earlier, and the passes that
 * were then skipped instead of executed (see reo_identify_degs; REO_CYCLE=0 switches the watch off), 19 the bytes that the last
 * reo_set_matrix_i64 / _f64 put on the PCIe link (chunks whose values all fit travel as int16 / int32 -- Float64 chunks of
 * integer-valued or single-precision numbers too, as int16 / int32 / float32 -- converted by REO_UPLOAD_THREADS host threads,
 * default 12, and widened on the device: bit-exact; 0 threads = the caller's array as it is; reo_set_matrix_f32 / _i32: the caller's
 * array as it is, 4 bytes per value, no host threads), 20 the launches of the pair kernel that
 * the last pipelined reo_set_matrix_* made over a RANGE of a group's sample blocks (the pair kernel then starts before the whole group
 * has arrived; the counts of a range wait in HBM for the group's last range, which classifies -- REO_EAGER_RANGES=1 in the environment
 * launches whole sides only, as in round 5; 2..6 asks for that many ranges per side; default: by the number of blocks), 21 the last
 * host matrix was read row-major in place (reo_set_matrix_rm_*: 1; every other reo_set_matrix_*: 0), 22 the last host matrix came as CSC
 * (reo_set_matrix_csc_*: 1; every other reo_set_matrix_*: 0), 23 the stored entries (nnz) of that CSC matrix, 24 the element type of the
 * resident matrix (0 none, 1 Float64, 2 Int64 -- Int32 input is widened --, 3 Float32), 25 the last class table was built with the genes
 * in slot order (tie-free data of two groups on one shard; REO_K1_SLOTS=0 switches it off; the table is the same bit for bit), 26 the
 * half-height tiles of that build whose count loop was skipped (counted when asked for, n > 26: one small kernel and a wait), 27 the matrix
 * was made dense from CSC arrays on the device (reo_set_matrix_csc_dev_*: 1, and 23 then reports its nnz; every other reo_set_matrix_*: 0), 28 how that build put the table's columns back
 * into gene order (0: no slot build; 8 or 4: a word at a time, 8 or 4 table rows per 32- or 16-bit entry -- the default, by the LDS the
 * gene count needs; 1: a bit at a time, REO_K1_UNSLOT=0 in the environment; REO_K1_UNSLOT=8 or 4 asks for that word form wherever its
 * LDS fits; the table is the same bit for bit under all of them), 29 the treat group of the resident class table (reo_build_pairs_contrast;
 * -1: every other sample, reo_build_pairs with more than two groups, and -1 while there is no table), 30 the slot orders of that
 * build (0: no slot build; 1: one order for both sides; 2: an order per side, the default where the two sides together have at least
 * 16 sample blocks of 32 and a word form puts the columns back; REO_K1_SLOT_SIDES=1 or 2 in the environment asks for that one
 * everywhere; the table is the same bit for bit under both), 31 the resident class table came from reo_build_pairs_masked (1; any other
 * build, and no table: 0), 32 the operands of that slot build were sliced straight from the transform's 16-bit position rows into slot
 * order (1, the default; 0: no slot build, or REO_K1_SLOT_SLICE=0 in the environment -- the gene-order bit planes are made and gathered;
 * the table is the same bit for bit), 33 how many times the gene-order bit planes of the current transform were made on demand (a
 * transform of tie-free data that a slot build can follow leaves them unmade; the first pair query, masked build or identity-order build
 * makes them once: 0 or 1), 34 the tables per batch of the last reo_perm_null, 35 the microseconds that its launches of the permuted pair
 * kernel took in all (HIP events around each launch), 36 and 37 the microseconds of the histogram passes and of the emit pass of the
 * last reo_top_pairs, 38 the permutations per launch of the last reo_top_pairs_null, 39 the microseconds that its launches of the null
 * kernel took in all (HIP events around each launch), 40 and 41 the microseconds of k_loo_words and of k_loo_select of the last
 * reo_top_pairs_loo, 42 and 43 the microseconds of the launches of k_top_partners_count and of k_top_partners_select of the last
 * reo_top_partners, 44 the permutations per launch of the last reo_top_partners_null, 45 the microseconds that its launches of
 * k_top_partners_null took in all (HIP events around each launch). */
int32_t reo_get_info(reo_ctx *ctx, int64_t *info, int32_t n);

#ifdef __cplusplus
}
#endif
#endif /* REO_HIP_H */
