// The query entry points of the C ABI (include/reo_hip.h): reo_pair_list, reo_sample_counts, reo_sample_tests, reo_sample_calls,
// reo_pair_support, reo_rank_shift, reo_top_pairs, reo_top_pairs_null, reo_top_pairs_loo, reo_top_partners, reo_top_partners_null.  Host code
// only; the kernels are in pairlist.hip, samplecounts.hip, sampletests.hip, samplecalls.hip, pairsupport.hip, toppairs.hip, toppairsnull.hip,
// toppairsloo.hip, toppartners.hip and toppartnersnull.hip.  What they share stands once, in front.
#include <algorithm>
#include <cstdlib>
#include <utility>

#include "pair_list.h"
#include "reo_internal.h"
#include "sample_counts.h"
#include "sample_tests.h"
#include "sample_calls.h"
#include "pair_support.h"
#include "top_pairs.h"
#include "top_pairs_null.h"
#include "top_pairs_loo.h"
#include "top_partners.h"
#include "top_partners_null.h"

namespace reo {
namespace {

// How every query begins: one GPU, a usable context and, for the three that read it, a whole class table.
int32_t begin_query(reo_ctx *c, const char *what, bool need_table)
{
    int32_t rc = no_multi(c, what);
    if (rc || (rc = use(c))) return rc;
    return need_table ? need_complete_table(c) : REO_OK;
}

// A null partner_mask stands for the reference set of the last reo_identify_degs: there must be one.
int32_t need_partner_set(reo_ctx *c, const char *what, const uint8_t *partner_mask)
{
    if (partner_mask || c->ref_slot >= 0) return REO_OK;
    set_error("%s: partner_mask is null and there is no reference set to take its place: %s", what, c->ref_gone);
    return REO_EINVAL;
}

// The partner mask as bits on the device: the caller's bytes packed into buffers of the call, or the resident reference set.  Declared in
// FRONT of the call's DrainOnExit, like every other device buffer of a call: the wait comes before their release.
struct PartnerMask {
    DevBuf<uint8_t> bytes;
    DevBuf<uint32_t> packed;
    const uint32_t *bits = nullptr;   // what the kernels read (after prepare)
    int32_t prepare(reo_ctx *c, const uint8_t *partner_mask)   // behind need_partner_set: a null mask indexes refbits with ref_slot >= 0
    {
        int32_t rc;
        if (!partner_mask) { bits = c->refbits[c->ref_slot].p; return REO_OK; }
        if ((rc = bytes.ensure(c->Gp)) || (rc = packed.ensure(c->Wp))) return rc;
        bits = packed.p;
        return REO_OK;
    }
    int32_t upload(reo_ctx *c, const uint8_t *partner_mask)   // on the stream; nothing to do for the reference set
    {
        if (!partner_mask) return REO_OK;
        REO_HIP_CHECK(hipMemsetAsync(bytes.p, 0, c->Gp, c->stream));
        REO_HIP_CHECK(hipMemcpyAsync(bytes.p, partner_mask, static_cast<size_t>(c->G), hipMemcpyHostToDevice, c->stream));
        return launch_pack_ref(c, bytes.p, packed.p);
    }
};

// The caller's column of every sample slot, from the group labels the transform laid the slots out by.
int32_t query_slot_map(reo_ctx *c, const char *what, std::vector<int32_t> &map)
{
    if (sc_slot_map(c->group_id.data(), c->S, c->ngroups, map) && !c->goff32.empty() && static_cast<int64_t>(map.size()) == c->goff32.back())
        return REO_OK;
    set_error("%s: the sample slots of the bit planes do not match the group labels", what);
    return REO_EHIP;
}

// REO_*_BATCH (tests): a batch size that can only lower the budget's; 0 when unset.
int64_t env_batch(const char *name) { const char *env = getenv(name); return env ? atoll(env) : 0; }

// n elements from the device into host[at ..], on the stream; a null host array is one the caller did not ask for.
template <class T>
int32_t copy_back(reo_ctx *c, T *host, size_t at, const T *dev, size_t n)
{
    if (host) REO_HIP_CHECK(hipMemcpyAsync(host + at, dev, n * sizeof(T), hipMemcpyDeviceToHost, c->stream));
    return REO_OK;
}

// How reo_rank_shift and reo_top_pairs begin: a context, its device, and -- on one GPU -- a matrix and groups of one size (the refusals of
// ensure_transform: nothing runs).  The context checks proper are tp_check_context's.
int32_t top_begin(reo_ctx *c, const char *what)
{
    int32_t rc = use(c);
    if (rc) return rc;
    if (!c->in_multi && (c->dtype == 0 || c->group_id.empty() || static_cast<int64_t>(c->group_id.size()) != c->S)) return ensure_transform(c);
    return REO_OK;
}

TpState top_state(reo_ctx *c)
{
    TpState st;
    st.multi = c->in_multi; st.world = c->world; st.has_mask = mask_in_force(c); st.G = c->G; st.S = c->S; st.ngroups = c->ngroups;
    return st;
}

// Two timing events around a launch; the elapsed time is read behind a wait for the stream.  Declared in FRONT of the call's DrainOnExit:
// the events are destroyed behind its wait.
struct TimedPair {
    hipEvent_t a = nullptr, b = nullptr;
    TimedPair() = default;
    TimedPair(const TimedPair &) = delete;
    TimedPair &operator=(const TimedPair &) = delete;
    ~TimedPair()
    {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
    int32_t make()
    {
        REO_HIP_CHECK(hipEventCreate(&a));
        REO_HIP_CHECK(hipEventCreate(&b));
        return REO_OK;
    }
    int32_t start(reo_ctx *c) { REO_HIP_CHECK(hipEventRecord(a, c->stream)); return REO_OK; }
    int32_t stop(reo_ctx *c) { REO_HIP_CHECK(hipEventRecord(b, c->stream)); return REO_OK; }
    int32_t add_us(int64_t *sum)
    {
        float ms = 0.f;
        REO_HIP_CHECK(hipEventElapsedTime(&ms, a, b));
        *sum += static_cast<int64_t>(ms * 1000.0f + 0.5f);
        return REO_OK;
    }
};

// The two sides of a search: group a against group b, or against every other sample (b = -1); a and b have passed tp_check_context.
struct TopSides {
    std::vector<int32_t> gside;   // per group: 0 side A, 1 side B, 2 neither
    int s_a = 0, s_b = 0;
    void count(reo_ctx *c, int32_t a, int32_t b)   // the sides and their sizes, unchecked
    {
        gside.assign(static_cast<size_t>(c->ngroups), 2);
        for (int g = 0; g < c->ngroups; ++g) gside[static_cast<size_t>(g)] = g == a ? 0 : ((b < 0 || g == b) ? 1 : 2);
        s_a = s_b = 0;
        for (const int32_t g : c->group_id) {
            if (g < 0 || g >= c->ngroups) continue;
            if (gside[static_cast<size_t>(g)] == 0) ++s_a;
            else if (gside[static_cast<size_t>(g)] == 1) ++s_b;
        }
    }
    int32_t make(reo_ctx *c, const char *what, int32_t a, int32_t b)
    {
        count(c, a, b);
        if (s_a > 0 && s_b > 0) return REO_OK;
        set_error("%s: side A has %d samples and side B %d, both sides need at least one", what, s_a, s_b);
        return REO_EINVAL;
    }
};

}  // namespace
}  // namespace reo

using namespace reo;

extern "C" {

// The partners behind the tallies (include/reo_hip.h): count on the device, prefix sums on the host (the caller wants rowptr anyway), fill on
// the device into buffers sized from the counted total.
int32_t reo_pair_list(reo_ctx *c, const int32_t *genes, int64_t n_genes, const uint8_t *partner_mask, uint32_t class_mask, int64_t *rowptr,
                      int32_t *partner, uint8_t *code, int64_t capacity)
{
    int32_t rc = begin_query(c, "reo_pair_list", true);
    if (rc) return rc;
    char msg[320];
    if (pair_list_check_args(c->G, genes, n_genes, class_mask, rowptr, partner, code, capacity, msg, sizeof msg)) { set_error("%s", msg); return REO_EINVAL; }
    if ((rc = need_partner_set(c, "reo_pair_list", partner_mask))) return rc;
    const size_t n = static_cast<size_t>(n_genes);
    DevBuf<int32_t> d_genes, d_count, d_partner, d_flag;
    DevBuf<int64_t> d_rowptr;
    DevBuf<uint8_t> d_code;
    PartnerMask mask;
    if ((rc = d_genes.ensure(n)) || (rc = d_count.ensure(n)) || (rc = mask.prepare(c, partner_mask))) return rc;
    std::vector<int32_t> count(n);
    int32_t flag = 0;
    DrainOnExit drain(c);   // genes and partner_mask in, partner and code out (declared after the buffers: the wait comes before their release)
    REO_HIP_CHECK(hipMemcpyAsync(d_genes.p, genes, n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    if ((rc = mask.upload(c, partner_mask))) return rc;
    if ((rc = launch_pair_count(c, d_genes.p, n_genes, mask.bits, class_mask, d_count.p))) return rc;
    REO_HIP_CHECK(hipMemcpyAsync(count.data(), d_count.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if ((rc = wait_or_drop_table(c))) return rc;
    for (size_t q = 0; q < n; ++q)
        if (count[q] < 0 || count[q] >= c->G) { set_error("reo_pair_list: the count of query %zu reads %d with %lld genes", q, count[q], (long long)c->G); return REO_EHIP; }
    const int64_t total = pair_list_rowptr(count.data(), n_genes, rowptr);
    if (!partner || total == 0) { drain.dismiss(); return REO_OK; }
    if (total > capacity) {
        set_error("reo_pair_list: the lists hold %lld entries, capacity is %lld (rowptr has been filled: allocate rowptr[n_genes] entries)",
                  (long long)total, (long long)capacity);
        return REO_EINVAL;
    }
    const size_t nt = static_cast<size_t>(total);
    if ((rc = d_rowptr.ensure(n + 1)) || (rc = d_partner.ensure(nt)) || (rc = d_code.ensure(nt)) || (rc = d_flag.ensure(1))) return rc;
    REO_HIP_CHECK(hipMemcpyAsync(d_rowptr.p, rowptr, (n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    REO_HIP_CHECK(hipMemsetAsync(d_flag.p, 0, sizeof(int32_t), c->stream));
    if ((rc = launch_pair_fill(c, d_genes.p, n_genes, mask.bits, class_mask, d_rowptr.p, d_partner.p, d_code.p, total, d_flag.p))) return rc;
    if ((rc = copy_back(c, partner, 0, d_partner.p, nt)) || (rc = copy_back(c, code, 0, d_code.p, nt)) || (rc = copy_back(c, &flag, 0, d_flag.p, 1)))
        return rc;
    if ((rc = wait_or_drop_table(c))) return rc;
    drain.dismiss();
    if (flag) {
        set_error("reo_pair_list: the fill pass found another number of pairs in a row than the count pass (the class table changed between them?); "
                  "the lists are not valid");
        return REO_EHIP;
    }
    return REO_OK;
}

// In which samples (include/reo_hip.h): the queries in batches whose two count buffers stay under the budget of sample_counts.h; per batch one
// launch and the copies of its rows into the caller's arrays.  Reads the class table, the bit planes and a reference mask slot; writes none of them.
int32_t reo_sample_counts(reo_ctx *c, const int32_t *genes, int64_t n_genes, const uint8_t *partner_mask, uint32_t class_mask, int32_t *n_sel,
                          int32_t *n_gt, int32_t *n_eq)
{
    int32_t rc = begin_query(c, "reo_sample_counts", true);
    if (rc || (rc = refuse_under_mask(c, "reo_sample_counts"))) return rc;
    char msg[320];
    if (sample_counts_check_args(c->G, genes, n_genes, class_mask, n_gt, msg, sizeof msg)) { set_error("%s", msg); return REO_EINVAL; }
    if ((rc = need_partner_set(c, "reo_sample_counts", partner_mask))) return rc;
    if ((rc = ensure_transform(c))) return rc;   // (in place whenever there is a class table: nothing runs)
    std::vector<int32_t> map;
    if ((rc = query_slot_map(c, "reo_sample_counts", map))) return rc;
    const size_t S = static_cast<size_t>(c->S), slots = map.size();
    const int64_t batch = sc_batch_rows(n_genes, static_cast<int64_t>(slots), env_batch("REO_SAMPLE_COUNTS_BATCH"));
    const size_t nb = static_cast<size_t>(batch);
    DevBuf<int32_t> d_genes, d_sel, d_gt, d_eq;
    PartnerMask mask;
    if ((rc = d_genes.ensure(nb)) || (rc = d_sel.ensure(nb)) || (rc = d_gt.ensure(nb * slots)) || (n_eq && (rc = d_eq.ensure(nb * slots))) ||
        (rc = c->sc_slot2col.ensure(slots)) || (rc = mask.prepare(c, partner_mask)))
        return rc;
    DrainOnExit drain(c);   // genes and partner_mask in, the counts out (declared after the buffers: the wait comes before their release)
    if ((rc = upload_slot2col(c, map)) || (rc = mask.upload(c, partner_mask))) return rc;
    for (int64_t q0 = 0; q0 < n_genes; q0 += batch) {
        const int64_t nq = std::min(batch, n_genes - q0);
        const size_t at = static_cast<size_t>(q0), nrow = static_cast<size_t>(nq);
        REO_HIP_CHECK(hipMemcpyAsync(d_genes.p, genes + q0, nrow * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        if ((rc = launch_sample_counts(c, d_genes.p, nq, mask.bits, class_mask, c->sc_slot2col.p, d_sel.p, d_gt.p, n_eq ? d_eq.p : nullptr))) return rc;
        if ((rc = copy_back(c, n_gt, at * S, d_gt.p, nrow * S)) || (rc = copy_back(c, n_eq, at * S, d_eq.p, nrow * S)) ||
            (rc = copy_back(c, n_sel, at, d_sel.p, nrow)))
            return rc;
        if ((rc = wait_or_drop_table(c))) return rc;   // the next batch reuses the buffers
    }
    drain.dismiss();
    return REO_OK;
}

// Up or down in one sample (include/reo_hip.h): the queries in batches; per batch two launches of the counting kernel of reo_sample_counts
// (class masks 0x1C0 and 0x007, with tied counts) into device buffers that stay there, one launch of k_sample_fisher (sampletests.hip)
// over them, and the copies of the batch's rows into the caller's arrays.  Reads the class table, the bit planes and a reference mask
// slot; writes none of them.
int32_t reo_sample_tests(reo_ctx *c, const int32_t *genes, int64_t n_genes, const uint8_t *partner_mask, int32_t *n_above_ctrl,
                         int32_t *n_below_ctrl, int32_t *rev_up, int32_t *rev_down, int32_t *tied, double *p_up, double *p_down)
{
    int32_t rc = begin_query(c, "reo_sample_tests", true);
    if (rc || (rc = refuse_under_mask(c, "reo_sample_tests"))) return rc;
    char msg[320];
    if (sample_tests_check_args(c->G, genes, n_genes, p_up, p_down, msg, sizeof msg)) { set_error("%s", msg); return REO_EINVAL; }
    if ((rc = need_partner_set(c, "reo_sample_tests", partner_mask))) return rc;
    if ((rc = ensure_transform(c))) return rc;   // (in place whenever there is a class table: nothing runs)
    std::vector<int32_t> map;
    if ((rc = query_slot_map(c, "reo_sample_tests", map))) return rc;
    const size_t S = static_cast<size_t>(c->S), slots = map.size();
    const int64_t batch = st_batch_rows(n_genes, static_cast<int64_t>(slots), env_batch("REO_SAMPLE_TESTS_BATCH"));
    const size_t nb = static_cast<size_t>(batch), cells = nb * S;
    const int64_t lf_entries = st_lf_entries(c->G);
    DevBuf<int32_t> d_genes, d_sel_a, d_sel_b, d_gt_a, d_eq_a, d_gt_b, d_eq_b, d_rev_up, d_rev_down, d_tied, d_flag;
    DevBuf<double> d_p_up, d_p_down;
    PartnerMask mask;
    if ((rc = d_genes.ensure(nb)) || (rc = d_sel_a.ensure(nb)) || (rc = d_sel_b.ensure(nb)) || (rc = d_gt_a.ensure(nb * slots)) ||
        (rc = d_eq_a.ensure(nb * slots)) || (rc = d_gt_b.ensure(nb * slots)) || (rc = d_eq_b.ensure(nb * slots)) ||
        (rev_up && (rc = d_rev_up.ensure(cells))) || (rev_down && (rc = d_rev_down.ensure(cells))) || (tied && (rc = d_tied.ensure(cells))) ||
        (rc = d_p_up.ensure(cells)) || (rc = d_p_down.ensure(cells)) || (rc = d_flag.ensure(1)) || (rc = c->sc_slot2col.ensure(slots)) ||
        (rc = c->st_lf.ensure(static_cast<size_t>(lf_entries))) || (rc = mask.prepare(c, partner_mask)))
        return rc;
    std::vector<double> lf;
    int32_t flag = 0;
    DrainOnExit drain(c);   // genes, partner_mask and lf in, the results out (declared after the buffers: the wait comes before their release)
    if (c->st_lf_G != c->G) {   // once per context and gene count
        st_build_lf(c->G, lf);
        c->st_lf_G = -1;
        REO_HIP_CHECK(hipMemcpyAsync(c->st_lf.p, lf.data(), lf.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
        REO_HIP_CHECK(hipStreamSynchronize(c->stream));   // (lf is a local)
        c->st_lf_G = c->G;
    }
    if ((rc = upload_slot2col(c, map)) || (rc = mask.upload(c, partner_mask))) return rc;
    REO_HIP_CHECK(hipMemsetAsync(d_flag.p, 0, sizeof(int32_t), c->stream));
    for (int64_t q0 = 0; q0 < n_genes; q0 += batch) {
        const int64_t nq = std::min(batch, n_genes - q0);
        const size_t at = static_cast<size_t>(q0), nrow = static_cast<size_t>(nq);
        REO_HIP_CHECK(hipMemcpyAsync(d_genes.p, genes + q0, nrow * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        if ((rc = launch_sample_counts(c, d_genes.p, nq, mask.bits, kStMaskAbove, c->sc_slot2col.p, d_sel_a.p, d_gt_a.p, d_eq_a.p)) ||
            (rc = launch_sample_counts(c, d_genes.p, nq, mask.bits, kStMaskBelow, c->sc_slot2col.p, d_sel_b.p, d_gt_b.p, d_eq_b.p)) ||
            (rc = launch_sample_fisher(c, nq, d_sel_a.p, d_sel_b.p, d_gt_a.p, d_eq_a.p, d_gt_b.p, d_eq_b.p, c->st_lf.p, lf_entries,
                                       rev_up ? d_rev_up.p : nullptr, rev_down ? d_rev_down.p : nullptr, tied ? d_tied.p : nullptr, d_p_up.p,
                                       d_p_down.p, d_flag.p)))
            return rc;
        if ((rc = copy_back(c, n_above_ctrl, at, d_sel_a.p, nrow)) || (rc = copy_back(c, n_below_ctrl, at, d_sel_b.p, nrow)) ||
            (rc = copy_back(c, rev_up, at * S, d_rev_up.p, nrow * S)) || (rc = copy_back(c, rev_down, at * S, d_rev_down.p, nrow * S)) ||
            (rc = copy_back(c, tied, at * S, d_tied.p, nrow * S)) || (rc = copy_back(c, p_up, at * S, d_p_up.p, nrow * S)) ||
            (rc = copy_back(c, p_down, at * S, d_p_down.p, nrow * S)) || (rc = copy_back(c, &flag, 0, d_flag.p, 1)))
            return rc;
        if ((rc = wait_or_drop_table(c))) return rc;   // the next batch reuses the buffers
        if (flag) {
            set_error("reo_sample_tests: the counting kernel delivered counts that %lld genes cannot produce; the results are not valid", (long long)c->G);
            return REO_EHIP;
        }
    }
    drain.dismiss();
    return REO_OK;
}

// The calls themselves (include/reo_hip.h): phase 1 is reo_sample_tests' batch loop with nothing copied back -- the two counting launches
// and k_sample_fisher into the batch's buffers, then k_call_rank (samplecalls.hip) turns the batch's tails into the cell words of
// sample_calls.h, stored by sample into a buffer that stays for the whole call; phase 2, k_call_cut, finds every sample column's
// Benjamini-Hochberg cut from a histogram of the ranks; phase 3, k_call_emit, stores the int8 calls, which come back in one copy.  The
// batches follow each other on the stream without a host wait: the query genes go up once.  Reads the class table, the bit planes and a
// reference mask slot; writes none of them.
int32_t reo_sample_calls(reo_ctx *c, const int32_t *genes, int64_t n_genes, const uint8_t *partner_mask, double pval_deg, double padj_deg,
                         int8_t *calls, int32_t *cut, int32_t *n_up, int32_t *n_down)
{
    int32_t rc = begin_query(c, "reo_sample_calls", true);
    if (rc || (rc = refuse_under_mask(c, "reo_sample_calls"))) return rc;
    char msg[320];
    if (sample_calls_check_args(c->G, genes, n_genes, pval_deg, padj_deg, calls, msg, sizeof msg)) { set_error("%s", msg); return REO_EINVAL; }
    if ((rc = need_partner_set(c, "reo_sample_calls", partner_mask))) return rc;
    if ((rc = ensure_transform(c))) return rc;   // (in place whenever there is a class table: nothing runs)
    std::vector<int32_t> map;
    if ((rc = query_slot_map(c, "reo_sample_calls", map))) return rc;
    const size_t S = static_cast<size_t>(c->S), slots = map.size(), n = static_cast<size_t>(n_genes);
    const int64_t batch = call_batch_rows(n_genes, static_cast<int64_t>(slots), env_batch("REO_SAMPLE_CALLS_BATCH"));
    const size_t nb = static_cast<size_t>(batch), cells = nb * S;
    const int64_t lf_entries = st_lf_entries(c->G);
    const int64_t need = call_device_bytes(n_genes, c->S, static_cast<int64_t>(slots), batch);
    size_t free_bytes = 0, total_bytes = 0;
    REO_HIP_CHECK(hipMemGetInfo(&free_bytes, &total_bytes));
    if (need < 0 || static_cast<uint64_t>(need) > free_bytes) {
        set_error("reo_sample_calls: %lld queries x %lld samples need %lld bytes of device memory (%lld of them the resident cell words), %zu are "
                  "free: query fewer genes per call", (long long)n_genes, (long long)c->S, (long long)need,
                  (long long)(4 * call_padded_rows(n_genes) * c->S), free_bytes);
        return REO_ENOMEM;
    }
    DevBuf<int32_t> d_genes, d_sel_a, d_sel_b, d_gt_a, d_eq_a, d_gt_b, d_eq_b, d_flag, d_kstar, d_cut, d_up, d_down;
    DevBuf<double> d_p_up, d_p_down;
    DevBuf<uint32_t> d_words;
    DevBuf<int8_t> d_calls;
    PartnerMask mask;
    if ((rc = d_genes.ensure(n)) || (rc = d_sel_a.ensure(nb)) || (rc = d_sel_b.ensure(nb)) || (rc = d_gt_a.ensure(nb * slots)) ||
        (rc = d_eq_a.ensure(nb * slots)) || (rc = d_gt_b.ensure(nb * slots)) || (rc = d_eq_b.ensure(nb * slots)) ||
        (rc = d_p_up.ensure(cells)) || (rc = d_p_down.ensure(cells)) || (rc = d_flag.ensure(1)) || (rc = d_kstar.ensure(S)) ||
        (rc = d_cut.ensure(S)) || (rc = d_up.ensure(S)) || (rc = d_down.ensure(S)) ||
        (rc = d_words.ensure(static_cast<size_t>(call_padded_rows(n_genes)) * S)) || (rc = d_calls.ensure(n * S)) ||
        (rc = c->sc_slot2col.ensure(slots)) || (rc = c->st_lf.ensure(static_cast<size_t>(lf_entries))) || (rc = mask.prepare(c, partner_mask)))
        return rc;
    std::vector<double> lf;
    int32_t flag = 0;
    DrainOnExit drain(c);   // genes, partner_mask and lf in, the calls out (declared after the buffers: the wait comes before their release)
    if (c->st_lf_G != c->G) {   // once per context and gene count, shared with reo_sample_tests
        st_build_lf(c->G, lf);
        c->st_lf_G = -1;
        REO_HIP_CHECK(hipMemcpyAsync(c->st_lf.p, lf.data(), lf.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
        REO_HIP_CHECK(hipStreamSynchronize(c->stream));   // (lf is a local)
        c->st_lf_G = c->G;
    }
    if ((rc = upload_slot2col(c, map)) || (rc = mask.upload(c, partner_mask))) return rc;
    REO_HIP_CHECK(hipMemsetAsync(d_flag.p, 0, sizeof(int32_t), c->stream));
    REO_HIP_CHECK(hipMemcpyAsync(d_genes.p, genes, n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    for (int64_t q0 = 0; q0 < n_genes; q0 += batch) {   // phase 1 (the stream orders the batches: they share the batch's buffers)
        const int64_t nq = std::min(batch, n_genes - q0);
        const int32_t *g = d_genes.p + q0;
        if ((rc = launch_sample_counts(c, g, nq, mask.bits, kStMaskAbove, c->sc_slot2col.p, d_sel_a.p, d_gt_a.p, d_eq_a.p)) ||
            (rc = launch_sample_counts(c, g, nq, mask.bits, kStMaskBelow, c->sc_slot2col.p, d_sel_b.p, d_gt_b.p, d_eq_b.p)) ||
            (rc = launch_sample_fisher(c, nq, d_sel_a.p, d_sel_b.p, d_gt_a.p, d_eq_a.p, d_gt_b.p, d_eq_b.p, c->st_lf.p, lf_entries, nullptr, nullptr,
                                       nullptr, d_p_up.p, d_p_down.p, d_flag.p)) ||
            (rc = launch_call_rank(c, n_genes, q0, nq, d_p_up.p, d_p_down.p, pval_deg, padj_deg, d_words.p)))
            return rc;
    }
    if ((rc = launch_call_cut(c, n_genes, d_words.p, d_kstar.p, d_cut.p, d_up.p, d_down.p)) ||   // phase 2
        (rc = launch_call_emit(c, n_genes, d_words.p, d_kstar.p, d_calls.p)))                     // phase 3
        return rc;
    if ((rc = copy_back(c, &flag, 0, d_flag.p, 1)) || (rc = wait_or_drop_table(c))) return rc;
    if (flag) {   // before anything of the caller's is written
        set_error("reo_sample_calls: the counting kernel delivered counts that %lld genes cannot produce; no call was written", (long long)c->G);
        return REO_EHIP;
    }
    if ((rc = copy_back(c, calls, 0, d_calls.p, n * S)) || (rc = copy_back(c, cut, 0, d_cut.p, S)) || (rc = copy_back(c, n_up, 0, d_up.p, S)) ||
        (rc = copy_back(c, n_down, 0, d_down.p, S)))
        return rc;
    if ((rc = wait_or_drop_table(c))) return rc;
    drain.dismiss();
    return REO_OK;
}

// How strongly (include/reo_hip.h): every check on the host first (pair_support.h), then the entries in batches whose count buffers and
// outcome buffer stay under the budget; per batch the work items and the partners go up, one launch, and the batch's rows come back into
// the caller's arrays.  Reads the bit planes of the transform and nothing of the class table or the iteration; writes none of them.
int32_t reo_pair_support(reo_ctx *c, const int32_t *genes, int64_t n_genes, const int64_t *rowptr, const int32_t *partner, int32_t *n_gt,
                         int32_t *n_eq, uint8_t *outcome)
{
    int32_t rc = begin_query(c, "reo_pair_support", false);
    if (rc || (rc = refuse_under_mask(c, "reo_pair_support"))) return rc;
    if (c->dtype == 0 || c->group_id.empty() || static_cast<int64_t>(c->group_id.size()) != c->S) return ensure_transform(c);   // (its refusals: nothing runs)
    char msg[320];
    if (pair_support_check_args(c->G, genes, n_genes, rowptr, partner, n_gt, msg, sizeof msg)) { set_error("%s", msg); return REO_EINVAL; }
    const int64_t total = rowptr[n_genes];
    if (total == 0) return REO_OK;   // nothing listed: no transform, no launch
    if ((rc = ensure_transform(c))) return rc;
    const size_t S = static_cast<size_t>(c->S), ng = static_cast<size_t>(c->ngroups);
    std::vector<int32_t> map;
    if (outcome && (rc = query_slot_map(c, "reo_pair_support", map))) return rc;
    const int64_t batch = ps_batch_entries(total, c->ngroups, c->S, outcome != nullptr, env_batch("REO_PAIR_SUPPORT_BATCH"));
    const size_t nb = static_cast<size_t>(batch);
    DevBuf<PsItem> d_items;
    DevBuf<int32_t> d_partner, d_gt, d_eq;
    DevBuf<uint8_t> d_out;
    if ((rc = d_items.ensure(nb)) || (rc = d_partner.ensure(nb)) || (rc = d_gt.ensure(nb * ng)) || (n_eq && (rc = d_eq.ensure(nb * ng))) ||
        (outcome && ((rc = d_out.ensure(nb * S)) || (rc = c->sc_slot2col.ensure(map.size())))))
        return rc;
    std::vector<PsItem> items;
    DrainOnExit drain(c);   // items and partners in, counts and outcomes out (declared after the buffers: the wait comes before their release)
    if (outcome && (rc = upload_slot2col(c, map))) return rc;
    int64_t row = 0;
    for (int64_t e0 = 0; e0 < total; e0 += batch) {
        const int64_t ne = std::min(batch, total - e0);
        ps_build_items(genes, rowptr, n_genes, e0, e0 + ne, &row, items);
        if (items.empty() || static_cast<int64_t>(items.size()) > ne) { set_error("reo_pair_support: %zu work items for %lld entries", items.size(), (long long)ne); return REO_EHIP; }
        const size_t at = static_cast<size_t>(e0), n = static_cast<size_t>(ne);
        REO_HIP_CHECK(hipMemcpyAsync(d_items.p, items.data(), items.size() * sizeof(PsItem), hipMemcpyHostToDevice, c->stream));
        REO_HIP_CHECK(hipMemcpyAsync(d_partner.p, partner + e0, n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        if ((rc = launch_pair_support(c, d_items.p, static_cast<int64_t>(items.size()), d_partner.p, outcome ? c->sc_slot2col.p : nullptr, d_gt.p,
                                      n_eq ? d_eq.p : nullptr, outcome ? d_out.p : nullptr)))
            return rc;
        if ((rc = copy_back(c, n_gt, at * ng, d_gt.p, n * ng)) || (rc = copy_back(c, n_eq, at * ng, d_eq.p, n * ng)) ||
            (rc = copy_back(c, outcome, at * S, d_out.p, n * S)))
            return rc;
        if ((rc = wait_or_drop_table(c))) return rc;   // the next batch reuses the buffers and the item list
    }
    drain.dismiss();
    return REO_OK;
}

// The rank shift of every gene (include/reo_hip.h): the checks, the sides, one launch of k_rank_shift, G values back.
int32_t reo_rank_shift(reo_ctx *c, int32_t a, int32_t b, int64_t *D)
{
    int32_t rc = top_begin(c, "reo_rank_shift");
    if (rc) return rc;
    char msg[320];
    if (tp_check_shift_args(top_state(c), a, b, D, msg, sizeof msg)) { set_error("%s", msg); return REO_EINVAL; }
    TopSides sides;
    DevBuf<int32_t> d_gside;
    DevBuf<int64_t> d_D;
    if ((rc = sides.make(c, "reo_rank_shift", a, b)) || (rc = ensure_transform(c)) || (rc = d_gside.ensure(sides.gside.size())) ||
        (rc = d_D.ensure(static_cast<size_t>(c->Gp))))
        return rc;
    DrainOnExit drain(c);   // the sides in, D out (declared after the buffers: the wait comes before their release)
    REO_HIP_CHECK(hipMemcpyAsync(d_gside.p, sides.gside.data(), sides.gside.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    if ((rc = launch_rank_shift(c, d_gside.p, sides.s_a, sides.s_b, d_D.p)) || (rc = copy_back(c, D, 0, d_D.p, static_cast<size_t>(c->G))) ||
        (rc = wait_or_drop_table(c)))
        return rc;
    drain.dismiss();
    return REO_OK;
}

// The best n_want of all pairs (include/reo_hip.h): every check on the host first (top_pairs.h), then D, the pass loop of tp_select with
// k_top_pairs<HIST> as its histogram, one emit pass, and the host sort of the candidates by the full key.  Reads the bit planes of the
// transform and nothing of the class table or the iteration; writes none of them.
int32_t reo_top_pairs(reo_ctx *c, int32_t a, int32_t b, const uint8_t *gene_mask, int64_t n_want, int32_t *gene_i, int32_t *gene_j,
                      int32_t *counts, int64_t *key, int64_t *n_found, int32_t *passes_run)
{
    int32_t rc = top_begin(c, "reo_top_pairs");
    if (rc) return rc;
    char msg[320];
    if (tp_check_args(top_state(c), a, b, gene_mask, n_want, gene_i, gene_j, counts, key, n_found, msg, sizeof msg)) { set_error("%s", msg); return REO_EINVAL; }
    TopSides sides;
    if ((rc = sides.make(c, "reo_top_pairs", a, b)) || (rc = ensure_transform(c))) return rc;
    const int G = static_cast<int>(c->G);
    const int64_t capacity = tp_capacity(n_want, env_batch("REO_TOP_PAIRS_CAP"));
    std::vector<uint32_t> bits;
    if (gene_mask) {
        bits.assign(static_cast<size_t>(c->Wp), 0u);
        for (int g = 0; g < G; ++g)
            if (gene_mask[g]) bits[static_cast<size_t>(g) >> 5] |= 1u << (g & 31);
    }
    DevBuf<int32_t> d_gside;
    DevBuf<int64_t> d_D;
    DevBuf<uint32_t> d_bits, d_cand_n;
    DevBuf<unsigned long long> d_hist;
    DevBuf<TpRec> d_cand;
    if ((rc = d_gside.ensure(sides.gside.size())) || (rc = d_D.ensure(static_cast<size_t>(c->Gp))) || (gene_mask && (rc = d_bits.ensure(bits.size()))) ||
        (rc = d_hist.ensure(kTpHistWords)) || (rc = d_cand.ensure(static_cast<size_t>(capacity))) || (rc = d_cand_n.ensure(1)))
        return rc;
    TimedPair ev;   // (reo_get_info 36, 37: what the passes cost on the device)
    if ((rc = ev.make())) return rc;
    std::vector<int64_t> D(static_cast<size_t>(G));
    std::vector<unsigned long long> hist(kTpHistWords);
    std::vector<TpRec> cand;
    uint32_t n_cand = 0;
    DrainOnExit drain(c);   // the sides and the mask in, D, histograms and candidates out (declared after the buffers: the wait comes before their release)
    REO_HIP_CHECK(hipMemcpyAsync(d_gside.p, sides.gside.data(), sides.gside.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    if (gene_mask) REO_HIP_CHECK(hipMemcpyAsync(d_bits.p, bits.data(), bits.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    const uint32_t *maskbits = gene_mask ? d_bits.p : nullptr;
    if ((rc = launch_rank_shift(c, d_gside.p, sides.s_a, sides.s_b, d_D.p)) || (rc = copy_back(c, D.data(), 0, d_D.p, D.size())) ||
        (rc = wait_or_drop_table(c)))
        return rc;
    const auto mm = std::minmax_element(D.begin(), D.end());
    const uint64_t n_max = 2 * static_cast<uint64_t>(sides.s_a) * static_cast<uint64_t>(sides.s_b), g_max = static_cast<uint64_t>(*mm.second - *mm.first);
    if (n_max >> 31 || g_max >> kTpGammaBits) {
        set_error("reo_top_pairs: the rank shifts span %llu and 2 S_A S_B is %llu: more than the key's 48 and 31 bits hold", (unsigned long long)g_max,
                  (unsigned long long)n_max);
        return REO_EHIP;
    }
    c->top_hist_us = 0; c->top_emit_us = 0;
    int32_t hist_rc = REO_OK;
    const auto run_hist = [&](const TpKey &prefix, int shift, uint64_t *out) -> int {
        if (hipMemsetAsync(d_hist.p, 0, kTpHistWords * sizeof(unsigned long long), c->stream) != hipSuccess) { set_error("reo_top_pairs: the histogram could not be cleared"); hist_rc = REO_EHIP; return 1; }
        if ((hist_rc = ev.start(c)) || (hist_rc = launch_top_hist(c, d_gside.p, sides.s_a, sides.s_b, d_D.p, maskbits, prefix, shift, d_hist.p)) ||
            (hist_rc = ev.stop(c)) || (hist_rc = copy_back(c, hist.data(), 0, d_hist.p, hist.size())) || (hist_rc = wait_or_drop_table(c)) ||
            (hist_rc = ev.add_us(&c->top_hist_us)))
            return 1;
        for (int w = 0; w < kTpHistWords; ++w) out[w] = hist[static_cast<size_t>(w)];
        return 0;
    };
    TpSelect sel;
    const int src = tp_select(run_hist, tp_bound_mask(n_max, g_max), static_cast<uint64_t>(n_want), static_cast<uint64_t>(capacity), &sel);
    if (src > 0) return hist_rc;
    if (src < 0 || sel.n_cand > static_cast<uint64_t>(capacity)) {
        set_error("reo_top_pairs: pass %d counted other pairs above its prefix than the passes before it (%llu candidates for %lld records)", sel.passes,
                  (unsigned long long)sel.n_cand, (long long)capacity);
        return REO_EHIP;
    }
    if (sel.n_cand > 0) {
        cand.resize(static_cast<size_t>(sel.n_cand));
        REO_HIP_CHECK(hipMemsetAsync(d_cand_n.p, 0, sizeof(uint32_t), c->stream));
        if ((rc = ev.start(c)) || (rc = launch_top_emit(c, d_gside.p, sides.s_a, sides.s_b, d_D.p, maskbits, sel.cut, sel.shift, d_cand.p, capacity, d_cand_n.p)) ||
            (rc = ev.stop(c)) || (rc = copy_back(c, &n_cand, 0, d_cand_n.p, 1)) || (rc = copy_back(c, cand.data(), 0, d_cand.p, cand.size())) ||
            (rc = wait_or_drop_table(c)) || (rc = ev.add_us(&c->top_emit_us)))
            return rc;
    }
    drain.dismiss();
    if (n_cand != sel.n_cand) {
        set_error("reo_top_pairs: the emit pass found %u candidates, the histogram passes counted %llu; nothing was written", n_cand,
                  (unsigned long long)sel.n_cand);
        return REO_EHIP;
    }
    std::vector<std::pair<TpKey, uint32_t>> order(cand.size());
    for (size_t e = 0; e < cand.size(); ++e) {
        const TpRec &r = cand[e];
        if (r.i < 0 || r.i >= r.j || r.j >= G) { set_error("reo_top_pairs: candidate %zu is the pair (%d, %d) with %d genes; nothing was written", e, r.i, r.j, G); return REO_EHIP; }
        order[e] = {tp_rec_key(r, D.data(), G, sides.s_a, sides.s_b), static_cast<uint32_t>(e)};
    }
    std::sort(order.begin(), order.end(), [](const std::pair<TpKey, uint32_t> &x, const std::pair<TpKey, uint32_t> &y) { return tp_before(x.first, y.first); });
    const size_t n_out = std::min(order.size(), static_cast<size_t>(n_want));
    for (size_t e = 0; e < n_out; ++e) {
        const TpRec &r = cand[order[e].second];
        gene_i[e] = r.i; gene_j[e] = r.j;
        counts[4 * e] = r.gt_a; counts[4 * e + 1] = r.eq_a; counts[4 * e + 2] = r.gt_b; counts[4 * e + 3] = r.eq_b;
        key[2 * e] = tp_num(r.gt_a, r.eq_a, r.gt_b, r.eq_b, sides.s_a, sides.s_b);
        key[2 * e + 1] = static_cast<int64_t>(tp_gamma(D[static_cast<size_t>(r.i)], D[static_cast<size_t>(r.j)]));
    }
    *n_found = static_cast<int64_t>(n_out);
    if (passes_run) *passes_run = sel.passes;
    return REO_OK;
}

// The null of the best score (include/reo_hip.h): every check on the host first (top_pairs_null.h), then per batch of at most 64 label
// rows the A-words, one launch of k_top_pairs_null and the batch's keys and counters back.  Reads the bit planes of the transform and
// nothing of the class table or the iteration; writes none of them.  The caller's arrays are written once every batch has run.
int32_t reo_top_pairs_null(reo_ctx *c, int32_t a, int32_t b, const uint8_t *sides, int64_t n_perm, const uint8_t *gene_mask, const int64_t *cuts,
                           int32_t n_cuts, int64_t *max_n, int32_t *arg_i, int32_t *arg_j, int64_t *n_reach)
{
    const char *what = "reo_top_pairs_null";
    int32_t rc = top_begin(c, what);
    if (rc) return rc;
    char msg[320];
    int64_t s_a = 0, s_b = 0;
    if (tn_check_args(top_state(c), c->group_id.data(), a, b, sides, n_perm, gene_mask, cuts, n_cuts, max_n, arg_i, arg_j, n_reach, &s_a, &s_b, msg,
                      sizeof msg)) {
        set_error("%s", msg);
        return REO_EINVAL;
    }
    std::vector<int32_t> map;
    if ((rc = ensure_transform(c)) || (rc = query_slot_map(c, what, map))) return rc;
    const int G = static_cast<int>(c->G);
    const size_t S = static_cast<size_t>(c->S);
    const int nblk = c->goff32.back() / 32;
    const int64_t P = tn_batch(n_perm, env_batch("REO_TOP_NULL_BATCH"));
    std::vector<uint32_t> bits;
    if (gene_mask) {
        bits.assign(static_cast<size_t>(c->Wp), 0u);
        for (int g = 0; g < G; ++g)
            if (gene_mask[g]) bits[static_cast<size_t>(g) >> 5] |= 1u << (g & 31);
    }
    DevBuf<uint8_t> d_side;
    DevBuf<uint32_t> d_aw, d_live, d_bits;
    DevBuf<unsigned long long> d_keys, d_reach;
    if ((rc = d_side.ensure(static_cast<size_t>(P) * S)) || (rc = d_aw.ensure(pn_word_count(P, nblk))) || (rc = d_live.ensure(static_cast<size_t>(nblk))) ||
        (gene_mask && (rc = d_bits.ensure(bits.size()))) || (rc = d_keys.ensure(kTnBatchCap)) || (rc = d_reach.ensure(kTnBatchCap * kTnMaxCuts)) ||
        (rc = c->sc_slot2col.ensure(map.size())))
        return rc;
    TimedPair ev;   // (reo_get_info 39: what the launches cost on the device)
    if ((rc = ev.make())) return rc;
    std::vector<unsigned long long> keys(static_cast<size_t>(n_perm)), reach(static_cast<size_t>(n_perm) * kTnMaxCuts);
    DrainOnExit drain(c);   // the rows and the mask in, keys and counters out (declared after the buffers: the wait comes before their release)
    if ((rc = upload_slot2col(c, map))) return rc;
    if (gene_mask) REO_HIP_CHECK(hipMemcpyAsync(d_bits.p, bits.data(), bits.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    c->top_null_batch = P; c->top_null_us = 0;
    for (int64_t p0 = 0; p0 < n_perm; p0 += P) {
        const int np = static_cast<int>(std::min<int64_t>(P, n_perm - p0));
        REO_HIP_CHECK(hipMemcpyAsync(d_side.p, sides + static_cast<size_t>(p0) * S, static_cast<size_t>(np) * S, hipMemcpyHostToDevice, c->stream));
        REO_HIP_CHECK(hipMemsetAsync(d_keys.p, 0, kTnBatchCap * sizeof(unsigned long long), c->stream));
        REO_HIP_CHECK(hipMemsetAsync(d_reach.p, 0, kTnBatchCap * kTnMaxCuts * sizeof(unsigned long long), c->stream));
        if ((rc = launch_top_null_words(c, d_side.p, np, c->sc_slot2col.p, d_aw.p, d_live.p)) || (rc = ev.start(c)) ||
            (rc = launch_top_pairs_null(c, d_aw.p, d_live.p, np, static_cast<int>(s_a), static_cast<int>(s_b), gene_mask ? d_bits.p : nullptr, cuts, n_cuts,
                                        d_keys.p, d_reach.p)) ||
            (rc = ev.stop(c)) || (rc = copy_back(c, keys.data(), static_cast<size_t>(p0), d_keys.p, static_cast<size_t>(np))) ||
            (rc = copy_back(c, reach.data(), static_cast<size_t>(p0) * kTnMaxCuts, d_reach.p, static_cast<size_t>(np) * kTnMaxCuts)) ||
            (rc = wait_or_drop_table(c)) || (rc = ev.add_us(&c->top_null_us)))   // (the next batch reuses the buffers)
            return rc;
    }
    drain.dismiss();
    for (int64_t p = 0; p < n_perm; ++p) {
        int64_t m = -1;
        int32_t gi = -1, gj = -1;
        tn_unpack(keys[static_cast<size_t>(p)], G, &m, &gi, &gj);
        if (m >= 0 && !(gi >= 0 && gi < gj && gj < G && m <= 2 * s_a * s_b)) {
            set_error("%s: permutation %lld reduced to the pair (%d, %d) with |N| = %lld of %d genes; nothing was written", what, (long long)p, gi, gj,
                      (long long)m, G);
            return REO_EHIP;
        }
    }
    for (int64_t p = 0; p < n_perm; ++p) {
        tn_unpack(keys[static_cast<size_t>(p)], G, &max_n[p], &arg_i[p], &arg_j[p]);
        for (int t = 0; t < n_cuts; ++t) n_reach[p * n_cuts + t] = static_cast<int64_t>(reach[static_cast<size_t>(p) * kTnMaxCuts + static_cast<size_t>(t)]);
    }
    return REO_OK;
}

// Leave-one-out cross-validation of the k-TSP selection (include/reo_hip.h): every check on the host first (top_pairs_loo.h).  Step 1: the
// full-data list of reo_top_pairs itself, deepened until its greedy disjoint walk yields 2 kmax pairs, gives the cut T (loo_cut).  Step 2:
// the emit pass of k_top_pairs with the cut on the |N| field of the key leaves every pair with |N| >= T on the device; a counter past the
// buffer sizes a second emit.  Step 3: k_loo_words; step 4: k_loo_select, one workgroup per fold (toppairsloo.hip).  Reads the bit planes
// of the transform and nothing of the class table or the iteration; writes none of them.  The caller's arrays are written at the end.
int32_t reo_top_pairs_loo(reo_ctx *c, int32_t a, int32_t b, const uint8_t *gene_mask, int32_t kmax, int32_t *gene_i, int32_t *gene_j, int64_t *num,
                          int64_t *rank_num, int8_t *outcome, int8_t *side, int64_t *stats)
{
    const char *what = "reo_top_pairs_loo";
    int32_t rc = top_begin(c, what);
    if (rc) return rc;
    char msg[320];
    if (loo_check_args(top_state(c), a, b, gene_mask, kmax, gene_i, gene_j, num, rank_num, outcome, side, stats, msg, sizeof msg)) { set_error("%s", msg); return REO_EINVAL; }
    TopSides sides;
    sides.count(c, a, b);
    if (loo_check_sides(sides.s_a, sides.s_b, msg, sizeof msg)) { set_error("%s", msg); return REO_EINVAL; }
    std::vector<int32_t> map;
    if ((rc = ensure_transform(c)) || (rc = query_slot_map(c, what, map))) return rc;
    const int G = static_cast<int>(c->G);
    const size_t S = static_cast<size_t>(c->S), cells = S * static_cast<size_t>(kmax);
    const int nblk = c->goff32.back() / 32;
    const uint64_t n_max = 2 * static_cast<uint64_t>(sides.s_a) * static_cast<uint64_t>(sides.s_b);
    if (n_max >> 31) { set_error("%s: 2 S_A S_B is %llu: more than the key's 31 bits hold", what, (unsigned long long)n_max); return REO_EHIP; }
    // step 1: the cut
    int64_t cut = 0, passes = 0;
    const char *all = getenv("REO_TOP_PAIRS_LOO_ALL");
    if (!(all && atoi(all) == 1)) {
        const int64_t hist_us = c->top_hist_us, emit_us = c->top_emit_us;   // (reo_get_info 36 / 37 belong to the caller's last reo_top_pairs)
        std::vector<int32_t> li, lj, lc;
        std::vector<int64_t> lk;
        for (int64_t n_want = kLooFirstWant; ; n_want *= 2) {
            const size_t n = static_cast<size_t>(n_want);
            li.resize(n); lj.resize(n); lc.resize(4 * n); lk.resize(2 * n);
            int64_t found = 0, last = -1;
            int32_t run = 0;
            rc = reo_top_pairs(c, a, b, gene_mask, n_want, li.data(), lj.data(), lc.data(), lk.data(), &found, &run);
            c->top_hist_us = hist_us; c->top_emit_us = emit_us;
            if (rc) return rc;
            passes += run;
            if (loo_disjoint(li.data(), lj.data(), found, G, 2 * static_cast<int64_t>(kmax), &last) >= 2 * static_cast<int64_t>(kmax)) {
                cut = loo_cut(static_cast<int64_t>(tp_abs(lk[2 * static_cast<size_t>(last)])), sides.s_a, sides.s_b);
                break;
            }
            if (found < n_want || n_want >= kTpMaxWant) break;   // every eligible pair is listed, or the deepest list: T = 0
        }
    }
    std::vector<uint32_t> bits;
    if (gene_mask) {
        bits.assign(static_cast<size_t>(c->Wp), 0u);
        for (int g = 0; g < G; ++g)
            if (gene_mask[g]) bits[static_cast<size_t>(g) >> 5] |= 1u << (g & 31);
    }
    const int64_t cap = loo_capacity(env_batch("REO_TOP_PAIRS_LOO_CAP"));
    int64_t have = loo_first_records(cap, env_batch("REO_TOP_PAIRS_LOO_FIRST"));
    DevBuf<int32_t> d_gside, d_oi, d_oj;
    DevBuf<int64_t> d_D, d_sums, d_on, d_og;
    DevBuf<int8_t> d_oo;
    DevBuf<uint32_t> d_bits, d_cand_n;
    DevBuf<TpRec> d_cand;
    DevBuf<uint2> d_words;
    if ((rc = d_gside.ensure(sides.gside.size())) || (rc = d_D.ensure(static_cast<size_t>(c->Gp))) || (rc = d_sums.ensure(2 * static_cast<size_t>(c->Gp))) ||
        (gene_mask && (rc = d_bits.ensure(bits.size()))) || (rc = d_cand.ensure(static_cast<size_t>(have))) || (rc = d_cand_n.ensure(1)) ||
        (rc = d_oi.ensure(cells)) || (rc = d_oj.ensure(cells)) || (rc = d_on.ensure(cells)) || (rc = d_og.ensure(cells)) || (rc = d_oo.ensure(cells)) ||
        (rc = c->sc_slot2col.ensure(map.size())))
        return rc;
    TimedPair ev_words, ev_select;   // (reo_get_info 40, 41: what the two kernels cost on the device)
    if ((rc = ev_words.make()) || (rc = ev_select.make())) return rc;
    std::vector<int32_t> h_i(cells), h_j(cells);
    std::vector<int64_t> h_n(cells), h_g(cells);
    std::vector<int8_t> h_o(cells);
    uint32_t n_cand = 0;
    DrainOnExit drain(c);   // the sides and the mask in, the counter and the picks out (declared after the buffers: the wait comes before their release)
    REO_HIP_CHECK(hipMemcpyAsync(d_gside.p, sides.gside.data(), sides.gside.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    if (gene_mask) REO_HIP_CHECK(hipMemcpyAsync(d_bits.p, bits.data(), bits.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    const uint32_t *maskbits = gene_mask ? d_bits.p : nullptr;
    if ((rc = upload_slot2col(c, map)) || (rc = launch_rank_shift(c, d_gside.p, sides.s_a, sides.s_b, d_D.p, d_sums.p))) return rc;
    // step 2: the candidates; the cut sits on the |N| field of the key
    const TpKey ref{0, static_cast<uint64_t>(cut)};
    const int shift = kTpGammaBits + 32;
    REO_HIP_CHECK(hipMemsetAsync(d_cand_n.p, 0, sizeof(uint32_t), c->stream));
    if ((rc = launch_top_emit(c, d_gside.p, sides.s_a, sides.s_b, d_D.p, maskbits, ref, shift, d_cand.p, have, d_cand_n.p)) ||
        (rc = copy_back(c, &n_cand, 0, d_cand_n.p, 1)) || (rc = wait_or_drop_table(c)))
        return rc;
    size_t free_bytes = 0, total_bytes = 0;
    REO_HIP_CHECK(hipMemGetInfo(&free_bytes, &total_bytes));
    if (loo_check_count(n_cand, cut, cap, nblk, static_cast<uint64_t>(free_bytes) + static_cast<uint64_t>(have) * sizeof(TpRec), msg, sizeof msg)) {
        set_error("%s", msg);
        return REO_ENOMEM;
    }
    if (n_cand > have) {   // the counter ran past the buffer: size it from the counter and emit again
        uint32_t again = 0;
        have = n_cand;
        if ((rc = d_cand.ensure(static_cast<size_t>(have)))) return rc;
        REO_HIP_CHECK(hipMemsetAsync(d_cand_n.p, 0, sizeof(uint32_t), c->stream));
        if ((rc = launch_top_emit(c, d_gside.p, sides.s_a, sides.s_b, d_D.p, maskbits, ref, shift, d_cand.p, have, d_cand_n.p)) ||
            (rc = copy_back(c, &again, 0, d_cand_n.p, 1)) || (rc = wait_or_drop_table(c)))
            return rc;
        if (again != n_cand) { set_error("%s: the second emit pass found %u candidates, the first %u; nothing was written", what, again, n_cand); return REO_EHIP; }
    }
    // the rows of samples that are no folds, and the picks that a fold does not have
    REO_HIP_CHECK(hipMemsetAsync(d_oi.p, 0xFF, cells * sizeof(int32_t), c->stream));
    REO_HIP_CHECK(hipMemsetAsync(d_oj.p, 0xFF, cells * sizeof(int32_t), c->stream));
    REO_HIP_CHECK(hipMemsetAsync(d_on.p, 0, cells * sizeof(int64_t), c->stream));
    REO_HIP_CHECK(hipMemsetAsync(d_og.p, 0, cells * sizeof(int64_t), c->stream));
    REO_HIP_CHECK(hipMemsetAsync(d_oo.p, 0, cells, c->stream));
    c->top_loo_words_us = 0; c->top_loo_select_us = 0;
    if (n_cand > 0) {
        if ((rc = d_words.ensure(static_cast<size_t>(n_cand) * static_cast<size_t>(nblk)))) return rc;
        if ((rc = ev_words.start(c)) || (rc = launch_loo_words(c, d_cand.p, n_cand, d_words.p)) || (rc = ev_words.stop(c)) ||   // step 3
            (rc = ev_select.start(c)) ||
            (rc = launch_loo_select(c, d_cand.p, n_cand, d_words.p, d_gside.p, c->sc_slot2col.p, d_sums.p, sides.s_a, sides.s_b, kmax, d_oi.p, d_oj.p,
                                    d_on.p, d_og.p, d_oo.p)) ||                                                                   // step 4
            (rc = ev_select.stop(c)))
            return rc;
    }
    if ((rc = copy_back(c, h_i.data(), 0, d_oi.p, cells)) || (rc = copy_back(c, h_j.data(), 0, d_oj.p, cells)) ||
        (rc = copy_back(c, h_n.data(), 0, d_on.p, cells)) || (rc = copy_back(c, h_g.data(), 0, d_og.p, cells)) ||
        (rc = copy_back(c, h_o.data(), 0, d_oo.p, cells)) || (rc = wait_or_drop_table(c)))
        return rc;
    drain.dismiss();
    if (n_cand > 0 && ((rc = ev_words.add_us(&c->top_loo_words_us)) || (rc = ev_select.add_us(&c->top_loo_select_us)))) return rc;
    for (size_t e = 0; e < cells; ++e)
        if (h_i[e] != -1 && !(h_i[e] >= 0 && h_i[e] < h_j[e] && h_j[e] < G && h_o[e] >= -1 && h_o[e] <= 1)) {
            set_error("%s: fold %zu picked the pair (%d, %d) with %d genes; nothing was written", what, e / static_cast<size_t>(kmax), h_i[e], h_j[e], G);
            return REO_EHIP;
        }
    std::copy(h_i.begin(), h_i.end(), gene_i); std::copy(h_j.begin(), h_j.end(), gene_j);
    std::copy(h_n.begin(), h_n.end(), num); std::copy(h_g.begin(), h_g.end(), rank_num);
    std::copy(h_o.begin(), h_o.end(), outcome);
    for (size_t s = 0; s < S; ++s) {
        const int32_t g = c->group_id[s];
        side[s] = static_cast<int8_t>((g < 0 || g >= c->ngroups) ? 2 : (sides.gside[static_cast<size_t>(g)] == 0 ? 1 : (sides.gside[static_cast<size_t>(g)] == 1 ? 0 : 2)));
    }
    stats[0] = cut; stats[1] = n_cand; stats[2] = passes; stats[3] = static_cast<int64_t>(sides.s_a) + sides.s_b;
    return REO_OK;
}

// The best partners of given genes (include/reo_hip.h): every check on the host first (top_partners.h), then D, and per batch of query rows
// one launch of k_top_partners_count into the batch's cells, one of k_top_partners_select over them, and the batch's rows back into the
// caller's arrays.  Reads the bit planes of the transform and nothing of the class table or the iteration; writes none of them.
int32_t reo_top_partners(reo_ctx *c, int32_t a, int32_t b, const int32_t *genes, int64_t n_genes, const uint8_t *partner_mask, int32_t m_want,
                         int32_t *partner, int32_t *counts, int64_t *key, int32_t *n_found)
{
    const char *what = "reo_top_partners";
    int32_t rc = top_begin(c, what);
    if (rc) return rc;
    char msg[320];
    if (tpr_check_args(top_state(c), a, b, genes, n_genes, partner_mask, m_want, partner, counts, key, n_found, msg, sizeof msg)) { set_error("%s", msg); return REO_EINVAL; }
    TopSides sides;
    if ((rc = sides.make(c, what, a, b)) || (rc = ensure_transform(c))) return rc;
    const int G = static_cast<int>(c->G);
    const size_t m = static_cast<size_t>(m_want), padded = static_cast<size_t>(tpr_padded_rows(n_genes));
    std::vector<uint32_t> bits;
    if (partner_mask) {
        bits.assign(static_cast<size_t>(c->Wp), 0u);
        for (int g = 0; g < G; ++g)
            if (partner_mask[g]) bits[static_cast<size_t>(g) >> 5] |= 1u << (g & 31);
    }
    std::vector<int32_t> rows(padded, 0);   // (the rows that fill the last tile walk gene 0; nothing of them is selected)
    std::copy(genes, genes + n_genes, rows.begin());
    DevBuf<int32_t> d_gside, d_genes, d_partner, d_counts, d_found;
    DevBuf<int64_t> d_D, d_key;
    DevBuf<uint32_t> d_bits;
    DevBuf<unsigned long long> d_cells;
    if ((rc = d_gside.ensure(sides.gside.size())) || (rc = d_D.ensure(static_cast<size_t>(c->Gp))) || (rc = d_genes.ensure(padded)) ||
        (partner_mask && (rc = d_bits.ensure(bits.size()))))
        return rc;
    size_t free_bytes = 0, total_bytes = 0;
    REO_HIP_CHECK(hipMemGetInfo(&free_bytes, &total_bytes));
    const int64_t batch = tpr_batch_rows(n_genes, c->Gp, m_want, static_cast<uint64_t>(free_bytes), env_batch("REO_TOP_PARTNERS_BATCH"));
    const size_t nb = static_cast<size_t>(batch);
    if ((rc = d_cells.ensure(nb * static_cast<size_t>(c->Gp))) || (rc = d_partner.ensure(nb * m)) || (rc = d_counts.ensure(4 * nb * m)) ||
        (rc = d_key.ensure(2 * nb * m)) || (rc = d_found.ensure(nb)))
        return rc;
    TimedPair ev_count, ev_select;   // (reo_get_info 42, 43: what the two kernels cost on the device)
    if ((rc = ev_count.make()) || (rc = ev_select.make())) return rc;
    DrainOnExit drain(c);   // the sides, the genes and the mask in, the rows out (declared after the buffers: the wait comes before their release)
    REO_HIP_CHECK(hipMemcpyAsync(d_gside.p, sides.gside.data(), sides.gside.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    REO_HIP_CHECK(hipMemcpyAsync(d_genes.p, rows.data(), padded * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    if (partner_mask) REO_HIP_CHECK(hipMemcpyAsync(d_bits.p, bits.data(), bits.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    const uint32_t *maskbits = partner_mask ? d_bits.p : nullptr;
    if ((rc = launch_rank_shift(c, d_gside.p, sides.s_a, sides.s_b, d_D.p))) return rc;
    c->top_partners_count_us = 0; c->top_partners_select_us = 0;
    for (int64_t q0 = 0; q0 < n_genes; q0 += batch) {
        const int64_t nq = std::min(batch, n_genes - q0);
        const size_t at = static_cast<size_t>(q0), nrow = static_cast<size_t>(nq);
        const int32_t *g = d_genes.p + q0;   // (q0 is a multiple of kTpRows: the padded rows of this batch follow its own)
        if ((rc = ev_count.start(c)) || (rc = launch_top_partners_count(c, d_gside.p, sides.s_a, sides.s_b, g, tpr_padded_rows(nq), d_cells.p)) ||
            (rc = ev_count.stop(c)) || (rc = ev_select.start(c)) ||
            (rc = launch_top_partners_select(c, d_cells.p, g, nq, d_D.p, maskbits, sides.s_a, sides.s_b, m_want, d_partner.p, d_counts.p, d_key.p,
                                             d_found.p)) ||
            (rc = ev_select.stop(c)) || (rc = copy_back(c, partner, at * m, d_partner.p, nrow * m)) ||
            (rc = copy_back(c, counts, 4 * at * m, d_counts.p, 4 * nrow * m)) || (rc = copy_back(c, key, 2 * at * m, d_key.p, 2 * nrow * m)) ||
            (rc = copy_back(c, n_found, at, d_found.p, nrow)) || (rc = wait_or_drop_table(c)) ||   // (the next batch reuses the buffers)
            (rc = ev_count.add_us(&c->top_partners_count_us)) || (rc = ev_select.add_us(&c->top_partners_select_us)))
            return rc;
    }
    drain.dismiss();
    return REO_OK;
}

// The null of a gene's best partner (include/reo_hip.h): every check on the host first (top_partners_null.h), then per batch of at most 64
// label rows the A-words of reo_top_pairs_null, one launch of k_top_partners_null over all query rows and the batch's keys and counters
// back.  Reads the bit planes of the transform and nothing of the class table or the iteration; writes none of them.  The caller's arrays
// are written once every batch has run and every key has been found plausible.
int32_t reo_top_partners_null(reo_ctx *c, int32_t a, int32_t b, const uint8_t *sides, int64_t n_perm, const int32_t *genes, int64_t n_genes,
                              const uint8_t *partner_mask, const int64_t *cuts, int64_t *max_n, int32_t *arg_p, int32_t *n_reach)
{
    const char *what = "reo_top_partners_null";
    int32_t rc = top_begin(c, what);
    if (rc) return rc;
    char msg[320];
    int64_t s_a = 0, s_b = 0;
    if (tprn_check_args(top_state(c), c->group_id.data(), a, b, sides, n_perm, genes, n_genes, partner_mask, cuts, max_n, arg_p, n_reach, &s_a, &s_b, msg,
                        sizeof msg)) {
        set_error("%s", msg);
        return REO_EINVAL;
    }
    std::vector<int32_t> map;
    if ((rc = ensure_transform(c)) || (rc = query_slot_map(c, what, map))) return rc;
    const int G = static_cast<int>(c->G);
    const size_t S = static_cast<size_t>(c->S), nq = static_cast<size_t>(n_genes), padded = static_cast<size_t>(tprn_padded_rows(n_genes));
    const int nblk = c->goff32.back() / 32;
    std::vector<uint32_t> bits;
    if (partner_mask) {
        bits.assign(static_cast<size_t>(c->Wp), 0u);
        for (int g = 0; g < G; ++g)
            if (partner_mask[g]) bits[static_cast<size_t>(g) >> 5] |= 1u << (g & 31);
    }
    std::vector<int32_t> rows(padded, 0);   // (the rows that fill the last tile walk gene 0; nothing of them is stored)
    std::copy(genes, genes + n_genes, rows.begin());
    std::vector<uint32_t> cutw(cuts ? padded : 0, 0xFFFFFFFFu);
    for (size_t r = 0; cuts && r < nq; ++r) cutw[r] = tprn_cut_word(cuts[r]);
    DevBuf<uint8_t> d_side;
    DevBuf<int32_t> d_genes;
    DevBuf<uint32_t> d_aw, d_live, d_bits, d_cuts, d_reach;
    DevBuf<unsigned long long> d_keys;
    if ((rc = d_genes.ensure(padded)) || (rc = d_live.ensure(static_cast<size_t>(nblk))) || (partner_mask && (rc = d_bits.ensure(bits.size()))) ||
        (cuts && (rc = d_cuts.ensure(padded))) || (rc = c->sc_slot2col.ensure(map.size())))
        return rc;
    size_t free_bytes = 0, total_bytes = 0;
    REO_HIP_CHECK(hipMemGetInfo(&free_bytes, &total_bytes));
    const int64_t P = tprn_batch(n_perm, n_genes, static_cast<uint64_t>(free_bytes), env_batch("REO_TOP_PARTNERS_NULL_BATCH"));
    const size_t cells = static_cast<size_t>(P) * padded;
    if ((rc = d_side.ensure(static_cast<size_t>(P) * S)) || (rc = d_aw.ensure(pn_word_count(P, nblk))) || (rc = d_keys.ensure(cells)) ||
        (rc = d_reach.ensure(cells)))
        return rc;
    TimedPair ev;   // (reo_get_info 45: what the launches cost on the device)
    if ((rc = ev.make())) return rc;
    std::vector<unsigned long long> keys(static_cast<size_t>(n_perm) * padded);   // (rows of `padded` cells, as they lie on the device)
    std::vector<uint32_t> reach(cuts ? keys.size() : 0);
    DrainOnExit drain(c);   // the rows, the genes, the cuts and the mask in, keys and counters out (declared after the buffers: the wait comes before their release)
    if ((rc = upload_slot2col(c, map))) return rc;
    REO_HIP_CHECK(hipMemcpyAsync(d_genes.p, rows.data(), padded * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    if (partner_mask) REO_HIP_CHECK(hipMemcpyAsync(d_bits.p, bits.data(), bits.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    if (cuts) REO_HIP_CHECK(hipMemcpyAsync(d_cuts.p, cutw.data(), padded * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    c->top_partners_null_batch = P; c->top_partners_null_us = 0;
    for (int64_t p0 = 0; p0 < n_perm; p0 += P) {
        const int np = static_cast<int>(std::min<int64_t>(P, n_perm - p0));
        const size_t at = static_cast<size_t>(p0) * padded, n = static_cast<size_t>(np) * padded;
        REO_HIP_CHECK(hipMemcpyAsync(d_side.p, sides + static_cast<size_t>(p0) * S, static_cast<size_t>(np) * S, hipMemcpyHostToDevice, c->stream));
        REO_HIP_CHECK(hipMemsetAsync(d_keys.p, 0, n * sizeof(unsigned long long), c->stream));
        REO_HIP_CHECK(hipMemsetAsync(d_reach.p, 0, n * sizeof(uint32_t), c->stream));
        if ((rc = launch_top_null_words(c, d_side.p, np, c->sc_slot2col.p, d_aw.p, d_live.p)) || (rc = ev.start(c)) ||
            (rc = launch_top_partners_null(c, d_aw.p, d_live.p, np, static_cast<int>(s_a), static_cast<int>(s_b), d_genes.p, n_genes,
                                           partner_mask ? d_bits.p : nullptr, cuts ? d_cuts.p : nullptr, d_keys.p, d_reach.p)) ||
            (rc = ev.stop(c)) || (rc = copy_back(c, keys.data(), at, d_keys.p, n)) ||
            (cuts && (rc = copy_back(c, reach.data(), at, d_reach.p, n))) || (rc = wait_or_drop_table(c)) ||
            (rc = ev.add_us(&c->top_partners_null_us)))   // (the next batch reuses the buffers)
            return rc;
    }
    drain.dismiss();
    for (int64_t p = 0; p < n_perm; ++p)
        for (size_t r = 0; r < nq; ++r) {
            int64_t m = -1;
            int32_t gp = -1;
            tprn_unpack(keys[static_cast<size_t>(p) * padded + r], &m, &gp);
            if (m >= 0 && !(gp >= 0 && gp < G && gp != genes[r] && m <= 2 * s_a * s_b)) {
                set_error("%s: permutation %lld, row %lld (gene %d) reduced to the partner %d with |N| = %lld of %d genes; nothing was written", what,
                          (long long)p, (long long)r, genes[r], gp, (long long)m, G);
                return REO_EHIP;
            }
        }
    for (int64_t p = 0; p < n_perm; ++p)
        for (size_t r = 0; r < nq; ++r) {
            const size_t from = static_cast<size_t>(p) * padded + r, to = static_cast<size_t>(p) * nq + r;
            tprn_unpack(keys[from], &max_n[to], &arg_p[to]);
            if (cuts) n_reach[to] = static_cast<int32_t>(reach[from]);
        }
    return REO_OK;
}

}  // extern "C"
