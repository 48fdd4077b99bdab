// reo_sample_tests: per query gene and sample, Fisher's exact test of the sample's orderings against the pairs that are stable in the
// control group.  The counting is launch_sample_counts' (samplecounts.hip, twice: class masks 0x1C0 and 0x007, both with tied counts);
// this unit turns its six device counts into the two hypergeometric tails.
//   k_sample_fisher   one thread per (query, sample) of the batch, consecutive threads on consecutive samples of a query row: every load
//                     and store of the [batch][S] arrays is coalesced.  st_table (sample_tests.h) forms the 2 x 2 table and refuses
//                     counts that G genes cannot produce; st_tails reads the log-factorial table at indices <= N <= 2 (G - 1) only.
// Addresses: o = q * S + s < n_queries * S of the launch; q < n_queries for the per-query counts; the table index is bounded above.  A
// refused table stores NaN and raises the flag that the host answers REO_EHIP on; nothing is indexed with it.
#include "sample_tests.h"
#include "reo_internal.h"

namespace reo {

namespace {

constexpr int kStThreads = 256;

struct StArgs {
    const int32_t *sel_a, *sel_b, *gt_a, *eq_a, *gt_b, *eq_b;
    const double *lf;
    int32_t *rev_up, *rev_down, *tied, *flag;
    double *p_up, *p_down;
    int64_t total, lf_entries;   // n_queries * S
    int G, S;
};

__global__ __launch_bounds__(kStThreads) void k_sample_fisher(StArgs a)
{
    const int64_t o = static_cast<int64_t>(blockIdx.x) * kStThreads + threadIdx.x;
    if (o >= a.total) return;
    const int64_t q = o / a.S;
    StTable t;
    double up = NAN, down = NAN;
    if (st_table(a.G, a.sel_a[q], a.sel_b[q], a.gt_a[o], a.eq_a[o], a.gt_b[o], a.eq_b[o], &t)) {
        st_tails(a.lf, a.lf_entries, t.a, t.b, t.u, t.d, &up, &down);
    } else {
        t.rev_up = t.rev_down = t.tied = -1;
        atomicOr(a.flag, 1);
    }
    if (a.rev_up) a.rev_up[o] = t.rev_up;
    if (a.rev_down) a.rev_down[o] = t.rev_down;
    if (a.tied) a.tied[o] = t.tied;
    a.p_up[o] = up;
    a.p_down[o] = down;
}

}  // namespace

int32_t launch_sample_fisher(reo_ctx *c, int64_t n_queries, const int32_t *d_sel_a, const int32_t *d_sel_b, const int32_t *d_gt_a,
                             const int32_t *d_eq_a, const int32_t *d_gt_b, const int32_t *d_eq_b, const double *d_lf, int64_t lf_entries,
                             int32_t *d_rev_up, int32_t *d_rev_down, int32_t *d_tied, double *d_p_up, double *d_p_down, int32_t *d_flag)
{
    StArgs a;
    a.sel_a = d_sel_a; a.sel_b = d_sel_b; a.gt_a = d_gt_a; a.eq_a = d_eq_a; a.gt_b = d_gt_b; a.eq_b = d_eq_b;
    a.lf = d_lf; a.lf_entries = lf_entries;
    a.rev_up = d_rev_up; a.rev_down = d_rev_down; a.tied = d_tied; a.flag = d_flag;
    a.p_up = d_p_up; a.p_down = d_p_down;
    a.G = static_cast<int>(c->G); a.S = static_cast<int>(c->S);
    a.total = n_queries * c->S;
    const int64_t grid = (a.total + kStThreads - 1) / kStThreads;
    if (n_queries < 1 || c->S < 1 || lf_entries < st_lf_entries(c->G) || grid > 0x7FFFFFFF) {
        set_error("reo_sample_tests: a batch of %lld queries x %lld samples cannot be launched", (long long)n_queries, (long long)c->S);
        return REO_EINVAL;
    }
    k_sample_fisher<<<dim3(static_cast<unsigned>(grid)), kStThreads, 0, c->stream>>>(a);
    REO_HIP_CHECK(hipGetLastError());
    return REO_OK;
}

}  // namespace reo
