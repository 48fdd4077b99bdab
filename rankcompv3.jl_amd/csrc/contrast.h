// Pairwise group contrasts (reo_build_pairs_contrast): the class table of "group ctrl against group treat" of a run with more than two
// groups, classified from the per-group count planes that the one-vs-rest comparisons share (kernels.hip, k1_classify_contrast) -- nothing
// is counted again.  What the API and a host driver share, so that the driver can evaluate the very same functions under the sanitizers
// (tests/contrast_driver.cpp): the argument checks with their messages, which all run before anything of the context is touched, and the
// two sides of the comparison -- their sample blocks, sizes and thresholds -- from the group offsets and the threshold matrix.
// No HIP header in here: plain C++17.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>

namespace reo {

// What the checks look at (reo_ctx has more; the driver fills this by hand).
struct ContrastState {
    int32_t ngroups;        // reo_set_groups (0: none set)
    bool thr_set;           // reo_compute_thresholds / reo_set_thresholds
    bool multi_device;      // a reo_create_multi context, leader or peer
    int64_t S;              // samples (0: no matrix yet)
    bool share_counts;      // REO_SHARE_GROUP_COUNTS is not 0
    bool planes_fit;        // the count planes are resident, or device memory has room for them ...
    int64_t planes_bytes;   // ... and their size
};

// Argument checks of reo_build_pairs_contrast.  0 when everything is in order; otherwise the number of the failed check (1 ..) and its
// message in msg.  Checks 1 - 4 need the group count only; 5 and 6 the state of the context; 7 - 9 apply to more than two groups (two
// groups are a reo_build_pairs and need no planes).
inline int contrast_check_args(bool have_ctx, const ContrastState &st, int32_t ctrl, int32_t treat, char *msg, size_t msg_n)
{
    if (!have_ctx) { snprintf(msg, msg_n, "reo_build_pairs_contrast: null context"); return 1; }
    if (ctrl < 0 || ctrl >= st.ngroups) {
        snprintf(msg, msg_n, "reo_build_pairs_contrast: ctrl = %d is outside [0, %d) (the groups of reo_set_groups)", ctrl, st.ngroups);
        return 2;
    }
    if (treat < 0 || treat >= st.ngroups) {
        snprintf(msg, msg_n, "reo_build_pairs_contrast: treat = %d is outside [0, %d) (the groups of reo_set_groups)", treat, st.ngroups);
        return 3;
    }
    if (ctrl == treat) { snprintf(msg, msg_n, "reo_build_pairs_contrast: ctrl = treat = %d, a contrast needs two different groups", ctrl); return 4; }
    if (!st.thr_set) { snprintf(msg, msg_n, "reo_build_pairs_contrast: thresholds not set (reo_compute_thresholds, reo_set_thresholds)"); return 5; }
    if (st.multi_device) {
        snprintf(msg, msg_n, "reo_build_pairs_contrast: not available on a reo_create_multi context (one context per device: reo_create, reo_set_shard)");
        return 6;
    }
    if (st.ngroups == 2) return 0;
    if (st.S > 65535) {
        snprintf(msg, msg_n, "reo_build_pairs_contrast: no shared per-group counts with more than 65535 samples (%lld; the count planes are 16-bit), "
                             "and a contrast is classified from them", (long long)st.S);
        return 7;
    }
    if (!st.share_counts) {
        snprintf(msg, msg_n, "reo_build_pairs_contrast: no shared per-group counts, REO_SHARE_GROUP_COUNTS=0 is set in the environment, and a contrast "
                             "is classified from them");
        return 8;
    }
    if (!st.planes_fit) {
        snprintf(msg, msg_n, "reo_build_pairs_contrast: the per-group count planes do not fit the free device memory (%lld bytes needed for %d groups), "
                             "and a contrast is classified from them", (long long)st.planes_bytes, st.ngroups);
        return 9;
    }
    return 0;
}

// The two sides of contrast (ctrl, treat): their ranges in 32-sample blocks, their sizes and their thresholds.
struct ContrastSides {
    int cb, ce, tb, te;   // ctrl / treat blocks of the sorted sample order
    int nc, nt;           // S_ctrl, S_treat
    int m1, m2;           // thr[0, ctrl], thr[0, treat]: row 0 of the threshold matrix, each group's own size (row 1, "the rest", is not used)
};

// goff: [ngroups + 1] offsets of the groups in the sorted sample order; goff32: the same with every group padded to whole blocks of 32
// slots; thr: the 2 x ngroups threshold matrix, column-major (thr[2 g] = row 0 of group g).  ctrl and treat have passed the checks.
inline ContrastSides contrast_sides(const int32_t *goff, const int32_t *goff32, const int32_t *thr, int32_t ctrl, int32_t treat)
{
    ContrastSides s;
    s.cb = goff32[ctrl] / 32; s.ce = goff32[ctrl + 1] / 32;
    s.tb = goff32[treat] / 32; s.te = goff32[treat + 1] / 32;
    s.nc = goff[ctrl + 1] - goff[ctrl];
    s.nt = goff[treat + 1] - goff[treat];
    s.m1 = thr[2 * ctrl];
    s.m2 = thr[2 * treat];
    return s;
}

}  // namespace reo
