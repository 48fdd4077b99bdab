// Host half of reo_filter_matrix (filter.hip): the reference's low-expression filters, src/RankCompV3.jl:618 (profiles) then :626
// (genes), from the two count vectors that the device makes to the kept flags, the source-index lists of the gather and the verdict.
// Plain C++, no HIP: tests/filter_maps_driver.cpp runs it as a program of its own under the sanitizers.
#pragma once

#include <cstdint>
#include <vector>

#ifdef __HIPCC__
#define REO_FM_HD __host__ __device__
#else
#define REO_FM_HD
#endif

namespace reo {

// `x > 0` of the element type, decided on the value's bits as a signed integer of its width, so that no floating-point mode (flushed
// subnormals) has a say: an Int64 is positive iff bits > 0; a Float64 / Float32 iff bits > 0 (sign clear, not +0: subnormals count) and
// bits <= the bits of +Inf (above them lie the NaNs, for which every comparison is false).  -0.0 and negatives have the sign bit set.
constexpr int64_t kPosLimitI64 = INT64_MAX;
constexpr int64_t kPosLimitF64 = 0x7FF0000000000000LL;
constexpr int32_t kPosLimitF32 = 0x7F800000;
template <class W>
REO_FM_HD inline bool positive_bits(W bits, W limit) { return bits > 0 && bits <= limit; }

// kept[i] = counts[i] > min_count (strict, as :618 / :626 write it); returns how many are kept.  kept may be null.
inline int64_t filter_flags(const int32_t *counts, int64_t n, int64_t min_count, uint8_t *kept)
{
    int64_t k = 0;
    for (int64_t i = 0; i < n; ++i) {
        const bool on = static_cast<int64_t>(counts[i]) > min_count;
        if (kept) kept[i] = on ? 1 : 0;
        k += on ? 1 : 0;
    }
    return k;
}

struct FilterMaps {
    std::vector<int32_t> src_col;    // [S'] column of the old matrix that becomes column s'
    std::vector<int32_t> src_gene;   // [G'] row of the old matrix that becomes row g'
    int64_t S_kept = 0, G_kept = 0;
    bool identity = false;           // nothing dropped: the matrix stays where it is
    bool too_small = false;          // G' < 2 or S' < 2: no matrix that reo_set_matrix_* would take
};

// counts = [S column counts][G gene counts] as the device delivers them (the gene counts run over the kept columns only: the device
// applies the same `> min_profiles` to the column counts that filter_flags applies here).  Order is preserved.
inline FilterMaps filter_maps(const int32_t *counts, int64_t S, int64_t G, int64_t min_profiles, int64_t min_features,
                              uint8_t *profile_kept, uint8_t *gene_kept)
{
    FilterMaps m;
    m.S_kept = filter_flags(counts, S, min_profiles, profile_kept);
    m.G_kept = filter_flags(counts + S, G, min_features, gene_kept);
    m.identity = m.S_kept == S && m.G_kept == G;
    m.too_small = m.S_kept < 2 || m.G_kept < 2;
    if (m.identity || m.too_small) return m;
    m.src_col.reserve(static_cast<size_t>(m.S_kept));
    m.src_gene.reserve(static_cast<size_t>(m.G_kept));
    for (int64_t s = 0; s < S; ++s)
        if (static_cast<int64_t>(counts[s]) > min_profiles) m.src_col.push_back(static_cast<int32_t>(s));
    for (int64_t g = 0; g < G; ++g)
        if (static_cast<int64_t>(counts[S + g]) > min_features) m.src_gene.push_back(static_cast<int32_t>(g));
    return m;
}

}  // namespace reo
