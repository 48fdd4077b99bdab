"""Host-side mirror of the reference's hot-path interface.

`identify_degs` has the reference's positional signature
(/root/reference/src/RankCompV3.jl:339-350) and returns the same G x 17
matrix of [gene_name, 15 Float64 statistics, label] (:430,437); everything
numeric happens in libreo_hip.so on the GPU.  The Julia shim a maintainer
would drop into the reference (julia/RankCompV3HIP.jl) is the same ~60 lines
in Julia.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import NamedTuple

import numpy as np

from . import _ffi, synth
from ._ffi import PairList, PairSupport, PermNull, SampleCalls, SampleCounts, SampleScores, SampleTests, TopPairs, TopPairsLoo, TopPairsNull, TopPartners, TopPartnersNull, class_mask, permuted_labels, permuted_sides  # noqa: F401

HEADER = ["pval", "padj", "n11", "n12", "n13", "n21", "n22", "n23", "n31", "n32", "n33",
          "Δ1", "Δ2", "se", "z1", "up_down"]  # src/RankCompV3.jl:665


def encode_groups(group):
    """unique(group) in first-appearance order (src/RankCompV3.jl:353,357) -> (ids, levels)."""
    levels: list = []
    index: dict = {}
    ids = np.empty(len(group), dtype=np.int32)
    for s, g in enumerate(group):
        key = g.item() if isinstance(g, np.generic) else g
        if key not in index:
            index[key] = len(levels)
            levels.append(key)
        ids[s] = index[key]
    return ids, levels


def parse_contrasts(levels, contrasts) -> list:
    """The contrasts of a run as (ctrl, treat) index pairs into `levels` (encode_groups' order).  "all": every unordered pair of levels, the
    level that appears first as control, in level order.  Otherwise a sequence of (ctrl_level, treat_level) pairs, kept in the order given.
    Raises DimensionMismatch -- before any context is opened -- for an unknown level, ctrl == treat, an empty list and the same ordered
    contrast twice."""
    n = len(levels)
    if isinstance(contrasts, str):
        if contrasts != "all":
            raise _ffi.DimensionMismatch(_ffi.REO_EINVAL, f"contrasts: {contrasts!r} is not \"all\" and not a sequence of (ctrl, treat) level pairs")
        out = [(a, b) for a in range(n) for b in range(a + 1, n)]
    else:
        index = {lv: q for q, lv in enumerate(levels)}
        out = []
        for item in contrasts:
            pair = tuple(item)
            if len(pair) != 2:
                raise _ffi.DimensionMismatch(_ffi.REO_EINVAL, f"contrasts: {item!r} is not a (ctrl, treat) pair of levels")
            ids = []
            for lv in pair:
                key = lv.item() if isinstance(lv, np.generic) else lv
                if key not in index:
                    raise _ffi.DimensionMismatch(_ffi.REO_EINVAL, f"contrasts: unknown level {key!r} (the levels of 'group' are {list(levels)!r})")
                ids.append(index[key])
            if ids[0] == ids[1]:
                raise _ffi.DimensionMismatch(_ffi.REO_EINVAL, f"contrasts: ctrl == treat == {pair[0]!r}, a contrast needs two different levels")
            if (ids[0], ids[1]) in out:
                raise _ffi.DimensionMismatch(_ffi.REO_EINVAL, f"contrasts: ({pair[0]!r}, {pair[1]!r}) is listed twice")
            out.append((ids[0], ids[1]))
    if not out:
        raise _ffi.DimensionMismatch(_ffi.REO_EINVAL, "contrasts: the list is empty (None runs the comparisons of the reference)")
    return out


def comparison_plan(levels, contrasts) -> list:
    """What a run builds, in order: (k, treat) per comparison -- treat None: comparison k of the reference (one for two groups, else one per
    group against every other sample); with `contrasts`: parse_contrasts' pairs."""
    if contrasts is None:
        return [(k, None) for k in range(1 if len(levels) == 2 else len(levels))]
    return parse_contrasts(levels, contrasts)


def build_comparison(ctx, levels, k, treat) -> dict:
    """Builds the class table of one entry of comparison_plan on `ctx` and starts its comparison dict."""
    if treat is None:
        ctx.build_pairs(k)
        return {"k": k}
    ctx.build_contrast(k, treat)
    return {"k": k, "ctrl": levels[k], "treat": levels[treat]}


def label_genes(result: np.ndarray, pval_deg: float, padj_deg: float) -> np.ndarray:
    """up / down / no change, src/RankCompV3.jl:426-429."""
    sig = (result[:, 0] <= pval_deg) & (result[:, 1] <= padj_deg)
    out = np.full(result.shape[0], "no change", dtype=object)
    out[sig & (result[:, 14] > 0)] = "up"
    out[sig & (result[:, 14] < 0)] = "down"
    return out


@dataclass
class DegRun:
    """Everything the comparisons produced (the reference only keeps `res`)."""
    result: np.ndarray              # G x 15 Float64 of the first comparison
    labels: np.ndarray              # labels of the first comparison
    levels: list
    thresholds: np.ndarray          # 2 x ngroups (:362)
    iters_run: int
    trace: list = field(default_factory=list)   # (#DEG, #non-DEG) per pass (:418), first comparison
    timings: dict = field(default_factory=dict)
    info: dict = field(default_factory=dict)
    comparisons: list = field(default_factory=list)  # per comparison: dict(k, result, labels, iters_run, trace); contrasts: ctrl, treat too
    gene_names: object = None
    _res: object = None

    @property
    def res(self) -> np.ndarray:
        """G x (1 + 16 C) object matrix, the reference's return value (:430,437).  Built on first use: boxing
        20 000 x 15 floats costs 10 ms of host time, more than the GPU spends on a small problem."""
        if self._res is None:
            r = self.result.shape[0]
            res = np.empty((r, 1 + 16 * len(self.comparisons)), dtype=object)  # hcat(res, result, gene_up_down) per comparison
            res[:, 0] = np.asarray(self.gene_names, dtype=object)
            for q, cm in enumerate(self.comparisons):
                res[:, 1 + 16 * q: 16 + 16 * q] = cm["result"]
                res[:, 16 + 16 * q] = cm["labels"]
            self._res = res
        return self._res


def deg_pairs(ctx, labels, pairs) -> dict:
    """{"ref_mask", "pairs"} of the comparison whose identify_degs has just returned on `ctx`: the reference set of its tallies and the
    pair list (class selection `pairs`) of its DEGs against that set.  No DEGs: an empty PairList, no library call for it."""
    mask = class_mask(pairs)
    ref = ctx.ref_mask()
    degs = np.flatnonzero(np.asarray(labels) != "no change").astype(np.int32)
    if degs.size == 0:
        pl = PairList(degs, np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.uint8))
    else:
        pl = ctx.pair_list(degs, mask)
    return {"ref_mask": ref, "pairs": pl}


def deg_sample_scores(ctx, labels) -> dict:
    """{"sample_scores"} of the comparison whose identify_degs has just returned on `ctx`: the SampleScores of its DEGs against the reference
    set of its tallies.  No DEGs: an empty object, no library call for it."""
    degs = np.flatnonzero(np.asarray(labels) != "no change").astype(np.int32)
    if degs.size == 0:
        z = np.zeros((0, ctx.S), dtype=np.int32)
        return {"sample_scores": SampleScores(degs, np.zeros(0, dtype=np.int32), z, z.copy(), z.copy())}
    return {"sample_scores": ctx.sample_scores(degs)}


def write_sample_calls_tsv(path, gene_names, sample_names, genes, calls) -> None:
    """gene<TAB>one column per sample; one row per gene of `genes` (the queries of a SampleTests) with at least one non-zero call in its
    row of `calls` (SampleTests.calls: -1, 0 or 1), in ascending gene order; "\n" line ends, like the result writers of reoa."""
    genes = np.asarray(genes, dtype=np.int64).reshape(-1)
    calls = np.asarray(calls).reshape(genes.size, len(sample_names))
    with open(path, "w") as f:
        f.write("\t".join(["gene"] + [str(n) for n in sample_names]) + "\n")
        for q in np.argsort(genes, kind="stable"):
            if calls[q].any():
                f.write("\t".join([str(gene_names[int(genes[q])])] + [str(int(v)) for v in calls[q]]) + "\n")


def need_pairs_for_support(pairs, pair_support) -> None:
    """pair_support=True asks for the support of the comparison's pair list: without `pairs` there is no list.  Raised before any context is
    opened."""
    if pair_support and pairs is None:
        raise _ffi.DimensionMismatch(_ffi.REO_EINVAL, "pair_support=True needs `pairs`: it is the support of the comparison's pair list "
                                                      "(pass pairs=\"reversed\" or another class selection)")


def deg_pair_support(ctx, pair_list) -> dict:
    """{"pair_support"} of the comparison whose pair list has just been taken on `ctx`: the PairSupport of that list (tied counts, no
    outcomes).  An empty list: an empty object, no library call for it."""
    return {"pair_support": ctx.pair_support(pair_list)}


def write_pair_support_tsv(path, gene_names, levels, support) -> None:
    """gene<TAB>partner<TAB>class, then <level>_gt and <level>_eq per group level, one line per listed pair in the list's own order; names
    from gene_names, the class as its tally's header name (n13, ...; empty for pairs that came without class codes); a header line, "\n"
    line ends, like the result writers of reoa.  Needs the tied counts."""
    if support.n_eq is None:
        raise _ffi.DimensionMismatch(_ffi.REO_EINVAL, "write_pair_support_tsv needs the tied counts: call pair_support with ties=True")
    names = _ffi.CLASS_NAMES
    with open(path, "w") as f:
        f.write("\t".join(["gene", "partner", "class"] + [f"{lv}_{w}" for lv in levels for w in ("gt", "eq")]) + "\n")
        for q, g in enumerate(support.genes):
            gname = gene_names[int(g)]
            for e in range(int(support.rowptr[q]), int(support.rowptr[q + 1])):
                cls = "" if support.code is None else names[int(support.code[e])]
                cells = [str(int(v)) for pair in zip(support.n_gt[e], support.n_eq[e]) for v in pair]
                f.write("\t".join([str(gname), str(gene_names[int(support.partner[e])]), cls] + cells) + "\n")


def write_sample_scores_tsv(path, gene_names, sample_names, scores) -> None:
    """gene<TAB>n_pairs<TAB>one column per sample, one row per scored gene, cells = scores.net; "\n" line ends, like the result writers."""
    net = scores.net
    with open(path, "w") as f:
        f.write("\t".join(["gene", "n_pairs"] + [str(n) for n in sample_names]) + "\n")
        for q, g in enumerate(scores.genes):
            f.write("\t".join([str(gene_names[int(g)]), str(int(scores.n_pairs[q]))] + [str(int(v)) for v in net[q]]) + "\n")


def write_pairs_tsv(path, gene_names, pair_list) -> None:
    """gene<TAB>partner<TAB>class, one line per listed pair in the list's own order, names from gene_names and the class as its tally's
    header name (n13, ...); a header line, "\n" line ends, like the result writers of reoa."""
    names = _ffi.CLASS_NAMES
    with open(path, "w") as f:
        f.write("gene\tpartner\tclass\n")
        for q, g in enumerate(pair_list.genes):
            partner, code = pair_list.row(q)
            gname = gene_names[int(g)]
            for j, c in zip(partner, code):
                f.write(f"{gname}\t{gene_names[int(j)]}\t{names[int(c)]}\n")


def perm_plan(permutations, *, contrasts=None, masked=False, shard=(0, 1)) -> None:
    """The refusals of `permutations`, raised before any context is opened: a count below 1, and the routes that have no permutation
    null -- `contrasts`, a validity mask (missing="pairwise" / `valid`) and shard[1] > 1."""
    if permutations is None:
        return

    def bad(why):
        return _ffi.DimensionMismatch(_ffi.REO_EINVAL, why)
    if int(permutations) < 1:
        raise bad(f"permutations = {permutations!r}: None (no permutation null) or a count of at least 1")
    if contrasts is not None:
        raise bad("permutations: the label-permutation null shuffles a comparison's two sides; it is not available together with `contrasts`")
    if masked:
        raise bad("permutations: the label-permutation null compares on the whole matrix and would count the fillers under the validity "
                  "mask; it is not available together with missing=\"pairwise\" or `valid`")
    if shard[1] > 1:
        raise bad(f"permutations: the permuted build has no sharded form (shard = {tuple(shard)!r})")


def deg_perm_null(ctx, gid, k, permutations, perm_seed, perm_strata, pval_deg, padj_deg) -> dict:
    """{"perm_null"} of the comparison whose identify_degs has just returned on `ctx`: the PermNull of `permutations` shuffles of its two
    sides (permuted_labels: seed perm_seed + k, within perm_strata if given), the reference set held at that of the run's last pass.
    Taken LAST among a comparison's read-outs: afterwards Context.ref_mask is refused until the next identify_degs."""
    rows = permuted_labels(gid, k, int(permutations), seed=int(perm_seed) + int(k), strata=perm_strata)
    return {"perm_null": ctx.permutation_null(rows, k=k, ref_mask=ctx.ref_mask(), pval_deg=pval_deg, padj_deg=padj_deg)}


def write_perm_null_tsv(path, gene_names, perm_null) -> None:
    """gene<TAB>delta1<TAB>n_ge<TAB>p_perm, one row per gene in gene order; a header line, "\n" line ends, like the result writers."""
    pp = perm_null.p_perm
    with open(path, "w") as f:
        f.write("gene\tdelta1\tn_ge\tp_perm\n")
        for i, g in enumerate(gene_names):
            f.write(f"{g}\t{float(perm_null.delta1_obs[i])!r}\t{int(perm_null.n_ge[i])}\t{float(pp[i])!r}\n")


def write_perm_summary_tsv(path, perm_null) -> None:
    """perm<TAB>n_up<TAB>n_down<TAB>se, one row per permutation in the order of its label rows; a header line and no trailer."""
    with open(path, "w") as f:
        f.write("perm\tn_up\tn_down\tse\n")
        for p in range(perm_null.n_perm):
            f.write(f"{p}\t{int(perm_null.n_up[p])}\t{int(perm_null.n_down[p])}\t{float(perm_null.se_null[p])!r}\n")


def top_pairs_plan(top_pairs, *, masked=False, shard=(0, 1)) -> None:
    """The refusals of `top_pairs`, raised before any context is opened: a count outside [1, 2^20], and the routes that have no search --
    a validity mask (missing="pairwise" / `valid`) and shard[1] > 1."""
    if top_pairs is None:
        return

    def bad(why):
        return _ffi.DimensionMismatch(_ffi.REO_EINVAL, why)
    if isinstance(top_pairs, bool) or not isinstance(top_pairs, (int, np.integer)) or not 1 <= int(top_pairs) <= 1 << 20:
        raise bad(f"top_pairs = {top_pairs!r}: None (no search) or a number of pairs between 1 and 2^20")
    if masked:
        raise bad("top_pairs: the search compares on the whole matrix and would count the fillers under the validity mask; it is not "
                  "available together with missing=\"pairwise\" or `valid`")
    if shard[1] > 1:
        raise bad(f"top_pairs: the search has no sharded form (shard = {tuple(shard)!r})")


def deg_top_pairs(ctx, k, treat, top_pairs) -> dict:
    """{"top_pairs"} of one comparison on `ctx`: the TopPairs of group k against the contrast's treatment group, or against every other
    sample for the reference's comparisons (treat None)."""
    return {"top_pairs": ctx.top_pairs(int(top_pairs), a=k, b=treat)}


def write_top_pairs_tsv(path, gene_names, top) -> None:
    """gene_i, gene_j, direction, score, rank_score, gt_A, eq_A, gt_B, eq_B: one line per pair in the list's own order, names from
    gene_names, floats by repr; a header line, "\n" line ends, like the result writers of reoa."""
    score, rank_score, direction = top.score, top.rank_score, top.direction
    with open(path, "w") as f:
        f.write("gene_i\tgene_j\tdirection\tscore\trank_score\tgt_A\teq_A\tgt_B\teq_B\n")
        for e in range(top.gene_i.size):
            f.write("\t".join([str(gene_names[int(top.gene_i[e])]), str(gene_names[int(top.gene_j[e])]), str(int(direction[e])),
                               repr(float(score[e])), repr(float(rank_score[e])), str(int(top.n_gt[e, 0])), str(int(top.n_eq[e, 0])),
                               str(int(top.n_gt[e, 1])), str(int(top.n_eq[e, 1]))]) + "\n")


def top_pairs_loo_plan(top_pairs_loo, *, masked=False, shard=(0, 1)) -> None:
    """The refusals of `top_pairs_loo`, raised before any context is opened: a kmax outside [1, 64], and the routes that have no search --
    a validity mask (missing="pairwise" / `valid`) and shard[1] > 1."""
    if top_pairs_loo is None:
        return

    def bad(why):
        return _ffi.DimensionMismatch(_ffi.REO_EINVAL, why)
    if isinstance(top_pairs_loo, bool) or not isinstance(top_pairs_loo, (int, np.integer)) or not 1 <= int(top_pairs_loo) <= 64:
        raise bad(f"top_pairs_loo = {top_pairs_loo!r}: None (no cross-validation) or kmax, a number of picks per fold between 1 and 64")
    if masked:
        raise bad("top_pairs_loo: the search compares on the whole matrix and would count the fillers under the validity mask; it is not "
                  "available together with missing=\"pairwise\" or `valid`")
    if shard[1] > 1:
        raise bad(f"top_pairs_loo: the search has no sharded form (shard = {tuple(shard)!r})")


def deg_top_pairs_loo(ctx, k, treat, top_pairs_loo) -> dict:
    """{"top_pairs_loo"} of one comparison on `ctx`: the TopPairsLoo (kmax = top_pairs_loo) of group k against the contrast's treatment
    group, or against every other sample for the reference's comparisons (treat None)."""
    return {"top_pairs_loo": ctx.top_pairs_loo(int(top_pairs_loo), a=k, b=treat)}


def write_top_pairs_cv_tsv(path, loo) -> None:
    """k, n_folds, n_wrong, n_undecided, error: one line per k = 1 .. kmax of a TopPairsLoo, the error (wrong + undecided) / folds by repr."""
    e, rate = loo.errors(), loo.error_rate()
    with open(path, "w") as f:
        f.write("k\tn_folds\tn_wrong\tn_undecided\terror\n")
        for k in range(rate.size):
            f.write(f"{k + 1}\t{int(e['n_folds'][k])}\t{int(e['n_wrong'][k])}\t{int(e['n_undecided'][k])}\t{float(rate[k])!r}\n")


def write_top_pairs_loo_tsv(path, sample_names, loo) -> None:
    """sample, side (A / B), votes_1 .. votes_kmax: one line per fold of a TopPairsLoo in the samples' own order; the samples of neither
    side are no folds and have no line."""
    votes = loo.votes()
    with open(path, "w") as f:
        f.write("\t".join(["sample", "side"] + [f"votes_{k + 1}" for k in range(votes.shape[1])]) + "\n")
        for s in range(votes.shape[0]):
            if int(loo.side[s]) == 2:
                continue
            f.write("\t".join([str(sample_names[s]), "A" if int(loo.side[s]) == 1 else "B"] + [str(int(v)) for v in votes[s]]) + "\n")


def top_partners_plan(top_partners, *, masked=False, shard=(0, 1)) -> None:
    """The refusals of `top_partners`, raised before any context is opened: a number of partners outside [1, 1024], and the routes that have
    no search -- a validity mask (missing="pairwise" / `valid`) and shard[1] > 1."""
    if top_partners is None:
        return

    def bad(why):
        return _ffi.DimensionMismatch(_ffi.REO_EINVAL, why)
    if isinstance(top_partners, bool) or not isinstance(top_partners, (int, np.integer)) or not 1 <= int(top_partners) <= 1024:
        raise bad(f"top_partners = {top_partners!r}: None (no partner lists) or m, a number of partners per DEG between 1 and 1024")
    if masked:
        raise bad("top_partners: the search compares on the whole matrix and would count the fillers under the validity mask; it is not "
                  "available together with missing=\"pairwise\" or `valid`")
    if shard[1] > 1:
        raise bad(f"top_partners: the search has no sharded form (shard = {tuple(shard)!r})")


def deg_top_partners(ctx, labels, k, treat, top_partners) -> dict:
    """{"top_partners"} of one comparison on `ctx`: the TopPartners (m = top_partners) of its DEGs against all genes, for group k against the
    contrast's treatment group, or against every other sample for the reference's comparisons (treat None).  No DEGs: an empty object, no
    library call for it."""
    degs = np.flatnonzero(np.asarray(labels) != "no change").astype(np.int32)
    m = int(top_partners)
    if degs.size == 0:
        a, b, sizes = ctx._sides(k, treat)
        return {"top_partners": _ffi.TopPartners(degs, np.zeros((0, m), np.int32), np.zeros((0, m, 2), np.int32), np.zeros((0, m, 2), np.int32),
                                                 np.zeros((0, m), np.int64), np.zeros((0, m), np.int64), np.zeros(0, np.int32), sizes, a,
                                                 None if b < 0 else b)}
    return {"top_partners": ctx.top_partners(degs, m, a=k, b=treat)}


def write_top_partners_tsv(path, gene_names, tp) -> None:
    """gene, rank, partner, num, score, rank_num, gt_A, eq_A, gt_B, eq_B: one line per found partner of a TopPartners, row by row in the
    rows' own order, rank counted from 1; names from gene_names, the score by repr; a header line, "\n" line ends."""
    score = tp.score
    with open(path, "w") as f:
        f.write("gene\trank\tpartner\tnum\tscore\trank_num\tgt_A\teq_A\tgt_B\teq_B\n")
        for r in range(tp.genes.size):
            for e in range(int(tp.n_found[r])):
                f.write("\t".join([str(gene_names[int(tp.genes[r])]), str(e + 1), str(gene_names[int(tp.partner[r, e])]), str(int(tp.num[r, e])),
                                   repr(float(score[r, e])), str(int(tp.rank_num[r, e])), str(int(tp.n_gt[r, e, 0])), str(int(tp.n_eq[r, e, 0])),
                                   str(int(tp.n_gt[r, e, 1])), str(int(tp.n_eq[r, e, 1]))]) + "\n")


def top_partners_null_plan(top_partners, top_partners_permutations) -> None:
    """The refusals of `top_partners_permutations`, raised before any context is opened (ValueError): given without `top_partners`, or no
    number of permutations between 1 and 2^20."""
    B = top_partners_permutations
    if B is None:
        return
    if top_partners is None:
        raise ValueError("top_partners_permutations needs top_partners: the null is that of the best partner score of the listed genes")
    if isinstance(B, bool) or not isinstance(B, (int, np.integer)) or not 1 <= int(B) <= 1 << 20:
        raise ValueError(f"top_partners_permutations = {B!r}: None (no null) or a number of permutations between 1 and 2^20")


def top_partners_null_cuts(tp) -> np.ndarray:
    """The cuts of a comparison's partner null: per row |N| of its last found partner (int64; 0 for a row that found none)."""
    last = np.maximum(np.asarray(tp.n_found, dtype=np.int64) - 1, 0)
    if tp.num.shape[1] == 0:
        return np.zeros(tp.genes.size, dtype=np.int64)
    return np.where(tp.n_found > 0, np.abs(tp.num[np.arange(tp.genes.size), last]), 0).astype(np.int64)


def deg_top_partners_null(ctx, gid, k, treat, tp, permutations, perm_seed, perm_strata) -> dict:
    """{"top_partners_null"} of one comparison on `ctx`: the TopPartnersNull of `permutations` label shuffles of the two sides for the genes
    of its "top_partners" (the DEGs) against all genes (permuted_sides: seed perm_seed + k, within perm_strata if given -- the rows that
    top_pairs_permutations uses), with the cuts of top_partners_null_cuts.  No DEGs: an empty object, no library call for it."""
    B = int(permutations)
    if tp.genes.size == 0:
        return {"top_partners_null": TopPartnersNull(tp.genes, np.zeros((B, 0), np.int64), np.zeros((B, 0), np.int32), np.zeros((B, 0), np.int32),
                                                     np.zeros(0, np.int64), tp.side_sizes, tp.a, tp.b)}
    rows = permuted_sides(gid, k, treat, B, seed=int(perm_seed) + int(k), strata=perm_strata)
    return {"top_partners_null": ctx.top_partners_null(rows, tp.genes, a=k, b=treat, cuts=top_partners_null_cuts(tp))}


def write_top_partners_null_tsv(path, gene_names, tp, null) -> None:
    """The columns of write_top_partners_tsv plus p_row (TopPartnersNull.p_row, by repr): one line per found partner, row by row."""
    score, p_row = tp.score, null.p_row(tp)
    with open(path, "w") as f:
        f.write("gene\trank\tpartner\tnum\tscore\trank_num\tgt_A\teq_A\tgt_B\teq_B\tp_row\n")
        for r in range(tp.genes.size):
            for e in range(int(tp.n_found[r])):
                f.write("\t".join([str(gene_names[int(tp.genes[r])]), str(e + 1), str(gene_names[int(tp.partner[r, e])]), str(int(tp.num[r, e])),
                                   repr(float(score[r, e])), str(int(tp.rank_num[r, e])), str(int(tp.n_gt[r, e, 0])), str(int(tp.n_eq[r, e, 0])),
                                   str(int(tp.n_gt[r, e, 1])), str(int(tp.n_eq[r, e, 1])), repr(float(p_row[r, e]))]) + "\n")


def top_pairs_null_plan(top_pairs, top_pairs_permutations) -> None:
    """The refusals of `top_pairs_permutations`, raised before any context is opened (ValueError): given without `top_pairs`, or no number
    of permutations between 1 and 2^20."""
    B = top_pairs_permutations
    if B is None:
        return
    if top_pairs is None:
        raise ValueError("top_pairs_permutations needs top_pairs: the null is that of the best score of the listed pairs")
    if isinstance(B, bool) or not isinstance(B, (int, np.integer)) or not 1 <= int(B) <= 1 << 20:
        raise ValueError(f"top_pairs_permutations = {B!r}: None (no null) or a number of permutations between 1 and 2^20")


def top_pairs_null_cuts(top) -> np.ndarray:
    """The cuts of a comparison's null: |N| of the list's entries 1, 10, 100 and its last, where they exist (int64, each entry once)."""
    at = sorted({e for e in (0, 9, 99, top.num.size - 1) if 0 <= e < top.num.size})
    return np.abs(top.num[at]).astype(np.int64)


def deg_top_pairs_null(ctx, gid, k, treat, top, permutations, perm_seed, perm_strata) -> dict:
    """{"top_pairs_null"} of one comparison on `ctx`: the TopPairsNull of `permutations` label shuffles of the two sides of its "top_pairs"
    (permuted_sides: seed perm_seed + k, within perm_strata if given; the samples of other groups take no part), with the cuts of
    top_pairs_null_cuts."""
    rows = permuted_sides(gid, k, treat, int(permutations), seed=int(perm_seed) + int(k), strata=perm_strata)
    return {"top_pairs_null": ctx.top_pairs_null(rows, a=k, b=treat, cuts=top_pairs_null_cuts(top))}


def write_top_pairs_null_tsv(path, gene_names, top, null) -> None:
    """The pair columns of write_top_pairs_tsv plus p_max (TopPairsNull.p_max, by repr): one line per pair in the list's own order."""
    score, rank_score, direction, p_max = top.score, top.rank_score, top.direction, null.p_max(top)
    with open(path, "w") as f:
        f.write("gene_i\tgene_j\tdirection\tscore\trank_score\tgt_A\teq_A\tgt_B\teq_B\tp_max\n")
        for e in range(top.gene_i.size):
            f.write("\t".join([str(gene_names[int(top.gene_i[e])]), str(gene_names[int(top.gene_j[e])]), str(int(direction[e])),
                               repr(float(score[e])), repr(float(rank_score[e])), str(int(top.n_gt[e, 0])), str(int(top.n_eq[e, 0])),
                               str(int(top.n_gt[e, 1])), str(int(top.n_eq[e, 1])), repr(float(p_max[e]))]) + "\n")


def missing_plan(data, missing, valid, *, shard=(0, 1), contrasts=None, sample_scores=False, sample_tests=False, sample_calls=False,
                 pair_support=False):
    """The pairwise route of run_identify_degs, decided before any context is opened.  Pure: no library, no GPU.  Returns (data, mask):
    mask None -- neither `missing` nor `valid` given -- and `data` as it came; otherwise the host matrix to upload and the bool G x S
    validity mask.  missing="pairwise": a floating host matrix, valid = ~isnan, the NaN cells filled with 0 in a COPY (the caller's array
    is untouched).  `valid`: an explicit mask for any host dtype; the matrix must then be free of NaN.  Raises DimensionMismatch, the
    message naming the reason, for: `missing` other than None / "pairwise"; a sparse or device-resident `data`; shard[1] > 1;
    `contrasts`, `sample_scores`, `sample_tests`, `sample_calls` or `pair_support` together with a mask; a mask of the wrong shape; an
    integer matrix with missing="pairwise" and no `valid` (it cannot hold a NaN); NaN in the matrix beside an explicit `valid`."""
    def bad(why):
        return _ffi.DimensionMismatch(_ffi.REO_EINVAL, why)
    if missing is not None and missing != "pairwise":
        raise bad(f"missing = {missing!r}: None (a NaN is refused) or \"pairwise\" (pairs are compared in the samples where both genes exist)")
    if missing is None and valid is None:
        return data, None
    if _ffi.is_sparse(data) or _ffi.is_device_sparse(data) or _ffi.is_device_tensor(data):
        raise bad("missing values: a sparse or device-resident 'data' has no pairwise route (the validity mask is made from a dense host matrix)")
    if shard[1] > 1:
        raise bad(f"missing values: the masked build has no sharded form (shard = {tuple(shard)!r})")
    for name, on in (("contrasts", contrasts is not None), ("sample_scores", sample_scores), ("sample_tests", sample_tests),
                     ("sample_calls", sample_calls), ("pair_support", pair_support)):
        if on:
            raise bad(f"missing values: `{name}` compares on the whole matrix and would count the fillers under the validity mask; "
                      "it is not available together with a mask")
    X = np.asarray(data)
    if X.ndim != 2:
        raise bad("'data' must be a genes x samples matrix")
    floating = np.issubdtype(X.dtype, np.floating)
    nan = np.isnan(X) if floating else np.zeros(X.shape, dtype=bool)
    if valid is not None:
        mask = np.asarray(valid)
        if mask.ndim != 2 or mask.shape != X.shape:
            raise bad(f"valid mask has shape {tuple(mask.shape)}, 'data' is {tuple(X.shape)} (genes x samples)")
        if nan.any():
            raise bad("an explicit `valid` mask needs a matrix without NaN: write a filler under the invalid cells (or pass missing=\"pairwise\" alone)")
        return X, mask != 0
    if not floating:
        raise bad(f"missing=\"pairwise\" derives the mask from NaN: 'data' of dtype {X.dtype} cannot hold one (pass `valid`)")
    if nan.any():
        X = X.copy()
        X[nan] = 0
    return X, ~nan


def run_identify_degs(data, group, gene_names, pval_reo, pval_deg, padj_deg, ref_gene, n_iter, n_conv, *,
                      seed: int = 0, device: int = -1, shard=(0, 1), allreduce=None, allgather=None, profile: bool = False,
                      pairs=None, sample_scores: bool = False, pair_support: bool = False, contrasts=None,
                      sample_tests: bool = False, sample_calls: bool = False, missing=None, valid=None, min_complete=None,
                      permutations=None, perm_seed: int = 0, perm_strata=None, top_pairs=None, top_pairs_permutations=None,
                      top_pairs_loo=None, top_partners=None, top_partners_permutations=None) -> DegRun:
    """identify_degs with the extras (trace, timings) kept.  `data` is a host matrix (numpy, anything np.asarray takes) or a torch
    tensor on a ROCm device, which is used in place (_ffi.device_matrix).  A column-major host matrix is read in place; a row-major one
    (numpy's default C order, column slices of a wider C-ordered array) is copied column-major on the host first, or, with REO_ROWMAJOR=1
    in the environment, read in place through reo_set_matrix_rm_* -- no transposing host copy, the library transposes on the device
    (_ffi.host_matrix_entry; opt-in until its timing has been recorded).
    A scipy.sparse matrix (CSR / COO / CSC: AnnData's X) goes up as CSC -- no toarray(), the zeros never exist on the host or on the
    link -- and becomes dense on the device (_ffi.csc_entry, reo_set_matrix_csc_*); the caller's matrix is not modified.
    A sparse torch tensor on a ROCm device (sparse_csc, the .t() of a cells x genes sparse_csr, or COO / CSR through to_sparse_csc()) never
    leaves the device: its index arrays are checked by a kernel and the matrix becomes dense where it is (_ffi.device_csc_entry,
    reo_set_matrix_csc_dev_*).  The mirror does not canonicalise: unsorted or repeated row indices inside a column are refused.
    Two groups: one comparison, group 1 vs
    group 2 (the reference's `gnum == 2` path, :387-389,431-434).  More groups: one comparison per
    group, that group vs every other sample (:375-390,396-436), 16 more columns each.
    `pairs` (not in the reference): a class selection (_ffi.class_mask: "reversed", names "n11" .. "n33", codes, a mask).  Every comparison
    dict then gains "ref_mask", the reference set its returned tallies were counted over (Context.ref_mask), and "pairs", the PairList of its
    DEGs (label != "no change", ascending gene index) against that set -- taken right after its identify_degs, while its class table is
    still the current one.  None (the default): no further call is made and the dicts have the keys they always had.
    `sample_scores` (not in the reference): True adds "sample_scores" to every comparison dict, the SampleScores of its DEGs against the
    reference set of its tallies (Context.sample_scores; rows = DEGs ascending, columns = the samples as given), taken at the same moment.
    False (the default): no further call, no new key.
    `sample_tests` (not in the reference): True adds "sample_tests" to every comparison dict, the SampleTests of ALL genes against the
    reference set of its tallies (Context.sample_tests: per gene and sample, Fisher's exact test of the sample's orderings against the pairs
    that are stable in the comparison's control side), taken at the same moment as "sample_scores".  False (the default): no further call,
    no new key.
    `sample_calls` (not in the reference): True adds "sample_calls" to every comparison dict, the SampleCalls of ALL genes with the run's own
    pval_deg and padj_deg against the reference set of its tallies (Context.sample_calls: what "sample_tests" .calls(pval_deg, padj_deg)
    gives, formed on the device, one byte per cell coming back), taken at the same moment.  False (the default): no further call, no new key.
    `pair_support` (not in the reference): True needs `pairs` (DimensionMismatch otherwise) and adds "pair_support" to every comparison
    dict, the PairSupport of that comparison's pair list (Context.pair_support: per listed pair and group, in how many samples the DEG lies
    above its partner, and in how many the two are tied), taken at the same moment as "pairs".  False (the default): no further call, no new
    key.
    `contrasts` (not in the reference): "all" or a sequence of (ctrl_level, treat_level) pairs (parse_contrasts).  One comparison per
    contrast, in the order given, instead of the reference's: group ctrl against group treat ALONE (Context.build_contrast; with more than two
    groups every contrast is classified from the per-group counts of the first build, nothing is counted again).  Each comparison dict
    carries "ctrl" and "treat" (level names) besides today's keys, "k" is the control's index, and `res` has 1 + 16 len(contrasts) columns;
    `pairs`, `sample_scores` and `pair_support` work per contrast.  None (the default): the reference's comparisons.
    `missing`, `valid`, `min_complete` (not in the reference, which drops every gene with a missing cell): missing="pairwise" takes a
    floating host matrix with NaN -- valid = ~isnan, the NaN cells are filled with 0 in a copy, the caller's array is untouched --;
    `valid` is an explicit boolean G x S mask for any host dtype and implies the pairwise route (the matrix must then be free of NaN).
    Every comparison is then built by Context.build_pairs_masked: a pair is compared in the samples where both genes are valid, each side
    against the threshold of that many samples, and a side with fewer than `min_complete` of them (None: per side min(side size, 8 at
    pval_reo = 0.01); an int: both sides) is unstable.  The comparison dict gains "min_complete", and info["masked_build"] reads 1.
    `pairs` works; `contrasts`, `sample_scores`, `sample_tests`, `sample_calls`, `pair_support`, a sparse or device-resident matrix and
    shard[1] > 1 are refused together with a mask (missing_plan).  Defaults: nothing changes, and a NaN is refused as always.
    `permutations`, `perm_seed`, `perm_strata` (not in the reference): permutations=B adds "perm_null" to every comparison dict, the
    PermNull of B label shuffles of the comparison's two sides (Context.permutation_null; rows from permuted_labels with seed perm_seed + k,
    shuffled within perm_strata -- one label per sample -- when given), the reference set held at that of the run's last pass; taken after
    every other read-out of the comparison.  Refused with `contrasts`, with a mask and with shard[1] > 1 (perm_plan).  None (the default):
    no further call, no new key.
    `top_pairs` (not in the reference): an int K adds "top_pairs" to every comparison dict, the TopPairs of the K best of ALL gene pairs
    (Context.top_pairs: the top-scoring-pair search) for the comparison's group k against the contrast's treatment group, or against every
    other sample for the reference's comparisons; taken after the other read-outs and before the permutation null.  Refused with a mask and
    with shard[1] > 1 (top_pairs_plan).  None (the default): no further call, no new key.
    `top_pairs_permutations` (not in the reference): an int B, together with `top_pairs`, adds "top_pairs_null" to every comparison dict,
    the TopPairsNull of B label shuffles of the search's two sides (Context.top_pairs_null; rows from permuted_sides with seed
    perm_seed + k, shuffled within perm_strata when given; cuts: |N| of the list's entries 1, 10, 100 and K) -- .p_max(top_pairs) is the
    single-step maxT adjusted p-value of every listed pair.  Works for the reference's comparisons and for contrasts.  Without `top_pairs`:
    ValueError.  None (the default): no further call, no new key.
    `top_pairs_loo` (not in the reference): an int kmax adds "top_pairs_loo" to every comparison dict, the TopPairsLoo of the
    leave-one-out cross-validation of the k-TSP selection (Context.top_pairs_loo) with the sides of `top_pairs` -- the comparison's group
    against the contrast's treatment group or every other sample; independent of `top_pairs`.  Refused with a mask and with shard[1] > 1
    (top_pairs_loo_plan).  None (the default): no further call, no new key.
    `top_partners` (not in the reference): an int m adds "top_partners" to every comparison dict, the TopPartners of the comparison's DEGs
    against all genes (Context.top_partners: per DEG its m best partner genes, with the counts and the score of the two-gene rule), with the
    sides of `top_pairs`.  A comparison without DEGs gets an empty TopPartners.  Refused with a mask and with shard[1] > 1
    (top_partners_plan).  None (the default): no further call, no new key.
    `top_partners_permutations` (not in the reference): an int B, together with `top_partners`, adds "top_partners_null" to every comparison
    dict, the TopPartnersNull of B label shuffles of the two sides for the comparison's DEGs against all genes (Context.top_partners_null;
    the rows of `top_pairs_permutations`: permuted_sides with seed perm_seed + k, within perm_strata when given; cuts: |N| of each row's
    last found partner) -- .p_row(top_partners) is the single-step maxT p-value of every listed partner over the gene's partners.  Gamma
    is no tie-break under the null; a DEG was selected with the same labels, so its p_row is a permutation p-value of the partner
    search, not of the DEG call.  Without `top_partners`: ValueError.  None (the default): no further call, no new key."""
    need_pairs_for_support(pairs, pair_support)
    data, mask = missing_plan(data, missing, valid, shard=shard, contrasts=contrasts, sample_scores=sample_scores, sample_tests=sample_tests,
                              sample_calls=sample_calls, pair_support=pair_support)
    perm_plan(permutations, contrasts=contrasts, masked=mask is not None, shard=shard)
    top_pairs_plan(top_pairs, masked=mask is not None, shard=shard)
    top_pairs_null_plan(top_pairs, top_pairs_permutations)
    top_pairs_loo_plan(top_pairs_loo, masked=mask is not None, shard=shard)
    top_partners_plan(top_partners, masked=mask is not None, shard=shard)
    top_partners_null_plan(top_partners, top_partners_permutations)
    if mask is not None:
        _ffi.resolve_min_complete(min_complete, (1, 1), pval_reo)   # (its refusals, before a context is opened)
    # a torch tensor on a ROCm device: a strided one is used where it is, a sparse one is made dense there (its device is the context's)
    on_device = _ffi.is_device_sparse(data) or _ffi.is_device_tensor(data)
    if on_device:
        device = data.device.index if data.device.index is not None else -1
    elif not _ffi.is_sparse(data):   # (np.asarray of a sparse matrix is a 0-d object array)
        data = np.asarray(data)
    if len(data.shape) != 2:
        raise _ffi.DimensionMismatch(_ffi.REO_EINVAL, "'data' must be a genes x samples matrix")
    r, c = data.shape
    if c != len(group):  # :355
        raise _ffi.DimensionMismatch(_ffi.REO_EINVAL, "'data' and 'group' do not have compatiable sizes")
    gid, levels = encode_groups(group)
    if len(levels) < 2:  # :356
        raise _ffi.DimensionMismatch(_ffi.REO_EINVAL, "Only 1 level in 'group1, at least 2 levels!")
    if len(gene_names) != r or len(ref_gene) != r:
        raise _ffi.DimensionMismatch(_ffi.REO_EINVAL, "gene_names / ref_gene length != number of rows of 'data'")
    plan = comparison_plan(levels, contrasts)
    comps = []
    with _ffi.Context(device=device, seed=seed) as ctx:
        ctx.set_profiling(profile)
        # groups, thresholds and sharding BEFORE the matrix: reo_set_matrix then ranks the samples as their columns arrive and, on
        # one GPU with two groups, starts the pair kernel's first side while the second group is still crossing PCIe
        ctx.set_groups(gid, len(levels))
        if mask is None:   # (the masked build has thresholds of its own: nothing is started on the fillers while the matrix arrives)
            thr = ctx.compute_thresholds(pval_reo)
        if shard[1] > 1:
            ctx.set_shard(*shard)
            if allgather is not None:
                ctx.set_allgather(allgather)   # all-gather of the shards' own table words (what the in-library RCCL path does)
            else:
                ctx.set_allreduce(allreduce)   # in-place sum of the whole table
        if on_device:
            ctx.set_matrix_tensor(data)   # (the context keeps the tensor alive until it is closed, behind the last build_pairs)
        else:
            ctx.set_matrix(data)
        if mask is not None:
            thr = ctx.compute_thresholds(pval_reo)   # (reported only: what the complete sides would be held to)
            ctx.set_valid_mask(mask)
        for k, treat in plan:  # `for k=1:gnum ... if gnum==2 break` (:396,431-434), or the contrasts
            if mask is not None:
                cm = {"k": k, "min_complete": ctx.build_pairs_masked(k, pval_reo, min_complete)}
            else:
                cm = build_comparison(ctx, levels, k, treat)
            result, iters, trace = ctx.identify_degs(np.asarray(ref_gene, dtype=bool), pval_deg, padj_deg, n_iter, n_conv)
            cm.update({"result": result, "labels": label_genes(result, pval_deg, padj_deg), "iters_run": iters, "trace": trace})
            comps.append(cm)
            if pairs is not None:
                comps[-1].update(deg_pairs(ctx, comps[-1]["labels"], pairs))
                if pair_support:
                    comps[-1].update(deg_pair_support(ctx, comps[-1]["pairs"]))
            if sample_scores:
                comps[-1].update(deg_sample_scores(ctx, comps[-1]["labels"]))
            if sample_tests:
                comps[-1]["sample_tests"] = ctx.sample_tests()   # all genes, against the reference set of this comparison's tallies
            if sample_calls:
                comps[-1]["sample_calls"] = ctx.sample_calls(pval_deg, padj_deg)   # all genes, the run's thresholds, the same reference set
            if top_pairs is not None:
                comps[-1].update(deg_top_pairs(ctx, k, treat, top_pairs))
                if top_pairs_permutations is not None:
                    comps[-1].update(deg_top_pairs_null(ctx, gid, k, treat, comps[-1]["top_pairs"], top_pairs_permutations, perm_seed, perm_strata))
            if top_pairs_loo is not None:
                comps[-1].update(deg_top_pairs_loo(ctx, k, treat, top_pairs_loo))
            if top_partners is not None:
                comps[-1].update(deg_top_partners(ctx, comps[-1]["labels"], k, treat, top_partners))
                if top_partners_permutations is not None:
                    comps[-1].update(deg_top_partners_null(ctx, gid, k, treat, comps[-1]["top_partners"], top_partners_permutations, perm_seed,
                                                           perm_strata))
            if permutations is not None:   # last: it uses the iteration's buffers (ref_mask is refused behind it)
                comps[-1].update(deg_perm_null(ctx, gid, k, permutations, perm_seed, perm_strata, pval_deg, padj_deg))
        timings = ctx.timings() if profile else {}
        info = ctx.info()
    first = comps[0]
    return DegRun(result=first["result"], labels=first["labels"], levels=levels, thresholds=thr, iters_run=first["iters_run"],
                  trace=first["trace"], timings=timings, info=info, comparisons=comps, gene_names=list(gene_names))


def cells_partition(cell_group, n_pseudo: int, seed: int = 0):
    """The pseudo-bulk plan of a cell matrix whose column t belongs to group cell_group[t] (src/RankCompV3.jl:608-612), pure numpy: the
    groups in order of first appearance, the cells of a group in column order, each group cut by reoa.pseudobulk_partition(c, n_pseudo,
    seed, gi) -- the reference's shuffled chunks of ceil(c / n_pseudo) cells (:60-62) -- and the pieces concatenated.  Returns (order,
    chunk_ptr, profile names `<g>_x<k>`, profile groups): what Context.pseudobulk / set_matrix_pseudobulk take, and what reoa.prepare
    builds from its tables."""
    from .reoa import pseudobulk_partition
    gid, levels = encode_groups(cell_group)
    orders, ptr, names, groups = [], [0], [], []
    for gi, g in enumerate(levels):
        cols = np.flatnonzero(gid == gi)
        o, p = pseudobulk_partition(cols.size, n_pseudo, seed, gi)
        orders.append(cols[o])
        ptr += (p[1:].astype(np.int64) + ptr[-1]).tolist()
        names += [f"{g}_x{k + 1}" for k in range(len(p) - 1)]
        groups += [g] * (len(p) - 1)
    order = np.concatenate(orders).astype(np.int32) if orders else np.zeros(0, dtype=np.int32)
    return order, np.asarray(ptr, dtype=np.int32), names, groups


class CellsDegRun(NamedTuple):
    """identify_degs_cells: the DegRun of the pseudo-bulk profiles and what the filters kept."""
    run: DegRun
    gene_kept: np.ndarray        # bool over the input genes; run.gene_names are the kept ones
    profile_kept: np.ndarray     # bool over the pseudo-bulk profiles cells_partition made
    profile_names: list          # `<g>_x<k>` of the kept profiles (the columns of the matrix that was analysed)
    profile_groups: list         # their groups


def identify_degs_cells(cells, cell_group, gene_names, n_pseudo, pval_reo, pval_deg, padj_deg, ref_gene, n_iter, n_conv, *,
                        min_profiles: int = 0, min_features: int = 0, ref_gene_max: int = 3000, seed: int = 0, device: int = 0,
                        profile: bool = False, pairs=None, sample_scores: bool = False, pair_support: bool = False,
                        contrasts=None, sample_tests: bool = False, sample_calls: bool = False,
                        permutations=None, perm_seed: int = 0, perm_strata=None, top_pairs=None,
                        top_pairs_permutations=None, top_pairs_loo=None, top_partners=None,
                        top_partners_permutations=None) -> CellsDegRun:
    """Cells to DEGs without a host trip for the profiles: `cells` is a genes x cells matrix (scipy.sparse, anything np.asarray takes, or
    a torch tensor on a ROCm device -- sparse or strided -- which is read where it is: reo_set_matrix_pseudobulk_*_dev_*),
    cell_group one label per cell.  cells_partition -> the pseudo-bulk sums written into the context's matrix (set_matrix_pseudobulk) ->
    the reference's two low-expression filters on the device (filter_matrix, :618 / :626) -> groups of the kept profiles, thresholds,
    pair table and iteration as in run_identify_degs.  ref_gene is a bool mask over the INPUT genes (subset by gene_kept here), or None for
    synth.ref_mask(G', min(G', ref_gene_max), seed), the draw reoa makes.  Bit-identical to Context.pseudobulk -> numpy filters ->
    run_identify_degs on the same seed.  (reoa() keeps its host route: its writers want the profile matrix on the host.)
    `pairs`, `sample_scores`, `pair_support`, `sample_tests`, `sample_calls`: as in run_identify_degs; gene indices are those of the KEPT genes (run.gene_names), columns
    the kept profiles.  `contrasts`: as in run_identify_degs, over the group levels of the cells (checked against the levels of cell_group
    before any context is opened, and again against those of the kept profiles).  `permutations`, `perm_seed`, `perm_strata`: as in
    run_identify_degs; perm_strata has one label per pseudo-bulk PROFILE of cells_partition (the kept ones are used).  `top_pairs`,
    `top_pairs_permutations`, `top_pairs_loo`, `top_partners`, `top_partners_permutations`: as in run_identify_degs."""
    need_pairs_for_support(pairs, pair_support)
    perm_plan(permutations, contrasts=contrasts)
    top_pairs_plan(top_pairs)
    top_pairs_null_plan(top_pairs, top_pairs_permutations)
    top_pairs_loo_plan(top_pairs_loo)
    top_partners_plan(top_partners)
    top_partners_null_plan(top_partners, top_partners_permutations)
    on_device = _ffi.is_device_sparse(cells) or _ffi.is_device_tensor(cells)
    if on_device:   # a torch tensor on a ROCm device, sparse or strided: summed where it is, on its own device
        device = cells.device.index if cells.device.index is not None else -1
    elif not _ffi.is_sparse(cells):
        cells = np.asarray(cells)
    if len(cells.shape) != 2:
        raise _ffi.DimensionMismatch(_ffi.REO_EINVAL, "'cells' must be a genes x cells matrix")
    r, ncell = cells.shape
    if ncell != len(cell_group):
        raise _ffi.DimensionMismatch(_ffi.REO_EINVAL, "'cells' and 'cell_group' do not have compatible sizes")
    if len(gene_names) != r or (ref_gene is not None and len(ref_gene) != r):
        raise _ffi.DimensionMismatch(_ffi.REO_EINVAL, "gene_names / ref_gene length != number of rows of 'cells'")
    if n_pseudo < 1:
        raise _ffi.DimensionMismatch(_ffi.REO_EINVAL, "n_pseudo must be at least 1")
    order, chunk_ptr, names, groups = cells_partition(cell_group, n_pseudo, seed)
    if contrasts is not None:
        parse_contrasts(encode_groups(groups)[1], contrasts)
    comps = []
    with _ffi.Context(device=device, seed=seed) as ctx:
        ctx.set_profiling(profile)
        ctx.set_matrix_pseudobulk(cells, order, chunk_ptr)
        profile_kept, gene_kept = ctx.filter_matrix(min_profiles, min_features)
        names = [n for n, k in zip(names, profile_kept) if k]
        groups = [g for g, k in zip(groups, profile_kept) if k]
        kept_genes = [n for n, k in zip(gene_names, gene_kept) if k]
        gid, levels = encode_groups(groups)
        if len(levels) < 2:  # :356
            raise _ffi.DimensionMismatch(_ffi.REO_EINVAL, "Only 1 level in 'group1, at least 2 levels!")
        G = len(kept_genes)
        ref = synth.ref_mask(G, min(G, ref_gene_max), seed) if ref_gene is None else np.asarray(ref_gene, dtype=bool)[gene_kept]
        ctx.set_groups(gid, len(levels))
        thr = ctx.compute_thresholds(pval_reo)
        for k, treat in comparison_plan(levels, contrasts):
            cm = build_comparison(ctx, levels, k, treat)
            result, iters, trace = ctx.identify_degs(ref, pval_deg, padj_deg, n_iter, n_conv)
            cm.update({"result": result, "labels": label_genes(result, pval_deg, padj_deg), "iters_run": iters, "trace": trace})
            comps.append(cm)
            if pairs is not None:
                comps[-1].update(deg_pairs(ctx, comps[-1]["labels"], pairs))
                if pair_support:
                    comps[-1].update(deg_pair_support(ctx, comps[-1]["pairs"]))
            if sample_scores:
                comps[-1].update(deg_sample_scores(ctx, comps[-1]["labels"]))
            if sample_tests:
                comps[-1]["sample_tests"] = ctx.sample_tests()   # all genes, against the reference set of this comparison's tallies
            if sample_calls:
                comps[-1]["sample_calls"] = ctx.sample_calls(pval_deg, padj_deg)   # all genes, the run's thresholds, the same reference set
            if top_pairs is not None:
                comps[-1].update(deg_top_pairs(ctx, k, treat, top_pairs))
                if top_pairs_permutations is not None:
                    strata = None if perm_strata is None else np.asarray(perm_strata)[np.asarray(profile_kept, dtype=bool)]
                    comps[-1].update(deg_top_pairs_null(ctx, gid, k, treat, comps[-1]["top_pairs"], top_pairs_permutations, perm_seed, strata))
            if top_pairs_loo is not None:
                comps[-1].update(deg_top_pairs_loo(ctx, k, treat, top_pairs_loo))
            if top_partners is not None:
                comps[-1].update(deg_top_partners(ctx, comps[-1]["labels"], k, treat, top_partners))
                if top_partners_permutations is not None:
                    strata = None if perm_strata is None else np.asarray(perm_strata)[np.asarray(profile_kept, dtype=bool)]
                    comps[-1].update(deg_top_partners_null(ctx, gid, k, treat, comps[-1]["top_partners"], top_partners_permutations, perm_seed,
                                                           strata))
            if permutations is not None:   # last: it uses the iteration's buffers (ref_mask is refused behind it)
                strata = None if perm_strata is None else np.asarray(perm_strata)[np.asarray(profile_kept, dtype=bool)]
                comps[-1].update(deg_perm_null(ctx, gid, k, permutations, perm_seed, strata, pval_deg, padj_deg))
        timings = ctx.timings() if profile else {}
        info = ctx.info()
    first = comps[0]
    run = DegRun(result=first["result"], labels=first["labels"], levels=levels, thresholds=thr, iters_run=first["iters_run"],
                 trace=first["trace"], timings=timings, info=info, comparisons=comps, gene_names=kept_genes)
    return CellsDegRun(run, gene_kept, profile_kept, names, groups)


def identify_degs(data, group, gene_names, pval_reo, pval_deg, padj_deg, ref_gene, n_iter, n_conv, **kw) -> np.ndarray:
    """Drop-in for identify_degs (src/RankCompV3.jl:339-350): same arguments in the same order, same
    G x (1 + 16 C) return (C = 1 for two groups, else the number of groups).  `seed=` keys the tie
    coins that the reference draws from its unseeded global RNG (:73)."""
    return run_identify_degs(data, group, gene_names, pval_reo, pval_deg, padj_deg, ref_gene, n_iter, n_conv, **kw).res
