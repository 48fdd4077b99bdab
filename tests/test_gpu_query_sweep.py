"""The differential sweep of the query family on long-lived contexts: the 24 cases of tests/query_sweep_cases.py, each with every query
entry point -- reo_pair_list, reo_sample_counts, reo_pair_support, reo_sample_tests, reo_sample_calls, reo_rank_shift, reo_top_pairs,
reo_top_partners, reo_top_pairs_null, reo_top_pairs_loo, reo_perm_codes, reo_perm_null -- and reo_identify_degs made in the case's own
order, two of the calls once more later in the sequence.  Every expectation comes from the numpy restatements under tests/ and from the
oracle package (query_sweep_cases.Expect); the class rows that an expectation needs are the oracle's, never the context's.  Every
comparison is exact but three: the tails of the sample tests (sample_tests_cases.tolerance), the statistics of identify_degs (the bounds
of tests/test_gpu_parity.py) and delta1 of the permutation null (the same bound).

Contexts are long-lived: the cases run in 8 groups of 3 consecutive cases, each group on one context, so a context meets a new matrix
shape, element type and group layout twice with its buffers kept; the first case of a group (and a case replayed alone) opens a fresh one.
tests/test_query_sweep_cpu.py shows on the CPU what the cases cover and that each comparison used here fails on a planted error."""
import numpy as np
import pytest

import query_sweep_cases as qs
import sample_calls_cases as cc
import sample_tests_cases as stc
import top_pairs_cases as tpc
import top_pairs_loo_cases as tlc
import top_partners_cases as tprc
from test_gpu_contrasts import P_ATOL, STAT_RTOL
from test_gpu_pair_list import same as same_list
from test_gpu_pair_support import check as support_check
from test_gpu_sample_counts import same as same_counts
from test_gpu_sample_tests import same_integers

pytestmark = pytest.mark.gpu

TIMERS = ("perm_kernel_us", "top_pairs_hist_us", "top_pairs_emit_us", "top_pairs_null_us", "top_pairs_loo_words_us", "top_pairs_loo_select_us",
          "top_partners_count_us", "top_partners_select_us")
# what a call may change in info() besides the timers: the gene-order planes made behind a slot-order build, its own batch width, and
# what the iteration reports about its passes
PLANES = ("planes_on_demand",)
OWN = {"codes": (), "pair_list": (), "sample_counts": PLANES, "pair_support": PLANES, "sample_tests": PLANES, "sample_calls": PLANES,
       "rank_shift": PLANES, "top_pairs": PLANES, "top_partners": PLANES, "top_pairs_null": PLANES + ("top_pairs_null_batch",),
       "top_pairs_loo": PLANES, "perm_codes": PLANES + ("perm_batch",), "perm_null": PLANES + ("perm_batch",),
       "identify_degs": ("cycle_period", "cycle_found_at_pass", "cycle_passes_skipped", "eager_range_launches")}

_open = {}                                                                       # group of three -> (context, the last case it ran)


def context_for(pkg, no):
    """the context of case `no`: that of its group when the group's previous case has just run on it, else a fresh one"""
    grp = no // 3
    ctx, last = _open.get(grp, (None, None))
    if ctx is None or no % 3 == 0 or last != no - 1:
        for g in list(_open):                                                    # (one context at a time)
            _open.pop(g)[0].close()
        ctx = pkg.Context(device=0, seed=qs.SWEEP_SEED + grp)
    _open[grp] = (ctx, no)
    return ctx


@pytest.fixture(scope="module", autouse=True)
def close_contexts():
    yield
    for g in list(_open):
        _open.pop(g)[0].close()


def fields(x, names):
    return tuple(np.ascontiguousarray(getattr(x, f)) for f in names if getattr(x, f) is not None)


class Run:
    """one case on its context: the calls, each compared as it is made.  `ref` is the reference set that a NULL partner mask stands for
    (None: there is none, reo_get_ref_mask refuses)."""

    def __init__(self, pkg, ctx, no):
        self.pkg, self.ctx, self.cs, self.exp = pkg, ctx, qs.case(no), qs.expect(no)
        self.tag = self.cs["tag"]
        self.ref = None
        self.null_runs = 0

    def masks(self, name):
        """the explicit mask of a table query and, while a reference set stands, the NULL mask with the set it stands for"""
        out = [(self.cs[name + "_mask"], self.cs[name + "_mask"])]
        if self.ref is not None:
            out.append((None, self.ref))
            self.null_runs += 1
        return out

    # every method returns the arrays of its explicit-mask answer: a repeated call must return the same bytes

    def codes(self):
        G = self.cs["G"]
        got = self.ctx.get_codes(0, G, 0, G)
        assert np.array_equal(got, self.exp.codes), (self.tag, "get_codes", int((got != self.exp.codes).sum()), np.argwhere(got != self.exp.codes)[:4].tolist())
        return (got,)

    def pair_list(self):
        out = []
        for pm, mask in self.masks("pair_list"):
            pl = self.ctx.pair_list(self.cs["queries"], self.cs["pair_list_classes"], pm)
            same_list(pl, self.exp.pair_list(mask), (self.tag, "pair_list", pm is None))
            out.append(fields(pl, ("genes", "rowptr", "partner", "code")))
        return out[0]

    def sample_counts(self):
        out = []
        for pm, mask in self.masks("sample_counts"):
            got = self.ctx.sample_counts(self.cs["queries"], self.cs["sample_counts_classes"], pm)
            assert np.array_equal(got.genes, self.cs["queries"])
            same_counts(got, self.exp.sample_counts(mask), (self.tag, "sample_counts", pm is None))
            out.append(fields(got, ("n_sel", "n_gt", "n_eq")))
        no_ties = self.ctx.sample_counts(self.cs["queries"], self.cs["sample_counts_classes"], self.cs["sample_counts_mask"], ties=False)
        assert no_ties.n_eq is None and np.array_equal(no_ties.n_gt, out[0][1]), (self.tag, "sample_counts ties=False")
        return out[0]

    def pair_support(self):
        cs = self.cs
        rowptr, partner, _ = self.exp.pair_list(cs["pair_list_mask"])              # the rows that pair_list must list, from the oracle's codes
        csr = (cs["queries"], rowptr, partner)
        exp = self.exp.pair_support(csr)
        ps, _ = support_check(self.ctx, cs["Xo"], cs["gid"], csr, self.pkg, ties=True, outcomes=True, tag=(self.tag, "pair_support outcomes"), exp=exp)
        support_check(self.ctx, cs["Xo"], cs["gid"], csr, self.pkg, ties=False, outcomes=False, tag=(self.tag, "pair_support"), exp=exp)
        return fields(ps, ("n_gt", "n_eq", "outcome"))

    def sample_tests(self):
        out = []
        for pm, mask in self.masks("sample_tests"):
            tag = (self.tag, "sample_tests", pm is None)
            exp = self.exp.sample_tests(mask)
            got = self.ctx.sample_tests(self.cs["queries"], pm)
            assert np.array_equal(got.genes, self.cs["queries"]) and got.p_up.dtype == np.float64 and got.p_up.shape == got.p_down.shape == exp["u"].shape, tag
            same_integers(got, exp, tag)
            background = int((exp["n_above_ctrl"].astype(np.int64) + exp["n_below_ctrl"]).max(initial=0))
            stc.check_tails(got.p_up, got.p_down, exp["n_above_ctrl"][:, None], exp["n_below_ctrl"][:, None], exp["u"], exp["d"],
                            stc.tolerance(background), tag)
            out.append(fields(got, ("n_above_ctrl", "n_below_ctrl", "rev_up", "rev_down", "tied", "p_up", "p_down")))
        return out[0]

    def sample_calls(self):
        out = []
        for pm, _ in self.masks("sample_calls"):
            st = self.ctx.sample_tests(self.cs["queries"], pm, counts=False)
            got = self.ctx.sample_calls(qs.CALLS_PVAL, qs.CALLS_PADJ, self.cs["queries"], pm)
            cc.same(got, st, qs.CALLS_PVAL, qs.CALLS_PADJ, (self.tag, "sample_calls", pm is None))
            out.append(fields(got, cc.FIELDS))
        return out[0]

    def rank_shift(self):
        D = self.ctx.rank_shift(self.cs["a"], self.cs["b"])
        assert D.dtype == np.int64 and np.array_equal(D, self.exp.top.D), (self.tag, "rank_shift", np.flatnonzero(D != self.exp.top.D)[:4].tolist())
        return (D,)

    def top_pairs(self):
        cs = self.cs
        tp = self.ctx.top_pairs(cs["n"], cs["a"], cs["b"], cs["top_pairs_mask"])
        qs.check_top_pairs(tp, self.exp.top_masked, cs["n"], (self.tag, "top_pairs"))
        assert (tp.a, tp.b) == (cs["a"], cs["b"])
        return fields(tp, ("gene_i", "gene_j", "n_gt", "n_eq", "num", "rank_num"))

    def top_partners(self):
        cs = self.cs
        tp = self.ctx.top_partners(cs["queries"], cs["m"], cs["a"], cs["b"], cs["top_partners_mask"])
        tprc.check_table(tp, self.exp.partners(), cs["m"])
        assert np.array_equal(tp.genes, cs["queries"]) and (tp.a, tp.b) == (cs["a"], cs["b"]) and tuple(int(v) for v in tp.side_sizes) == self.exp.top.sizes, self.tag
        # and the same rows as the subsequence of the context's own search over every pair
        every = self.ctx.top_pairs(max(cs["n_all"], 1), cs["a"], cs["b"])
        assert every.gene_i.size == cs["n_all"], (self.tag, "top_pairs over all pairs")
        listed = tpc.Oracle(every.gene_i, every.gene_j, np.stack([every.n_gt[:, 0], every.n_eq[:, 0], every.n_gt[:, 1], every.n_eq[:, 1]], axis=1),
                            every.num, every.rank_num, None, tuple(int(v) for v in every.side_sizes), None)
        tprc.check_table(tp, [tprc.from_pairs(listed, int(q), cs["top_partners_mask"]) for q in cs["queries"]], cs["m"])
        return fields(tp, ("partner", "n_gt", "n_eq", "num", "rank_num", "n_found"))

    def top_pairs_null(self):
        cs = self.cs
        got = self.ctx.top_pairs_null(cs["null_rows"], cs["a"], cs["b"], cs["null_mask"], cs["null_cuts"])
        qs.check_null(got, self.exp.null, (self.tag, "top_pairs_null"))
        return fields(got, ("max_num", "arg_i", "arg_j", "n_reach"))

    def top_pairs_loo(self):
        cs = self.cs
        got = self.ctx.top_pairs_loo(cs["kmax"], cs["a"], cs["b"], cs["loo_mask"])
        exp = self.exp.loo
        assert tlc.same(got, exp), (self.tag, "top_pairs_loo", [f for f in tlc.FIELDS if not np.array_equal(getattr(got, f), getattr(exp, f))])
        return fields(got, tlc.FIELDS)

    def perm_codes(self):
        cs = self.cs
        G = cs["G"]
        before = self.ctx.get_codes(0, G, 0, G)
        got = self.ctx.perm_codes(cs["perm_rows"][0], cs["perm_k"])
        assert np.array_equal(self.ctx.get_codes(0, G, 0, G), before), (self.tag, "the resident table changed under reo_perm_codes")
        want = self.exp.perm_codes(0)
        assert got.shape == (G, G) and np.array_equal(got, want), (self.tag, "perm_codes", int((got != want).sum()), np.argwhere(got != want)[:4].tolist())
        return (got,)

    def perm_null(self):
        """the first and the last relabelling against one pass of oracle.iterate on perm_null_cases.permuted_codes; the resident table
        read before and after"""
        cs = self.cs
        G, rows, ref = cs["G"], cs["perm_rows"], cs["perm_ref"]
        before = self.ctx.get_codes(0, G, 0, G)
        pn = self.ctx.permutation_null(rows, k=cs["perm_k"], ref_mask=ref, pval_deg=qs.CALLS_PVAL, padj_deg=qs.CALLS_PADJ, keep_null=True)
        assert np.array_equal(self.ctx.get_codes(0, G, 0, G), before), (self.tag, "the resident table changed under reo_perm_null")
        self.ref = None                                                          # (reo_get_ref_mask is refused until the next identify_degs)
        tag = (self.tag, "perm_null")
        assert pn.delta1_null.shape == (rows.shape[0], G), tag
        obs = self.exp.one_pass(self.exp.codes, ref, qs.CALLS_PVAL, qs.CALLS_PADJ)
        assert np.allclose(pn.delta1_obs, obs[:, 11], rtol=STAT_RTOL, atol=1e-9), (tag, "delta1_obs")
        for p in (0, rows.shape[0] - 1):
            res = self.exp.one_pass(self.exp.perm_codes(p), ref, qs.CALLS_PVAL, qs.CALLS_PADJ)
            assert np.allclose(pn.delta1_null[p], res[:, 11], rtol=STAT_RTOL, atol=1e-9), (tag, p, np.abs(pn.delta1_null[p] - res[:, 11]).max())
        assert pn.n_ge.dtype == np.int32 and np.array_equal(pn.n_ge, (np.abs(pn.delta1_null) >= np.abs(pn.delta1_obs)[None, :]).sum(axis=0)), tag
        return fields(pn, ("delta1_obs", "n_ge", "n_up", "n_down", "se_null", "delta1_null"))

    def identify_degs(self):
        cs = self.cs
        res, it, trace, last = self.exp.degs
        got, iters, tr = self.ctx.identify_degs(cs["ref0"], qs.PVAL_DEG, qs.PADJ_DEG, cs["n_iter"], 1)
        tag = (self.tag, "identify_degs")
        assert iters == it and tr == trace, (tag, tr, trace)
        assert np.array_equal(got[:, 2:11], res[:, 2:11]), (tag, "tallies")
        assert np.allclose(got[:, :2], res[:, :2], rtol=0, atol=P_ATOL, equal_nan=True), (tag, np.nanmax(np.abs(got[:, :2] - res[:, :2])))
        assert np.allclose(got[:, 11:], res[:, 11:], rtol=STAT_RTOL, atol=1e-9, equal_nan=True), (tag, np.nanmax(np.abs(got[:, 11:] - res[:, 11:])))
        self.ref = last
        assert np.array_equal(self.ctx.ref_mask(), last), (tag, "ref_mask")
        return (got,)


def build(ctx, cs, thr):
    if cs["matrix_first"]:
        ctx.set_matrix(qs.handed_over(cs))
    ctx.set_groups(cs["gid"], cs["ngroups"])
    got = ctx.compute_thresholds(cs["pval_reo"])
    assert np.array_equal(got, thr), (cs["tag"], got.tolist(), thr.tolist())
    if not cs["matrix_first"]:
        ctx.set_matrix(qs.handed_over(cs))
    if cs["table"][0] == "pairs":
        ctx.build_pairs(cs["table"][1])
    else:
        ctx.build_contrast(cs["table"][1], cs["table"][2])


@pytest.mark.parametrize("no", range(qs.SWEEP_CASES))
def test_case(pkg, no):
    cs = qs.case(no)
    ctx = context_for(pkg, no)
    run = Run(pkg, ctx, no)
    build(ctx, cs, run.exp.thr)
    info = ctx.info()
    assert (info["G"], info["S"]) == (cs["G"], cs["S"]) and info["contrast_treat"] == (cs["table"][2] if cs["table"][0] == "contrast" else -1), cs["tag"]
    first = {}
    for step, name in enumerate(cs["order"]):
        try:
            got = getattr(run, name)()
        except AssertionError as err:                                            # (the helpers of other files know no case: name it here)
            raise AssertionError(f"{cs['tag']}, call {step} of {len(cs['order'])} ({name}; reference set {'standing' if run.ref is not None else 'none'}): {err}") from err
        if name in first:                                                        # the call made once more: byte for byte
            assert len(got) == len(first[name]), (cs["tag"], step, name)
            for x, y in zip(got, first[name]):
                assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (cs["tag"], step, name, "the repeated call differs")
        else:
            first[name] = got
    assert sum(cs["order"].count(c) == 2 for c in set(cs["order"])) == 2
    want = qs.null_mask_runs(cs["order"])                                        # the NULL-mask runs that the order calls for were made
    assert run.null_runs == want, (cs["tag"], run.null_runs, want)
    # the state at the end: the table and the reference set as the last call that may change them left them
    G = cs["G"]
    assert np.array_equal(ctx.get_codes(0, G, 0, G), run.exp.codes), (cs["tag"], "the table at the end")
    if run.ref is not None:
        assert np.array_equal(ctx.ref_mask(), run.ref), (cs["tag"], "ref_mask at the end")
    else:
        with pytest.raises(pkg.DimensionMismatch):
            ctx.ref_mask()
    after = ctx.info()
    own = set(TIMERS).union(*(OWN[c] for c in cs["order"]))
    assert all(after[k] == info[k] for k in info if k not in own), (cs["tag"], {k: (info[k], after[k]) for k in info if after[k] != info[k] and k not in own})
