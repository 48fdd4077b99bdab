"""Holds the query sweep (tests/query_sweep_cases.py, run by tests/test_gpu_query_sweep.py) to its purpose, on the CPU: the cases are
deterministic; the numpy oracles alone show what the cases cover, so the GPU test cannot pass vacuously; the bit-packed counts that keep
the restatements affordable equal the restatements' own; and every comparison the GPU test makes fails on a planted error."""
import math
import time

import numpy as np
import pytest

import masked_pairs_cases as mpc
import query_sweep_cases as qs
import sample_counts_cases as scc
import sample_tests_cases as stc
import top_pairs_cases as tpc
import top_pairs_loo_cases as tlc
import top_pairs_null_cases as tpnc
import top_partners_cases as tprc
from test_gpu_pair_list import same as same_list
from test_gpu_sample_counts import same as same_counts
from test_gpu_sample_tests import same_integers


# ---- a. determinism

def test_the_sweep_is_pinned_and_deterministic():
    assert (qs.SWEEP_SEED, qs.SWEEP_CASES) == (20261021, 24) and len(qs.sweep()) == 24
    for no in range(qs.SWEEP_CASES):
        one, two = qs.random_case(no), qs.random_case(no)
        assert one.keys() == two.keys()
        for k in one:
            x, y = one[k], two[k]
            if isinstance(x, np.ndarray):
                assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (no, k)
            else:
                assert x == y and type(x) is type(y), (no, k)
        assert qs.case(no)["no"] == no


def test_the_shape_of_every_case():
    tiny = 0
    for cs in qs.sweep():
        G, S, q = cs["G"], cs["S"], cs["queries"]
        tiny += G in (2, 3)
        assert G in (2, 3) or 33 <= G <= 700, cs["tag"]
        assert 2 <= cs["ngroups"] <= 5 and S == sum(cs["sizes"]) <= qs.S_MAX and cs["gid"][0] == 0, cs["tag"]
        seen = []                                                                # the labels number the groups in order of first appearance
        for g in cs["gid"].tolist():
            if g not in seen:
                seen.append(g)
        assert seen == list(range(cs["ngroups"])) and np.bincount(cs["gid"]).tolist() == cs["sizes"], cs["tag"]
        assert 2 <= q.size <= 40 and 0 in q and G - 1 in q and q.min() >= 0 and q.max() < G, cs["tag"]
        assert cs["X"].shape == (G, S) and cs["X"].dtype == {"float64_band": np.float64, "ranks": np.int64, "int64_ties": np.int64,
                                                              "int32_ties": np.int32, "float32_band": np.float32, "level": np.int64}[cs["kind"]]
        assert 3 <= cs["null_rows"].shape[0] <= 9 and 3 <= cs["perm_rows"].shape[0] <= 9
        assert (cs["perm_rows"].sum(axis=1) == cs["sizes"][cs["perm_k"]]).all() and np.array_equal(cs["null_rows"][0], tpnc.observed_row(cs["gid"], cs["a"], cs["b"]))
        s_a, s_b = qs.side_sizes(cs)
        assert min(s_a, s_b) >= 2 and 1 <= cs["kmax"] <= 64 and 1 <= cs["m"] <= 1024 and 1 <= cs["n"] <= 1 << 20, cs["tag"]
        order = cs["order"]
        left_out = {c for c in qs.CALLS if c not in order}
        assert left_out == ({"identify_degs", "perm_null"} if G < 10 else {"perm_null"} if cs["table"][0] == "contrast" else set()), cs["tag"]
        assert sorted(order.count(c) for c in set(order)) == [1] * (len(set(order)) - 2) + [2, 2], cs["tag"]
    assert tiny == 2
    assert sum(q["queries"].size % 8 != 0 for q in qs.sweep()) >= 18               # mostly no multiple of kTpRows
    assert sum(len(np.unique(q["queries"])) < q["queries"].size for q in qs.sweep()) >= 16
    assert sum(cs["form"] != "colmajor" for cs in qs.sweep()) >= 8                 # a third and more go up row-major or sparse
    assert {cs["form"] for cs in qs.sweep()} == set(qs.FORMS) and {cs["pval_reo"] for cs in qs.sweep()} == {0.01, 0.05, 0.1}


# ---- b. what the cases cover, from the oracles alone

@pytest.fixture(scope="module")
def survey():
    rows, t0 = [], time.time()
    for no in range(qs.SWEEP_CASES):
        cs, e = qs.case(no), qs.Expect(no)
        m = cs["m"]
        by_gamma = by_index = short_m = False
        for r in e.partners():
            k = min(m + 1, r.partner.size)                                       # the listed partners and the first one left out
            same_n = np.abs(r.num[1:k]) == np.abs(r.num[:k - 1])
            by_gamma |= bool((same_n & (r.rank_num[1:k] != r.rank_num[:k - 1])).any())
            by_index |= bool((same_n & (r.rank_num[1:k] == r.rank_num[:k - 1])).any())
            short_m |= r.partner.size < m
        st = e.sample_tests(cs["sample_tests_mask"])
        rows.append(dict(no=no, ties=bool(e.top.counts[:, 1::2].any()), by_gamma=by_gamma, by_index=by_index,
                         short=short_m or e.top_masked.gene_i.size < cs["n"], both=bool(st["rev_up"].any() and st["rev_down"].any()),
                         nine=set(range(9)) <= set(np.unique(e.codes).tolist())))
    print(f"query sweep: codes, searches, partner rows and sample tests of {qs.SWEEP_CASES} cases restated in {time.time() - t0:.1f} s")
    return rows


def test_coverage_conditions(survey):
    cases = qs.sweep()
    count = lambda key: sum(bool(r[key]) for r in survey)                         # noqa: E731
    kinds = [cs["kind"] for cs in cases]
    assert all(kinds.count(k) >= 4 for k in qs.KINDS), kinds
    assert count("ties") >= 16, count("ties")
    many = [cs for cs in cases if cs["ngroups"] >= 3]
    assert len(many) >= 8 and sum(cs["b"] is not None for cs in many) >= 4          # b a group, three or more groups: one on neither side
    assert sum(cs["interleaved"] for cs in cases) >= 10
    assert sum(any(n % 32 == 0 for n in cs["sizes"]) and any(n % 32 for n in cs["sizes"]) for cs in cases) >= 6
    assert count("by_gamma") >= 8 and count("by_index") >= 4, (count("by_gamma"), count("by_index"))
    assert count("short") >= 6, count("short")
    assert count("both") >= 8, count("both")
    assert count("nine") >= 12, count("nine")
    before, after = set(), set()
    for cs in cases:
        o = cs["order"]
        if "identify_degs" in o:
            first, last = o.index("identify_degs"), len(o) - 1 - o[::-1].index("identify_degs")
            before |= set(o[:last])
            after |= set(o[first + 1:])
    assert before == after == set(qs.CALLS), (set(qs.CALLS) - before, set(qs.CALLS) - after)
    runs = [qs.null_mask_runs(cs["order"]) for cs in cases]                      # the NULL partner mask: in most cases, every table query
    assert sum(r > 0 for r in runs) >= 12 and sum(runs) >= 24, runs
    assert all(any(qs.null_mask_runs(cs["order"][: i + 1]) > qs.null_mask_runs(cs["order"][:i]) for cs in cases for i, c in enumerate(cs["order"]) if c == name)
               for name in qs.TABLE_QUERIES)


# ---- the bit-packed counts equal the restatements' own

@pytest.mark.parametrize("no", [15, 19])
def test_counts_equal_the_restatements(no):
    """a level Int64 case and a Float32 case of 44 genes: masked_counts under the case's labels, under a relabelling and under two
    leave-one-out folds (the sums one sample away from one already made), and states for the queried rows"""
    cs = qs.case(no)
    assert cs["G"] == 44 and cs["kind"] == ("level" if no == 15 else "float32_band")
    X, gid, ng = cs["Xo"], cs["gid"], cs["ngroups"]
    c = qs.Counts(X)
    ones = np.ones(X.shape, dtype=bool)
    side = tlc.sides_of(gid, ng, cs["a"], cs["b"])
    folds = np.flatnonzero(side != 2)[[0, -1]]
    labellings = [(gid, ng), (tpnc.relabel(cs["null_rows"][1]), 3)] + [(tlc.fold_groups(side, int(s)), 3) for s in folds]
    for g, n in labellings:
        want = mpc.masked_counts(X, ones, g, n)
        got = c.masked_counts(X, ones, g, n)
        assert all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(got, want))
    assert len(c.summed) < sum(n for _, n in labellings)                          # some came from a neighbour
    q = cs["queries"][:6]
    want, got = scc.states(X, q), c.states(X, q)
    assert all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(got, want))
    with qs.fast(c):                                                             # and through the restatements as they are called
        quick = tpc.oracle(X, gid, ng, cs["a"], cs["b"])
    assert mpc.masked_counts is not c.masked_counts and scc.states is not c.states
    plain = tpc.oracle(X, gid, ng, cs["a"], cs["b"])
    assert all(np.array_equal(x, y) for x, y in zip(quick[:6], plain[:6])) and quick.sizes == plain.sizes


def test_permuted_codes_of_the_observed_row_is_the_table():
    """the two routes to a class table agree where they meet: perm_null_cases.permuted_codes of the observed labels of a two-group case is
    oracle.build_codes of comparison k"""
    no = next(cs["no"] for cs in qs.sweep() if cs["ngroups"] == 2 and cs["table"][0] == "pairs" and cs["kind"] != "float32_band" and cs["G"] <= 120)
    cs, e = qs.case(no), qs.Expect(no)
    k = cs["perm_k"]
    row = (cs["gid"] == k).astype(np.uint8)
    with qs.fast(e.cnt):
        import perm_null_cases as pnc
        got = pnc.permuted_codes(cs["Xo"], row, (int(e.thr[0, k]), int(e.thr[1, k])), cs["ctx_seed"])
    if k == 0:                                                                   # (the coins are keyed by side: side A is group 0 only for k = 0)
        assert np.array_equal(got, e.codes)
    assert got.shape == e.codes.shape and (np.diag(got) == 255).all()


# ---- c. the comparison can fail

def planted_case():
    """the first tie-rich case with three or more groups, sides of different sizes and a repeated query, with every mask of the planted
    errors set to one that bites: two genes in three, the first queried gene left out"""
    for base in qs.sweep():
        s_a, s_b = qs.side_sizes(base)
        q = base["queries"]
        if base["kind"] in ("int64_ties", "int32_ties") and 60 <= base["G"] <= 300 and base["ngroups"] >= 3 and s_a != s_b and len(np.unique(q)) < q.size:
            mask = np.arange(base["G"]) % 3 != 0
            mask[q[0]] = False
            cs = dict(base, m=12, n=200)
            for name in ("top_partners_mask", "top_pairs_mask", "pair_list_mask", "sample_counts_mask", "sample_tests_mask"):
                cs[name] = mask
            cs["pair_list_classes"] = cs["sample_counts_classes"] = 0x1FF
            return cs
    raise AssertionError("no case of the sweep serves the planted errors")


def answers(pkg, e, cs, queries=None, masks=True, flip=None, swap_sizes=False):
    """what the library must return on a case, as the package's own result objects, from the oracles -- with the planted error asked for"""
    q = cs["queries"] if queries is None else queries
    keep = lambda m: m if masks else None                                        # noqa: E731
    ones = np.ones(cs["G"], dtype=bool)
    pm = lambda name: cs[name] if masks else ones                                # noqa: E731
    s_a, s_b = qs.side_sizes(cs)
    rows = e.partners(q, keep(cs["top_partners_mask"]))
    if flip is not None:                                                         # one row as "partner above query"
        r = rows[flip]
        c = r.counts.copy()
        c[:, 0], c[:, 2] = s_a - r.counts[:, 0] - r.counts[:, 1], s_b - r.counts[:, 2] - r.counts[:, 3]
        rows[flip] = tprc.Row(r.partner, c, -r.num, r.rank_num)
    if swap_sizes:
        rows = [tprc.Row(r.partner, r.counts, (2 * r.counts[:, 0].astype(np.int64) + r.counts[:, 1] - s_a) * s_a
                         - (2 * r.counts[:, 2].astype(np.int64) + r.counts[:, 3] - s_b) * s_b, r.rank_num) for r in rows]
    partner, counts, num, gam, found = tprc.table(rows, cs["m"])
    out = {"top_partners": pkg.TopPartners(q, partner, counts[:, :, 0::2], counts[:, :, 1::2], num, gam, found, np.array([s_a, s_b]), cs["a"], cs["b"])}
    o = e.top_masked if masks else e.top
    n = min(cs["n"], o.gene_i.size)
    c, num = o.counts[:n].copy(), o.num[:n].copy()
    if flip is not None and n:
        c[0, 0], c[0, 2], num[0] = s_a - c[0, 0] - c[0, 1], s_b - c[0, 2] - c[0, 3], -num[0]
    if swap_sizes:
        num = (2 * c[:, 0].astype(np.int64) + c[:, 1] - s_a) * s_a - (2 * c[:, 2].astype(np.int64) + c[:, 3] - s_b) * s_b
    out["top_pairs"] = pkg.TopPairs(o.gene_i[:n], o.gene_j[:n], c[:, 0::2], c[:, 1::2], num, o.rank_num[:n], np.array([s_a, s_b]), cs["a"], cs["b"], 1)
    sub = qs.Expect(dict(cs, queries=q)) if queries is not None else e           # (the rows of another query list)
    sub.__dict__.setdefault("codes", e.codes)
    sub.__dict__.setdefault("cnt", e.cnt)
    rowptr, part, code = sub.pair_list(pm("pair_list_mask"))
    out["pair_list"] = pkg.PairList(q, rowptr, part, code)
    n_sel, n_gt, n_eq = sub.sample_counts(pm("sample_counts_mask"))
    out["sample_counts"] = pkg.SampleCounts(q, n_sel, n_gt, n_eq)
    st = sub.sample_tests(pm("sample_tests_mask"))
    p_up, p_down = np.ones(st["u"].shape), np.ones(st["u"].shape)
    for idx in np.ndindex(st["u"].shape):
        up, down, total = stc.exact_tails(st["n_above_ctrl"][idx[0]], st["n_below_ctrl"][idx[0]], st["u"][idx], st["d"][idx])
        p_up[idx], p_down[idx] = up / total, down / total
    out["sample_tests"] = (pkg.SampleTests(q, st["n_above_ctrl"], st["n_below_ctrl"], st["rev_up"], st["rev_down"], st["tied"], p_up, p_down), st)
    return out


def compare(got, e, cs, which):
    """the comparisons of tests/test_gpu_query_sweep.py, by name; raises AssertionError where they fail"""
    if which == "top_partners":
        tprc.check_table(got["top_partners"], e.partners(), cs["m"])
    elif which == "top_pairs":
        qs.check_top_pairs(got["top_pairs"], e.top_masked, cs["n"])
    elif which == "pair_list":
        same_list(got["pair_list"], e.pair_list(cs["pair_list_mask"]))
    elif which == "sample_counts":
        same_counts(got["sample_counts"], e.sample_counts(cs["sample_counts_mask"]))
    elif which == "same_integers":
        same_integers(got["sample_tests"][0], e.sample_tests(cs["sample_tests_mask"]))
    else:
        assert which == "check_tails"
        st, exp = got["sample_tests"][0], e.sample_tests(cs["sample_tests_mask"])
        assert st.p_up.shape == exp["u"].shape
        stc.check_tails(st.p_up, st.p_down, exp["n_above_ctrl"][:, None], exp["n_below_ctrl"][:, None], exp["u"], exp["d"], stc.tolerance(cs["G"]))


ALL = ("top_partners", "top_pairs", "pair_list", "sample_counts", "same_integers", "check_tails")


def test_every_planted_error_fails_the_comparison(pkg):
    cs = planted_case()
    e = qs.Expect(cs)
    s_a, s_b = qs.side_sizes(cs)
    assert cs["ngroups"] >= 3 and e.top.counts[:, 1::2].any()
    good = answers(pkg, e, cs)
    for which in ALL:                                                            # the oracle's own output passes
        compare(good, e, cs, which)
    assert tlc.same(e.loo, e.loo) and qs.check_null(e.null, e.null) is None

    def fails(got, names, why):
        for which in names:
            with pytest.raises(AssertionError):
                compare(got, e, cs, which)
                print(f"planted error not seen: {why}: {which}")

    # two samples' columns swapped before the oracle runs: one of side A, one of side B that differ
    side = tpnc.observed_row(cs["gid"], cs["a"], cs["b"])
    sa, sb = next((int(x), int(y)) for x in np.flatnonzero(side == 1) for y in np.flatnonzero(side == 0)
                  if (cs["Xo"][:, x] != cs["Xo"][:, y]).sum() > cs["G"] // 2)
    Xs = np.array(cs["Xo"])
    Xs[:, [sa, sb]] = Xs[:, [sb, sa]]
    es = qs.Expect(dict(cs, Xo=np.asfortranarray(Xs)))
    fails(answers(pkg, es, cs), ("top_partners", "top_pairs", "sample_counts", "same_integers", "check_tails"), "columns swapped")
    assert not tlc.same(es.loo, e.loo)
    with pytest.raises(AssertionError):
        qs.check_null(es.null, e.null)
    # the partner mask dropped
    fails(answers(pkg, e, cs, masks=False), ALL, "mask dropped")
    # one row's orientation flipped: a row that has a partner with N != 0
    flip = next(r for r, row in enumerate(e.partners()) if row.num[: cs["m"]].any())
    fails(answers(pkg, e, cs, flip=flip), ("top_partners",) + (("top_pairs",) if e.top_masked.num[0] else ()), "orientation flipped")
    # the side sizes exchanged
    assert s_a != s_b
    fails(answers(pkg, e, cs, swap_sizes=True), ("top_partners", "top_pairs"), "side sizes exchanged")
    # a query list with its repeats removed
    _, at = np.unique(cs["queries"], return_index=True)
    once = cs["queries"][np.sort(at)]
    assert once.size < cs["queries"].size
    fails(answers(pkg, e, cs, queries=once), ("top_partners", "pair_list", "sample_counts", "same_integers", "check_tails"), "repeats removed")


def test_exact_tails_feed_check_tails():
    """the tails that the planted-error test hands to check_tails are exact to a rounding: a table by hand"""
    up, down, total = stc.exact_tails(3, 2, 2, 1)                                # N = 8, K = 5, n = 3: P(X >= 2) = (30 + 10) / 56
    assert (up, down, total) == (40, 46, math.comb(8, 3))
