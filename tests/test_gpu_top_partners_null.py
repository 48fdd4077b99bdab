"""The label-permutation null of a gene's best partner score on the GPU (reo_top_partners_null; csrc/toppartnersnull.hip): per label row and
query gene the largest |N| over the gene's partners, the smallest partner that attains it and the partners that reach the gene's cut,
sixteen label rows from one walk over the bit planes.  The expected values come from the numpy restatements of the definition
(tests/top_partners_null_cases.py) and every comparison is exact.  Two identities tie the kernel to its neighbours on the same context:
over all genes the rows reduce to reo_top_pairs_null's answer (I1), and on the observed labels a row's maximum is |N| of the first partner
of reo_top_partners (I2)."""
import importlib
import os

import numpy as np
import pytest

from query_cases import planted_ranks
import top_pairs_cases as tpc
import top_pairs_null_cases as tnc
import top_partners_null_cases as pnc
import wide_top_pairs_cases as wt

pytestmark = pytest.mark.gpu


def open_case(pkg, name, seed=11, cases=tpc):
    """matrix and groups of a named case, nothing else: no thresholds, no class table"""
    X, gid, ng, a, b = cases.case(name)
    ctx = pkg.Context(device=0, seed=seed)
    ctx.set_groups(gid, ng)
    ctx.set_matrix(X)
    return ctx, a, b


def same(got, exp, tag=None):
    """a TopPartnersNull against a PNull of the restatement, field by field"""
    assert got.max_num.dtype == np.int64 and got.arg_partner.dtype == np.int32 and got.n_reach.dtype == np.int32, tag
    assert got.max_num.shape == exp.max_num.shape and np.array_equal(got.max_num, exp.max_num), (tag, got.max_num, exp.max_num)
    assert np.array_equal(got.arg_partner, exp.arg_partner), (tag, got.arg_partner, exp.arg_partner)
    assert got.n_reach.shape == exp.n_reach.shape and np.array_equal(got.n_reach, exp.n_reach), (tag, got.n_reach, exp.n_reach)


def identical(x, y):
    return all(np.array_equal(getattr(x, f), getattr(y, f)) for f in ("genes", "max_num", "arg_partner", "n_reach", "cuts", "side_sizes")) \
        and (x.a, x.b) == (y.a, y.b)


def overall_is(got, glob, tag=None):
    """I1: the rows of a TopPartnersNull reduce to a TopPairsNull"""
    top, gi, gj = got.overall()
    assert np.array_equal(top, glob.max_num) and np.array_equal(gi, glob.arg_i) and np.array_equal(gj, glob.arg_j), (tag, top, gi, gj, glob)
    assert pnc.overall(got.max_num, got.arg_partner, got.genes) == [(int(m), int(i), int(j)) for m, i, j in zip(glob.max_num, glob.arg_i, glob.arg_j)], tag


def launch_batch(B):
    """permutations per launch of B label rows: whole launch groups of 16 above 16"""
    return B if B <= 16 else min(B, 64) // 16 * 16


# ---- 1. the named cases

@pytest.mark.parametrize("name", pnc.NAMES)
def test_every_cell_equals_the_restatement(pkg, name):
    """B = 1, 16, 17 and 33 label rows: less than a launch group, a full one, a launch of 16 and one of 1, two launch groups and one row.
    All genes as queries, and seven rows that pad a row tile, repeat a gene and straddle a column tile"""
    exp, rows, cuts = pnc.expected(name), tnc.rows(name), pnc.cuts(name)
    X = tpc.case(name)[0]
    G = X.shape[0]
    seam = pnc.seam_queries(G)
    ctx, a, b = open_case(pkg, name)
    with ctx:
        if name in ("separated", "count_i64", "count_f32"):                      # the tie-free form of the kernel, and the form with ties
            assert ctx.info()["has_ties"] == (0 if name == "separated" else 1)
        for B in (1, 16, 17, 33):
            got = ctx.top_partners_null(rows[:B], a=a, b=b, cuts=cuts)
            same(got, pnc.select(exp, B), (name, B))
            assert (got.a, got.b) == (a, b) and np.array_equal(got.cuts, cuts) and np.array_equal(got.genes, np.arange(G))
            assert tuple(int(v) for v in got.side_sizes) == tpc.expected(name).sizes
            assert ctx.info()["top_partners_null_batch"] == launch_batch(B) and ctx.info()["top_partners_null_us"] > 0
            few = ctx.top_partners_null(rows[:B], seam, a=a, b=b, cuts=cuts[seam])
            same(few, pnc.select(exp, B, seam), (name, B, "seven rows"))
            assert np.array_equal(few.genes, seam)
        overall_is(got, ctx.top_pairs_null(rows, a=a, b=b), name)                # I1, all 33 rows
        tp = ctx.top_partners(None, 1, a=a, b=b)                                 # I2: the observed row
        assert np.array_equal(got.max_num[0], np.abs(tp.num[:, 0])) and (tp.n_found == 1).all()
        tp7 = ctx.top_partners(seam, 1, a=a, b=b)
        assert np.array_equal(few.max_num[0], np.abs(tp7.num[:, 0]))
        full = 2 * tpc.expected(name).sizes[0] * tpc.expected(name).sizes[1]
        assert np.array_equal(got.max_score, exp.max_num / float(full))
        if name == "level":                                                      # every |N| is 0: partner 1 for gene 0, partner 0 otherwise
            assert not got.max_num.any() and (got.arg_partner[:, 0] == 1).all() and not got.arg_partner[:, 1:].any()
        bare = ctx.top_partners_null(rows[:17], a=a, b=b)                        # no cuts: no counters
        same(bare, pnc.select(exp, 17, None, False), (name, "no cuts"))
        assert bare.n_reach.shape == (17, 0) and bare.cuts.size == 0
        same(ctx.top_partners_null(rows[:17], seam, a=a, b=b), pnc.select(exp, 17, seam, False), (name, "seven rows, no cuts"))


# ---- 2. the partner mask

def test_partner_mask(pkg):
    name = "float300"
    X, gid, ng, a, b = tpc.case(name)
    G = X.shape[0]
    rows, cuts = tnc.rows(name)[:17], pnc.cuts(name)
    mask = tpc.half_mask(G)
    ctx, a, b = open_case(pkg, name)
    with ctx:
        got = ctx.top_partners_null(rows, a=a, b=b, partner_mask=mask, cuts=cuts)   # the queries need not be inside the mask
        same(got, pnc.restate(X, rows, np.arange(G), cuts, mask), "half of the genes")
        assert mask[got.arg_partner].all() and not identical(got, ctx.top_partners_null(rows, a=a, b=b, cuts=cuts))
        same(ctx.top_partners_null(rows, a=a, b=b, partner_mask=np.ones(G, dtype=bool), cuts=cuts), pnc.select(pnc.expected(name), 17), "every gene")
        one = np.zeros(G, dtype=bool)
        one[G - 1] = True
        zero = np.zeros(G, dtype=np.int64)
        alone = ctx.top_partners_null(rows, a=a, b=b, partner_mask=one, cuts=zero)
        same(alone, pnc.restate(X, rows, np.arange(G), zero, one), "one gene")
        assert (alone.max_num[:, G - 1] == -1).all() and (alone.arg_partner[:, G - 1] == -1).all() and not alone.n_reach[:, G - 1].any()
        assert (alone.arg_partner[:, :G - 1] == G - 1).all() and (alone.n_reach[:, :G - 1] == 1).all()   # every other row finds exactly it
        two = one.copy()
        two[3] = True
        pair = ctx.top_partners_null(rows, a=a, b=b, partner_mask=two, cuts=zero)
        same(pair, pnc.restate(X, rows, np.arange(G), zero, two), "two genes")
        assert (pair.arg_partner[:, 3] == G - 1).all() and (pair.arg_partner[:, G - 1] == 3).all() and (pair.n_reach[:, [3, G - 1]] == 1).all()
        members = np.flatnonzero(mask).astype(np.int32)                          # I1 with gene_mask = partner_mask and genes its members
        inside = ctx.top_partners_null(rows, members, a=a, b=b, partner_mask=mask)
        overall_is(inside, ctx.top_pairs_null(rows, a=a, b=b, gene_mask=mask), "inside the half mask")
        bad = np.ones(G, dtype=np.uint8)
        bad[7] = 2
        with pytest.raises(pkg.DimensionMismatch, match=r"reo_top_partners_null: partner_mask\[7\] = 2"):
            ctx.top_partners_null(rows, a=a, b=b, partner_mask=bad)


# ---- 3. position and batch

@pytest.mark.parametrize("name", ["float300", "count_i64", "three_0_2"])
def test_the_outputs_do_not_depend_on_position_or_batch(pkg, monkeypatch, name):
    exp, rows, cuts = pnc.expected(name), tnc.rows(name), pnc.cuts(name)
    G = tpc.case(name)[0].shape[0]
    ctx, a, b = open_case(pkg, name)
    with ctx:
        plain = ctx.top_partners_null(rows, a=a, b=b, cuts=cuts)
        same(plain, exp, name)
        back = ctx.top_partners_null(rows[::-1], a=a, b=b, cuts=cuts)            # a label row's outputs do not depend on its place in the batch
        same(back, pnc.PNull(exp.max_num[::-1], exp.arg_partner[::-1], exp.n_reach[::-1], 0), (name, "rows reversed"))
        rev = np.arange(G - 1, -1, -1, dtype=np.int32)                           # nor a query's on its place among the queries
        turned = ctx.top_partners_null(rows, rev, a=a, b=b, cuts=cuts[rev])
        same(turned, pnc.select(exp, pnc.B_MAX, rev), (name, "queries reversed"))
        for batch, used in ((1, 1), (16, 16), (20, 16)):                         # the seam between launches: read per call
            monkeypatch.setenv("REO_TOP_PARTNERS_NULL_BATCH", str(batch))
            got = ctx.top_partners_null(rows, a=a, b=b, cuts=cuts)
            assert identical(got, plain), (name, batch)
            assert ctx.info()["top_partners_null_batch"] == used
        monkeypatch.setenv("REO_TOP_PARTNERS_NULL_BATCH", "500")                 # it can only lower the batch
        assert identical(ctx.top_partners_null(rows, a=a, b=b, cuts=cuts), plain) and ctx.info()["top_partners_null_batch"] == 32
        monkeypatch.delenv("REO_TOP_PARTNERS_NULL_BATCH")
        assert identical(ctx.top_partners_null(rows, a=a, b=b, cuts=cuts), plain) and ctx.info()["top_partners_null_batch"] == 32


# ---- 4. the plane chains

@pytest.mark.parametrize("G", [4095, 4096, 32767, 32768])
def test_the_12_15_and_16_plane_chains(pkg, G):
    """the kernel is compiled per number of position planes: 12 up to 4 095 genes, 15 up to 32 767, 16 above.  The first gene count of each
    and the last one before it, on a case whose expectation needs no G x G arrays (top_partners_null_cases.moved_restate), under the
    observed labels, the inverted ones and one shuffle; the queries are the six moved genes and three fixed ones"""
    X, gid, moved = tpc.moved_case(G, 31 + G)
    rows = tnc.moved_rows(gid, G)
    genes = np.concatenate([moved, [0, 64, G - 2]]).astype(np.int32)
    assert len(set(genes.tolist())) == 9
    bare = pnc.moved_restate(X, rows, genes)
    cuts = np.where(np.arange(9) % 2 == 0, bare.max_num[0], 1).astype(np.int64)  # the observed maximum, or 1: the partners with N != 0
    exp = pnc.moved_restate(X, rows, genes, cuts)
    with pkg.Context(device=0, seed=11) as ctx:
        ctx.set_groups(gid, 2)
        ctx.set_matrix(X)
        got = ctx.top_partners_null(rows, genes, cuts=cuts)
        glob = ctx.top_pairs_null(rows)
        tp = ctx.top_partners(genes, 1)
    same(got, exp, G)
    assert (got.max_num[:, :6] > 0).all() and (got.n_reach[0, 0::2] >= 1).all()
    overall_is(got, glob, G)                                                     # only pairs with a moved gene have N != 0: their rows hold the maximum
    assert np.array_equal(got.max_num[0], np.abs(tp.num[:, 0]))


# ---- 5. wide sample axes

WIDE = ["seam", "full_ranks", "three_33_31", "padding_20_30", "contrast_300_260"]


def wide_cuts(counts0, row0, G):
    """one cut per gene from the observed row: 300 (a count above 255 decides it), the gene's own maximum, 0 -- by gene index modulo 3"""
    mx = pnc.from_counts(counts0, row0, np.arange(G)).max_num[0]
    return np.where(np.arange(G) % 3 == 0, 300, np.where(np.arange(G) % 3 == 1, mx, 0)).astype(np.int64)


@pytest.mark.parametrize("name", WIDE)
def test_wide_sample_axes(pkg, name):
    """33 label rows over 10 to 21 sample blocks: the tie-free form over 16 blocks (full_ranks), groups on neither side and live words with
    no bit (three_33_31, padding_20_30, contrast_300_260), counts above 255"""
    X, gid, ng, a, b = wt.case(name)
    G = X.shape[0]
    rows = wt.rows(name)
    counts = wt.row_counts(X, rows)
    cuts = wide_cuts(tuple(c[:1] for c in counts), rows[:1], G)
    exp = pnc.from_counts(counts, rows, np.arange(G), cuts)
    if name == "contrast_300_260":
        assert max(int(c.max()) for c in counts) > 255                           # a count that no 8-bit counter holds
    ctx, a, b = open_case(pkg, name, cases=wt)
    with ctx:
        assert ctx.info()["sample_slots"] // 32 == wt.blocks(name) >= 10
        got = ctx.top_partners_null(rows, a=a, b=b, cuts=cuts)
        if name == "full_ranks":
            assert ctx.info()["has_ties"] == 0 and wt.blocks(name) == 16
        glob = ctx.top_pairs_null(rows, a=a, b=b)
    same(got, exp, name)
    overall_is(got, glob, name)
    assert tuple(int(v) for v in got.side_sizes) == wt.expected(name).sizes


def test_the_sample_limit(pkg):
    """S = 65 535, 2 048 blocks, |N| up to 2 S_A S_B = 2^31 - 65 536: the observed row and two shuffles, every gene a query; the cuts hold
    2 S_A S_B, which the separated genes' rows reach on the observed row, and 2 S_A S_B + 1"""
    name = "limit"
    X, gid, ng, a, b = wt.case(name)
    G = X.shape[0]
    rows = wt.deep_rows(name)
    full = 2 ** 31 - 65536
    cuts = np.where(np.arange(G) % 2 == 0, full, full + 1).astype(np.int64)
    exp = pnc.from_counts(wt._deep_counts(name), rows, np.arange(G), cuts)
    ctx, a, b = open_case(pkg, name, cases=wt)
    with ctx:
        assert ctx.info()["sample_slots"] // 32 == 2048 and ctx.S == 65535
        got = ctx.top_partners_null(rows, a=a, b=b, cuts=cuts)
    same(got, exp, name)
    assert got.max_num[0].max() == full and (got.max_num[0] == full).all()      # every gene has a separated partner on the observed row
    assert got.n_reach[0, 0::2].min() >= 6 and not got.n_reach[:, 1::2].any()
    want = wt.expected_deep_null(name)
    assert pnc.overall(got.max_num, got.arg_partner, got.genes) == [(int(m), int(i), int(j)) for m, i, j in zip(want.max_num, want.arg_i, want.arg_j)]


# ---- 6. a call disturbs nothing

def test_a_call_disturbs_nothing(pkg):
    G, S, seed = 300, 24, 7
    X = planted_ranks(G, S, seed)
    group = pkg.synth.groups(S)
    gid, lev = pkg.encode_groups(group)
    ref0 = pkg.synth.ref_mask(G, 100, seed)
    rows = tnc.shuffled_rows(tnc.observed_row(gid, 0, None), 17, 5)
    genes = np.array([0, 299, 17, 64], dtype=np.int32)
    cuts = np.array([0, 50, 100, 150], dtype=np.int64)
    with pkg.Context(device=0, seed=seed) as ctx:
        ctx.set_groups(gid, len(lev)); ctx.compute_thresholds(0.01); ctx.set_matrix(X); ctx.build_pairs(0)
        first = ctx.identify_degs(ref0, 1.0, 0.05, 8, 1)
        codes, ref, info = ctx.get_codes(0, G, 0, G), ctx.ref_mask(), ctx.info()
        got = ctx.top_partners_null(rows, genes, cuts=cuts)                      # (tie-free data: the gene-order planes are made on demand)
        same(got, pnc.restate(X, rows, genes, cuts), "after a build")
        assert np.array_equal(ctx.get_codes(0, G, 0, G), codes) and np.array_equal(ctx.ref_mask(), ref)
        after = ctx.info()
        own = ("planes_on_demand", "top_partners_null_batch", "top_partners_null_us")   # (the planes it had made, and its own two entries)
        assert all(after[k] == info[k] for k in info if k not in own), {k: (info[k], after[k]) for k in info if after[k] != info[k]}
        assert after["top_partners_null_batch"] == 16 and after["top_partners_null_us"] > 0 and info["top_partners_null_batch"] == 0
        again = ctx.identify_degs(ref0, 1.0, 0.05, 8, 1)
        assert again[1:] == first[1:] and np.array_equal(again[0], first[0], equal_nan=True)


# ---- 7. the refusals

def test_every_refusal_has_its_message_and_writes_nothing(pkg, monkeypatch):
    X, gid, ng, a, b = tpc.case("three_0_2")
    G, S = X.shape
    rows = np.array(tnc.rows("three_0_2")[:3])
    ctx, _, _ = open_case(pkg, "three_0_2")
    with ctx:
        ok = dict(sides=rows, genes=[4, 2], a=0, b=2)
        far = rows.copy(); far[1, 5] = 7
        part = rows.copy(); part[2, np.flatnonzero(rows[2] == 2)[0]] = 0
        gone = rows.copy(); gone[0, np.flatnonzero(rows[0] == 1)[0]] = 2
        more = rows.copy(); more[1, np.flatnonzero(rows[1] == 0)[0]] = 1
        for kw, pattern in ((dict(ok, b=0), "b == a == 0"), (dict(ok, a=3), "a = 3 is outside the groups \\[0, 3\\)"),
                            (dict(ok, b=3), "b = 3 is outside the groups"), (dict(ok, a=-1), "a = -1 is outside"),
                            (dict(ok, sides=rows[:0]), "n_perm = 0, between 1 and 2\\^20"),
                            (dict(ok, genes=[]), "n_genes = 0, between 1 and 2\\^20 query genes"),
                            (dict(ok, sides=np.tile(rows[:1], (257, 1)), genes=np.zeros((1 << 18) + 1, dtype=np.int32)),
                             "n_perm \\* n_genes = 257 x 262145, at most 2\\^26 cells"),
                            (dict(ok, genes=[0, 5, G]), f"genes\\[2\\] = {G} is outside the genes \\[0, {G}\\)"),
                            (dict(ok, genes=[-1]), "genes\\[0\\] = -1 is outside the genes"),
                            (dict(ok, cuts=[3, -2]), "cuts\\[1\\] = -2, a cut of \\|N\\| is not negative"),
                            (dict(ok, sides=far), "row 1 of sides holds the byte 7 in column 5"),
                            (dict(ok, sides=part), "row 2 of sides holds the byte 0 in column \\d+, whose sample is on neither side"),
                            (dict(ok, sides=gone), "row 0 of sides holds the byte 2 in column \\d+, whose sample is on one of the sides"),
                            (dict(ok, sides=more), "row 1 of sides has 21 ones and 11 zeros, side A has 20 samples and side B 12"),
                            (dict(ok, b=None), "row 0 of sides holds the byte 2 in column \\d+, whose sample is on one of the sides"),
                            (dict(ok, partner_mask=np.full(G, 2, dtype=np.uint8)), "partner_mask\\[0\\] = 2, a byte of the mask is 0 or 1")):
            with pytest.raises(pkg.DimensionMismatch, match=pattern) as e:
                ctx.top_partners_null(**kw)
            assert e.value.status == pkg._ffi.REO_EINVAL and "reo_top_partners_null" in e.value.message
        with pytest.raises(pkg.DimensionMismatch, match="sides has shape"):
            ctx.top_partners_null(rows[:, :-1], [4], a=0, b=2)
        with pytest.raises(pkg.DimensionMismatch, match="partner_mask has shape"):
            ctx.top_partners_null(rows, [4], a=0, b=2, partner_mask=np.ones(G + 1, dtype=bool))
        with pytest.raises(pkg.DimensionMismatch, match="cuts has 3 values, one per query gene is 2"):
            ctx.top_partners_null(rows, [4, 2], a=0, b=2, cuts=[1, 2, 3])
        # a refused call writes nothing; n_reach is null exactly when cuts is
        P = pkg._ffi._ptr
        call, h = ctx._L.reo_top_partners_null, ctx._h
        genes, bad_genes = np.array([4, 2], dtype=np.int32), np.array([4, G], dtype=np.int32)
        mx, ap, reach = np.full((3, 2), -7, dtype=np.int64), np.full((3, 2), -7, dtype=np.int32), np.full((3, 2), -7, dtype=np.int32)
        cuts, neg = np.array([0, 5], dtype=np.int64), np.array([0, -5], dtype=np.int64)
        bad_mask = np.ones(G, dtype=np.uint8)
        bad_mask[G - 1] = 3
        for args, pattern in (((2, 2, P(rows), 3, P(genes), 2, None, P(cuts), P(mx), P(ap), P(reach)), "b == a"),
                              ((0, 2, None, 3, P(genes), 2, None, P(cuts), P(mx), P(ap), P(reach)), "must not be null"),
                              ((0, 2, P(rows), 3, None, 2, None, P(cuts), P(mx), P(ap), P(reach)), "must not be null"),
                              ((0, 2, P(rows), 3, P(genes), 2, None, P(cuts), None, P(ap), P(reach)), "must not be null"),
                              ((0, 2, P(rows), 3, P(genes), 2, None, P(cuts), P(mx), None, P(reach)), "must not be null"),
                              ((0, 2, P(rows), 3, P(genes), 2, None, P(cuts), P(mx), P(ap), None), "n_reach is null and cuts is not"),
                              ((0, 2, P(rows), 3, P(genes), 2, None, None, P(mx), P(ap), P(reach)), "cuts is null and n_reach is not"),
                              ((0, 2, P(rows), 3, P(genes), 2, None, P(neg), P(mx), P(ap), P(reach)), "cuts\\[1\\] = -5"),
                              ((0, 2, P(far), 3, P(genes), 2, None, P(cuts), P(mx), P(ap), P(reach)), "holds the byte 7"),
                              ((0, 2, P(rows), (1 << 20) + 1, P(genes), 2, None, P(cuts), P(mx), P(ap), P(reach)), "n_perm = 1048577"),
                              ((0, 2, P(rows), 3, P(genes), (1 << 20) + 1, None, P(cuts), P(mx), P(ap), P(reach)), "n_genes = 1048577"),
                              ((0, 2, P(rows), 1 << 13, P(genes), (1 << 13) + 1, None, P(cuts), P(mx), P(ap), P(reach)), "at most 2\\^26 cells"),
                              ((0, 2, P(rows), 3, P(bad_genes), 2, None, P(cuts), P(mx), P(ap), P(reach)), f"genes\\[1\\] = {G}"),
                              ((0, 2, P(rows), 3, P(genes), 2, P(bad_mask), P(cuts), P(mx), P(ap), P(reach)), f"partner_mask\\[{G - 1}\\] = 3")):
            with pytest.raises(pkg.DimensionMismatch, match=pattern):
                pkg._ffi.check(call(h, *args))
        assert (mx == -7).all() and (ap == -7).all() and (reach == -7).all()
        exp = pnc.select(pnc.expected("three_0_2"), 3, genes)
        pkg._ffi.check(call(h, 0, 2, P(rows), 3, P(genes), 2, None, None, P(mx), P(ap), None))   # cuts and n_reach are optional, together
        assert np.array_equal(mx, exp.max_num) and np.array_equal(ap, exp.arg_partner) and (reach == -7).all()
        ctx.set_valid_mask(np.ones((G, S), dtype=bool))
        with pytest.raises(pkg.DimensionMismatch, match="reo_top_partners_null compares on the bit planes of the whole matrix.*while a mask is set"):
            ctx.top_partners_null(**ok)
        ctx.set_valid_mask(None)
        same(ctx.top_partners_null(**ok), pnc.select(exp, 3, None, False), "mask cleared")
        ctx.set_shard(0, 2)
        with pytest.raises(pkg.DimensionMismatch, match="reo_top_partners_null is not available on a sharded context"):
            ctx.top_partners_null(**ok)
    with pkg.Context(device=0, seed=1) as ctx:                                   # no matrix, no groups
        with pytest.raises(pkg.DimensionMismatch, match="no expression matrix"):
            ctx.top_partners_null(np.zeros((1, 0), dtype=np.uint8), [0])
    monkeypatch.setenv("REO_MULTI_ONE_DEVICE", "1")
    with pkg.Context(seed=1, n_gpus=2) as ctx:
        ctx.set_matrix(X)
        with pytest.raises(pkg.DimensionMismatch, match="reo_top_partners_null is not available on a reo_create_multi context"):
            ctx.top_partners_null(rows, [0], a=0, b=2)


# ---- 8. the run and the file

def test_run_identify_degs_carries_the_null(pkg):
    m, B = 3, 17
    seed = 0x5EED0001
    R = importlib.import_module(pkg.__name__ + ".reoa")
    golden = os.path.join(os.path.dirname(__file__), "golden")
    prep = R.prepare(os.path.join(golden, "fn_expr.txt"), os.path.join(golden, "fn_meta.txt"), seed=seed)
    args = (prep["data"], prep["sample_groups"], prep["gene_names"], 0.01, 1.0, 0.05, prep["ref"], 128, 5)
    # two groups: the dict's TopPartnersNull equals a direct call with the rows of permuted_sides and the cuts of the rows' last partners
    plain = pkg.run_identify_degs(*args, seed=seed, device=0)
    on = pkg.run_identify_degs(*args, seed=seed, device=0, top_partners=m, top_partners_permutations=B, perm_seed=4)
    assert set(on.comparisons[0]) == set(plain.comparisons[0]) | {"top_partners", "top_partners_null"}
    assert np.array_equal(on.result, plain.result, equal_nan=True) and on.trace == plain.trace
    tp, got = on.comparisons[0]["top_partners"], on.comparisons[0]["top_partners_null"]
    degs = np.flatnonzero(on.labels != "no change").astype(np.int32)
    assert degs.size > 0 and np.array_equal(got.genes, degs) and got.max_num.shape == (B, degs.size) and (got.a, got.b) == (0, None)
    gid, lev = pkg.encode_groups(prep["sample_groups"])
    rows = pkg.permuted_sides(gid, 0, None, B, seed=4)
    cuts = np.abs(tp.num[:, m - 1])
    assert (tp.n_found == m).all() and np.array_equal(got.cuts, cuts)
    with pkg.Context(device=0, seed=seed) as ctx:
        ctx.set_groups(gid, len(lev))
        ctx.set_matrix(np.asarray(prep["data"]))
        direct = ctx.top_partners_null(rows, degs, cuts=cuts)
        info = ctx.info()
        none_tp = pkg.hotpath.deg_top_partners(ctx, np.full(len(prep["gene_names"]), "no change", dtype=object), 0, None, m)["top_partners"]
        none = pkg.hotpath.deg_top_partners_null(ctx, gid, 0, None, none_tp, B, 4, None)["top_partners_null"]
        assert ctx.info() == info                                                # a comparison without DEGs: an empty object, no library call
    assert identical(got, direct)
    sel = np.unique(np.concatenate([np.arange(min(40, degs.size)), np.arange(max(degs.size - 10, 0), degs.size)]))   # (20 000 genes: no G x G arrays,
    want = pnc.query_restate(np.asarray(prep["data"]), rows, degs[sel], cuts[sel])                                    #  and the first and last DEGs)
    same(got._replace(max_num=got.max_num[:, sel], arg_partner=got.arg_partner[:, sel], n_reach=got.n_reach[:, sel]), want, "two groups")
    assert none.max_num.shape == (B, 0) and none.arg_partner.shape == (B, 0) and none.n_reach.shape == (B, 0) and none.genes.size == 0
    assert none.p_row(none_tp).shape == (0, m) and [v.tolist() for v in none.overall()] == [[-1] * B] * 3
    p = got.p_row(tp)
    assert p.shape == (degs.size, m) and p.min() >= 1.0 / (1 + B) and p.max() <= 1.0 and (np.diff(p, axis=1) >= 0).all()
    assert (got.p_max(tp) >= p).all()
    # three groups, one contrast: the samples of group 1 take no part; strata are honoured (padj_deg = 0.5: at 0.05 this case has no DEG)
    X, gid, ng, _, _ = tpc.case("three_0_2")
    G = X.shape[0]
    strata = np.arange(gid.size) % 2
    args = (X, gid.tolist(), [f"g{i}" for i in range(G)], 0.01, 1.0, 0.5, np.ones(G, dtype=bool), 3, 1)
    plain = pkg.run_identify_degs(*args, seed=3, device=0, contrasts=[(0, 2)])
    run = pkg.run_identify_degs(*args, seed=3, device=0, contrasts=[(0, 2)], top_partners=m, top_partners_permutations=B, perm_seed=9, perm_strata=strata)
    assert np.array_equal(run.result, plain.result, equal_nan=True) and run.trace == plain.trace and len(run.comparisons) == 1
    tp, got = run.comparisons[0]["top_partners"], run.comparisons[0]["top_partners_null"]
    degs = np.flatnonzero(run.labels != "no change").astype(np.int32)
    rows = pkg.permuted_sides(gid, 0, 2, B, seed=9, strata=strata)
    print("DEGs of the contrast:", degs.size)
    assert degs.size > 0 and (got.a, got.b) == (0, 2) and (rows[:, gid == 1] == 2).all() and np.array_equal(got.genes, degs)
    same(got, pnc.restate(X, rows, degs, np.abs(tp.num[:, m - 1])), "contrast (0, 2)")
    p = got.p_row(tp)
    assert p.min() >= 1.0 / (1 + B) and p.max() <= 1.0 and (np.diff(p, axis=1) >= 0).all()


def test_reoa_writes_a_top_partners_null_file(pkg, tmp_path):
    (tmp_path / "on").mkdir(); (tmp_path / "off").mkdir()
    df = pkg.reoa(use_testdata="yes", work_dir=str(tmp_path / "on"), seed=0x5EED0001, device=0, top_partners=3, top_partners_permutations=16)
    pkg.reoa(use_testdata="yes", work_dir=str(tmp_path / "off"), seed=0x5EED0001, device=0, top_partners=3)
    run = df.attrs["run"]
    tp, null = run.comparisons[0]["top_partners"], run.comparisons[0]["top_partners_null"]
    assert null.max_num.shape == (16, tp.genes.size) and tp.genes.size > 0 and np.array_equal(null.cuts, np.abs(tp.num[:, 2]))
    lines = (tmp_path / "on" / "fn_expr_group1_group2_top_partners_null.tsv").read_text().split("\n")
    assert lines[0].split("\t") == ["gene", "rank", "partner", "num", "score", "rank_num", "gt_A", "eq_A", "gt_B", "eq_B", "p_row"]
    assert lines[-1] == "" and len(lines) == 3 * tp.genes.size + 2
    p = np.array([float(l.split("\t")[10]) for l in lines[1:-1]]).reshape(-1, 3)
    assert np.array_equal(p, null.p_row(tp)) and (np.diff(p, axis=1) >= 0).all() and p.min() >= 1.0 / 17
    partners = (tmp_path / "on" / "fn_expr_group1_group2_top_partners.tsv").read_bytes()
    assert partners == (tmp_path / "off" / "fn_expr_group1_group2_top_partners.tsv").read_bytes()
    assert [l.split("\t")[:10] for l in lines[:-1]] == [l.split("\t") for l in partners.decode().split("\n")[:-1]]
    assert not (tmp_path / "off" / "fn_expr_group1_group2_top_partners_null.tsv").exists()
