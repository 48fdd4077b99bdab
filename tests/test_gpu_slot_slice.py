"""A slot build's operands straight from the 16-bit position rows (kernels.hip, k1_slot_slice; index rule: csrc/k1_slots.h, slot_slice_*),
and the gene-order bit planes on demand (transform.hip, ensure_planes).

a. The class table of the default build is, bit for bit, that of a build under REO_K1_SLOT_SLICE=0 (gene-order planes made by the
   transform, then k1_slot_gather) and the oracle's; k1_half_tiles_separated is equal; info()["k1_slot_slice"] is 1 and 0.  Whole tables
   up to 2 049 genes; above, sampled blocks against the oracle and blocks and tallies (which read every word of the table) between the
   builds.  The planted matrices separate items on both sides, so a slot misplaced by k1_slot_slice changes counts that are looped over
   and constants alike.
b. After a slot build the planes are unmade (info()["planes_on_demand"] == 0): the first reader makes them once, and every reader gives
   what a context under REO_K1_SLOTS=0 gives.
c. Tie-rich data on a slot-eligible shape: planes made in the transform, identity order.
d. One context across tie-free and tie-rich matrices; the pipelined upload (groups before the matrix)."""
import numpy as np
import pytest

import slot_cases as sc
import slot_sides_cases as ss
from test_gpu_parity import _expected_block_codes
from test_gpu_slot_matrix import _host, _open

pytestmark = pytest.mark.gpu

ENV = ("REO_K1_SLOTS", "REO_K1_WORKERS", "REO_K1_QUEUE", "REO_ROWMAJOR", "REO_K1_UNSLOT", "REO_K1_SLOT_SIDES", "REO_K1_SLOT_SLICE")
SEED = 3
WHOLE = 2049   # genes up to which a case compares whole tables


def _env(monkeypatch, **env):
    """REO_K1_<NAME> = value for every keyword, everything else of ENV unset"""
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    for name, v in env.items():
        monkeypatch.setenv("REO_K1_" + name.upper(), str(v))


def _blocks(G):
    if G <= WHOLE:
        return [(0, G, 0, G)]
    return [(0, 16, 0, 128), (G - 16, G, G - 128, G), (0, 48, G - 256, G), (G - 40, G, 0, 128), (G - 64, G, G - 64, G), (2000, 2040, 3000, 3200)]


def _device_ld(X):
    from test_gpu_float32 import _device_copy

    def load(ctx):
        keep, ptr, ld = _device_copy(X, pad=8)
        assert ld > X.shape[0]
        ctx.set_matrix_device(ptr, X.shape[0], X.shape[1], ld, "i64", keepalive=keep)
        return keep
    return load


def _build(pkg, monkeypatch, load, gid, k, pval_reo, env, want_slice):
    """(blocks, tally, thresholds, k1_half_tiles_separated, k1_slot_sides) of comparison k built under env"""
    _env(monkeypatch, **env)
    with _open(pkg, load, gid, 2, pval_reo, SEED) as ctx:
        G = ctx.info()["G"]
        thr = ctx.get_thresholds()
        ctx.build_pairs(k)
        info = ctx.info()
        print(env, {n: info[n] for n in ("k1_slot_order", "k1_slot_sides", "k1_slot_slice", "planes_on_demand", "k1_half_tiles_separated", "has_ties")})
        assert (info["k1_slot_order"], info["has_ties"], info["k1_slot_slice"]) == (1, 0, want_slice), info
        assert info["planes_on_demand"] == 0, info   # (a slot build reads no gene-order planes; under REO_K1_SLOT_SLICE=0 the transform made them)
        out = ([ctx.get_codes(*b) for b in _blocks(G)], ctx.tally(np.ones(G, dtype=bool)), thr, info["k1_half_tiles_separated"], info["k1_slot_sides"])
    _env(monkeypatch)
    return out


# (genes, side 0, side 1, order, comparison, pval_reo, form, slot orders)
TABLE_CASES = {
    "2x(2+2)": (2, 2, 2, "contiguous", 0, 0.01, "int64", 1),
    "33x(5+96)": (33, 5, 96, "contiguous", 0, 0.3, "int64", 1),
    "257x(32+32)": (257, 32, 32, "contiguous", 0, 0.01, "int64", 1),
    "1000x(20+44)-k1": (1000, 20, 44, "contiguous", 1, 0.01, "int64", 1),          # side 0's blocks lie behind side 1's
    "2049x(20+44)-shuffled": (2049, 20, 44, "shuffled", 0, 0.01, "int64", 1),
    "1000x(20+44)-float64": (1000, 20, 44, "contiguous", 0, 0.01, "float64", 1),
    "1000x(20+44)-device-ld": (1000, 20, 44, "contiguous", 0, 0.01, "device_ld", 1),
    "1000x(256+256)": (1000, 256, 256, "contiguous", 0, 0.3, "int64", 2),            # 8 + 8 blocks: an order per side
    "257x(256+256)-k1": (257, 256, 256, "contiguous", 1, 0.3, "int64", 2),
    "4097x(32+32)": (4097, 32, 32, "contiguous", 0, 0.01, "int64", 1),               # the 15-plane loop
    "32769x(32+32)": (32769, 32, 32, "contiguous", 0, 0.01, "int64", 1),             # the 16-plane loop
}


@pytest.mark.parametrize("name", list(TABLE_CASES))
def test_table_equality(pkg, oracle, monkeypatch, name):
    G, n0, n1, order, k, pval, form, sides = TABLE_CASES[name]
    side = sc.layout_side(n0, n1, order, k, seed=SEED + 1)
    gid = sc.gid_of(side, k)
    X = sc.planted(side, G, 11)
    load = _device_ld(X) if form == "device_ld" else _host(X.astype(form))
    got, tally, thr, sep, got_sides = _build(pkg, monkeypatch, load, gid, k, pval, {}, 1)
    assert got_sides == sides == ss.sides_by_rule(n0, n1)
    Xf = np.asfortranarray(X.astype(np.float64))
    if G <= WHOLE:
        code = oracle.build_codes(Xf, gid, 2, k, thr[:, k].tolist(), SEED)
        assert np.array_equal(got[0], code), f"class table differs from the oracle's in {int((got[0] != code).sum())} codes"
        assert np.array_equal(tally, oracle.tally(code, np.ones(G, dtype=bool)))
    else:
        for b, g in zip(_blocks(G)[:2], got[:2]):
            assert np.array_equal(g, _expected_block_codes(oracle, Xf, gid, thr, SEED, *b, k=k)), ("block differs from the oracle's", b)
        assert tally.sum() == G * (G - 1)   # (every ordered pair has one class)
    other, other_tally, _, other_sep, other_sides = _build(pkg, monkeypatch, load, gid, k, pval, dict(slot_slice=0), 0)
    assert other_sides == sides and other_sep == sep, (sep, other_sep)
    for b, g, w in zip(_blocks(G), got, other):
        assert np.array_equal(g, w), f"block {b} differs from the build's under REO_K1_SLOT_SLICE=0 in {int((g != w).sum())} codes"
    assert np.array_equal(tally, other_tally)


# ---- b. the planes on demand

def _queries(pkg, ctx, G, S):
    """the four readers of the gene-order planes, in the order pair_counts, pair_support, sample_counts, masked build; after each:
    info()["planes_on_demand"]"""
    rng = np.random.default_rng(5)
    out, demand = [], []
    out.append(ctx.pair_counts(0, G, 0, G)); demand.append(ctx.info()["planes_on_demand"])
    genes = np.array([0, G // 2, G - 1], dtype=np.int32)
    rowptr = np.array([0, 7, 7 + 40, 7 + 40 + 3], dtype=np.int64)
    partner = np.concatenate([rng.choice(np.delete(np.arange(G), int(i)), size=n) for i, n in zip(genes, np.diff(rowptr))]).astype(np.int32)
    ps = ctx.pair_support((genes, rowptr, partner), outcomes=True)
    out.append((ps.n_gt, ps.n_eq, ps.outcome)); demand.append(ctx.info()["planes_on_demand"])
    cnt = ctx.sample_counts(genes, 0x1FF, np.ones(G, dtype=bool))
    out.append((cnt.n_sel, cnt.n_gt, cnt.n_eq)); demand.append(ctx.info()["planes_on_demand"])
    V = rng.random((G, S)) > 0.2
    ctx.set_valid_mask(V)
    ctx.build_pairs_masked(0)
    out.append((ctx.get_codes(0, G, 0, G),) + tuple(ctx.pair_counts_masked(0, 40, G - 50, G))); demand.append(ctx.info()["planes_on_demand"])
    ctx.set_valid_mask(None)
    return out, demand


def test_planes_on_demand_after_a_slot_build(pkg, oracle, monkeypatch):
    G, S = 257, 64
    side = sc.layout_side(32, 32, "contiguous", 0)
    gid = sc.gid_of(side, 0)
    X = sc.planted(side, G, 11)
    Xf = np.asfortranarray(X.astype(np.float64))
    _env(monkeypatch)
    with _open(pkg, _host(X), gid, 2, 0.01, SEED) as ctx:
        thr = ctx.get_thresholds()
        ctx.build_pairs(0)
        info = ctx.info()
        assert (info["k1_slot_order"], info["k1_slot_slice"], info["planes_on_demand"]) == (1, 1, 0), info
        got, demand = _queries(pkg, ctx, G, S)
        assert demand == [1, 1, 1, 1], demand
        ctx.build_pairs(1)
        info = ctx.info()
        assert (info["k1_slot_order"], info["planes_on_demand"]) == (1, 1), info
        assert np.array_equal(ctx.get_codes(0, G, 0, G), oracle.build_codes(Xf, gid, 2, 1, thr[:, 1].tolist(), SEED))
    egt, eeq = oracle.pair_counts(Xf, gid, 2, 0, G, 0, G)
    assert np.array_equal(got[0][0], egt) and np.array_equal(got[0][1], eeq)
    _env(monkeypatch, slots=0)
    with _open(pkg, _host(X), gid, 2, 0.01, SEED) as ctx:
        ctx.build_pairs(0)
        info = ctx.info()
        assert (info["k1_slot_order"], info["k1_slot_slice"], info["planes_on_demand"]) == (0, 0, 0), info
        want, demand = _queries(pkg, ctx, G, S)
        assert demand == [0, 0, 0, 0], demand
    _env(monkeypatch)
    for what, g, w in zip(("pair_counts", "pair_support", "sample_counts", "masked build"), got, want):
        assert len(g) == len(w) and all(np.array_equal(a, b) for a, b in zip(g, w)), what


def test_three_groups_make_their_planes_in_the_transform(pkg, oracle, monkeypatch):
    G, S = 257, 66
    gid = np.array([0] * 20 + [1] * 22 + [2] * 24, dtype=np.int32)
    X = sc.planted((gid != 0).astype(np.int32), G, 11)
    Xf = np.asfortranarray(X.astype(np.float64))
    _env(monkeypatch)
    with _open(pkg, _host(X), gid, 3, 0.01, SEED) as ctx:
        thr = ctx.get_thresholds()
        ctx.build_pairs(2)
        info = ctx.info()
        assert (info["k1_slot_order"], info["k1_slot_slice"], info["planes_on_demand"]) == (0, 0, 0), info
        gt, eq = ctx.pair_counts(0, G, 0, G)
        assert ctx.info()["planes_on_demand"] == 0
        assert np.array_equal(ctx.get_codes(0, G, 0, G), oracle.build_codes(Xf, gid, 3, 2, thr[:, 2].tolist(), SEED))
    egt, eeq = oracle.pair_counts(Xf, gid, 3, 0, G, 0, G)
    assert np.array_equal(gt, egt) and np.array_equal(eq, eeq)


# ---- c. ties on a slot-eligible shape

def test_tie_rich_data_slices_in_the_transform(pkg, oracle, monkeypatch):
    G, S = 1000, 64
    X = pkg.synth.t1_counts(G, S, SEED)
    gid = np.array([0] * 32 + [1] * 32, dtype=np.int32)
    Xf = np.asfortranarray(X.astype(np.float64))
    _env(monkeypatch)
    with _open(pkg, _host(X), gid, 2, 0.01, SEED) as ctx:
        thr = ctx.get_thresholds()
        ctx.build_pairs(0)
        info = ctx.info()
        assert (info["has_ties"], info["k1_slot_order"], info["k1_slot_slice"], info["planes_on_demand"]) == (1, 0, 0, 0), info
        assert np.array_equal(ctx.get_codes(0, G, 0, G), oracle.build_codes(Xf, gid, 2, 0, thr[:, 0].tolist(), SEED))
        b = (G - 40, G, 0, 300)
        gt, eq = ctx.pair_counts(*b)
        assert ctx.info()["planes_on_demand"] == 0
    egt, eeq = oracle.pair_counts(Xf, gid, 2, *b)
    assert np.array_equal(gt, egt) and np.array_equal(eq, eeq) and eeq.any()


# ---- d. one context across matrices; the pipelined upload

def test_one_context_tie_free_tie_rich_tie_free(pkg, oracle, monkeypatch):
    G, S = 1000, 64
    side = sc.layout_side(32, 32, "contiguous", 0)
    gid = sc.gid_of(side, 0)
    Xs = sc.planted(side, G, 11)
    Xt = pkg.synth.t1_counts(G, S, SEED)
    b = (G - 33, G, 0, 200)
    _env(monkeypatch)
    with pkg.Context(device=0, seed=SEED) as ctx:
        for X, ties in ((Xs, 0), (Xt, 1), (Xs, 0)):
            Xf = np.asfortranarray(X.astype(np.float64))
            ctx.set_matrix(np.asfortranarray(X))
            ctx.set_groups(gid, 2)
            ctx.compute_thresholds(0.01)
            thr = ctx.get_thresholds()
            assert ctx.info()["k1_slot_slice"] == 0 and ctx.info()["planes_on_demand"] == 0   # (nothing built, nothing transformed yet)
            ctx.build_pairs(0)
            info = ctx.info()
            assert (info["has_ties"], info["k1_slot_order"], info["k1_slot_slice"], info["planes_on_demand"]) == (ties, 1 - ties, 1 - ties, 0), info
            assert np.array_equal(ctx.get_codes(0, G, 0, G), oracle.build_codes(Xf, gid, 2, 0, thr[:, 0].tolist(), SEED)), ties
            gt, eq = ctx.pair_counts(*b)
            assert ctx.info()["planes_on_demand"] == 1 - ties
            egt, eeq = oracle.pair_counts(Xf, gid, 2, *b)
            assert np.array_equal(gt, egt) and np.array_equal(eq, eeq), ties


def test_pipelined_upload_keeps_the_identity_order(pkg, oracle, monkeypatch):
    """T0 ranks (tie-free, small keys: every sample takes the histogram ranking, so the upload stays pipelined), 1 000 x (64 + 64)"""
    G = 1000
    gid = np.array([0] * 64 + [1] * 64, dtype=np.int32)
    X = pkg.synth.t0_ranks(G, 128, SEED)
    Xf = np.asfortranarray(X.astype(np.float64))
    b = (0, 40, G - 300, G)
    _env(monkeypatch)
    with pkg.Context(device=0, seed=SEED) as ctx:
        ctx.set_groups(gid, 2)                 # groups and thresholds first: the sides are ranked, sliced and paired as the matrix arrives
        ctx.compute_thresholds(0.01)
        ctx.set_matrix(np.asfortranarray(X))
        thr = ctx.get_thresholds()
        ctx.build_pairs(0)
        info = ctx.info()
        assert (info["has_ties"], info["k1_slot_order"], info["k1_slot_slice"], info["planes_on_demand"]) == (0, 0, 0, 0), info
        assert np.array_equal(ctx.get_codes(0, G, 0, G), oracle.build_codes(Xf, gid, 2, 0, thr[:, 0].tolist(), SEED))
        gt, eq = ctx.pair_counts(*b)
        assert ctx.info()["planes_on_demand"] == 0
    egt, eeq = oracle.pair_counts(Xf, gid, 2, *b)
    assert np.array_equal(gt, egt) and np.array_equal(eq, eeq)
