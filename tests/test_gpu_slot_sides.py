"""Per-side slot order of the pair kernel (csrc/k1_slots.h; kernels.hip, launch_k1): each side of a slot build has its own order of the
genes, key_z = pmin_z + pmax_z, its own g2s / s2g, and the pair form of the word un-permute (k1_unslot_pair) puts each side's plane pair
back with that side's map.  The table that leaves launch_k1 is the identity order's bit for bit.

Matrices and the rule in numpy: tests/slot_sides_cases.py (tests/test_slot_sides_cpu.py asserts that the per-side count of separated items
is strictly above the common rule's on every levelled case, so a build that ran the common order cannot pass here).  Every case asserts
info()["k1_slot_sides"] == 2, ["k1_slot_order"] == 1, ["has_ties"] == 0, ["k1_half_tiles_separated"] == 2 x the per-side model's count, and
that the table equals the oracle's, the table of a context under REO_K1_SLOTS=0 and the table of a context under REO_K1_SLOT_SIDES=1 --
the whole table up to 2 049 genes; above, sampled blocks (first and last rows and columns, the diagonal, the padded tail) and the tallies
of every gene, which read every word of the table.  Most cases have few samples and force the form with REO_K1_SLOT_SIDES=2; the rule
itself (16 sample blocks of both sides together) runs unforced at 1 024 genes."""
import numpy as np
import pytest

import slot_cases as sc
import slot_sides_cases as ss
from test_gpu_parity import _expected_block_codes
from test_gpu_slot_matrix import _host, _open

pytestmark = pytest.mark.gpu

ENV = ("REO_K1_SLOTS", "REO_K1_WORKERS", "REO_K1_QUEUE", "REO_ROWMAJOR", "REO_K1_UNSLOT", "REO_K1_SLOT_SIDES")
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
    return [(0, 16, 0, 128), (G - 16, G, G - 128, G), (0, 48, G - 256, G), (G - 40, G, 0, 128), (G - 64, G, G - 64, G), (16000, 16040, 16000, 16200),
            (20000, 20032, 300, 428), (5000, 5032, G - 3000, G - 2872)]


def _read(pkg, G):
    mask = np.ones(G, dtype=bool)
    return lambda ctx: ([ctx.get_codes(*b) for b in _blocks(G)], ctx.tally(mask))


def _build(pkg, monkeypatch, X, gid, k, env, want, read, pval_reo=0.01):
    """a build of comparison k under `env` whose info must report want = (k1_slot_order, k1_slot_sides, k1_half_tiles_separated or None)"""
    _env(monkeypatch, **env)
    with _open(pkg, _host(X), gid, 2, pval_reo, SEED) as ctx:
        thr = ctx.get_thresholds()
        ctx.build_pairs(k)
        info = ctx.info()
        print(env, {n: info[n] for n in ("k1_slot_order", "k1_slot_sides", "k1_half_tiles_separated", "k1_unslot_form", "has_ties")})
        assert info["has_ties"] == 0, info
        assert (info["k1_slot_order"], info["k1_slot_sides"]) == want[:2], info
        if want[2] is not None:
            assert info["k1_half_tiles_separated"] == want[2], info
        out = read(ctx, info)
    _env(monkeypatch)
    return out, thr


def _check(pkg, oracle, monkeypatch, X, side, gid, k, env, unslot_form=None, pval_reo=0.01):
    """One per-side case: everything the module's docstring lists.  env: what the per-side build runs under."""
    G = X.shape[0]
    rd = _read(pkg, G)
    per_side, common = ss.model_count(X, side), sc.model_count(X, side)
    print("separated items: per-side model", per_side, "common model", common)

    def read(ctx, info):
        if unslot_form is not None:
            assert info["k1_unslot_form"] == unslot_form, info
        return rd(ctx)

    (got, tally), thr = _build(pkg, monkeypatch, X, gid, k, env, (1, 2, 2 * per_side), read, pval_reo)
    partner = {n: v for n, v in env.items() if n != "slot_sides"}
    (ident, ident_tally), _ = _build(pkg, monkeypatch, X, gid, k, dict(partner, slots=0), (0, 0, 0), lambda ctx, info: rd(ctx), pval_reo)
    (comm, comm_tally), _ = _build(pkg, monkeypatch, X, gid, k, dict(partner, slot_sides=1), (1, 1, 2 * common), lambda ctx, info: rd(ctx), pval_reo)
    Xf = np.asfortranarray(X.astype(np.float64))
    if G <= WHOLE:
        code = oracle.build_codes(Xf, gid, 2, k, thr[:, k].tolist(), SEED)
        assert np.array_equal(got[0], code), f"class table differs from the oracle's in {int((got[0] != code).sum())} codes"
        assert np.array_equal(tally, oracle.tally(code, np.ones(G, dtype=bool))), "tallies differ from the oracle's"
    else:
        for b, g in zip(_blocks(G)[:2], got[:2]):
            assert np.array_equal(g, _expected_block_codes(oracle, Xf, gid, thr, SEED, *b, k=k)), ("block differs from the oracle's", b)
        assert tally.sum() == G * (G - 1)   # (every ordered pair has one class)
    for what, other, other_tally in (("identity order", ident, ident_tally), ("common order", comm, comm_tally)):
        for b, g, w in zip(_blocks(G), got, other):
            assert np.array_equal(g, w), f"block {b} differs from the {what}'s in {int((g != w).sum())} codes"
        assert np.array_equal(tally, other_tally), f"tallies differ from the {what}'s"


# ---- a. the named cases, forced

@pytest.mark.parametrize("name", list(ss.CASES))
def test_forced_per_side_order(pkg, oracle, monkeypatch, name):
    """257 genes (two chunks); 1 000 x 64 (12 planes, half-height items); 2 049 x 66 (15 planes, padded sample slots, a one-gene last tile);
    65 535 x 8 (16 planes, 64-bit rank keys, narrow un-permute); 30 000 x 8 (wide un-permute); sides of 2 + 62 and 33 + 32 samples; shuffled
    labels; comparison 1 (side 0 is the group that comes second: its blocks lie behind the other side's, and the gather must pick the maps
    by block range); every key of side 0 equal (the gene index decides that side's order) beside a levelled side 1."""
    X, side, gid, k = ss.case(name)
    form = {"65535x8": 4, "30000x8": 8}.get(name)
    _check(pkg, oracle, monkeypatch, X, side, gid, k, dict(slot_sides=2), unslot_form=form)


# ---- b. the switches beside it

@pytest.mark.parametrize("env,form", [(dict(queue=0), 4), (dict(unslot=4), 4), (dict(unslot=8), 8), (dict(workers=13), 4)])
def test_switches(pkg, oracle, monkeypatch, env, form):
    """2 049 x 66 with one workgroup per item (REO_K1_QUEUE=0), both word forms of the un-permute forced (T fits at 3 072 slots), few workers"""
    X, side, gid, k = ss.case("2049x66")
    _check(pkg, oracle, monkeypatch, X, side, gid, k, dict(env, slot_sides=2), unslot_form=form)


def test_bit_form_keeps_the_common_order(pkg, oracle, monkeypatch):
    """REO_K1_UNSLOT=0: the bit form has one map, so the build reports k1_slot_sides == 1 even where per-side order is asked for"""
    X, side, gid, k = ss.case("2049x66")
    G = X.shape[0]

    def read(ctx, info):
        assert info["k1_unslot_form"] == 1, info
        return ctx.get_codes(0, G, 0, G)

    got, thr = _build(pkg, monkeypatch, X, gid, k, dict(slot_sides=2, unslot=0), (1, 1, 2 * sc.model_count(X, side)), read)
    assert np.array_equal(got, oracle.build_codes(np.asfortranarray(X.astype(np.float64)), gid, 2, k, thr[:, k].tolist(), SEED))


# ---- c. the rule, unforced

@pytest.mark.parametrize("b0,b1,sides", [(7, 8, 1), (8, 8, 2), (15, 1, 2)])
def test_rule_by_sample_blocks(pkg, oracle, monkeypatch, b0, b1, sides):
    """1 024 genes, b0 + b1 sample blocks of 32 (the last sample of side 0 left out: a padded slot), nothing forced: per-side order from 16
    blocks of both sides together on."""
    n0, n1 = 32 * b0 - 1, 32 * b1
    assert ss.sides_by_rule(n0, n1) == sides
    side = sc.layout_side(n0, n1, "contiguous", 0)
    X = ss.planted(side, 1024, ss.SEED)
    gid = sc.gid_of(side, 0)
    if sides == 2:
        _check(pkg, oracle, monkeypatch, X, side, gid, 0, {}, pval_reo=0.3)
        return
    got, thr = _build(pkg, monkeypatch, X, gid, 0, {}, (1, 1, 2 * sc.model_count(X, side)), lambda ctx, info: ctx.get_codes(0, 1024, 0, 1024), pval_reo=0.3)
    assert np.array_equal(got, oracle.build_codes(np.asfortranarray(X.astype(np.float64)), gid, 2, 0, thr[:, 0].tolist(), SEED))


# ---- d. one context, three kinds of build in turn

def test_one_context_per_side_common_identity(pkg, oracle, monkeypatch):
    """The same context builds 1 024 x 512 (8 + 8 blocks: per-side order), 1 024 x 8 (common order), count data with ties (identity order)
    and the first matrix again: the maps of one build leave nothing behind for the next, and info() follows."""
    _env(monkeypatch)
    G = 1024
    big_side, small_side = sc.layout_side(256, 256, "contiguous", 0), sc.layout_side(4, 4, "contiguous", 0)
    mats = [(ss.planted(big_side, G, ss.SEED), big_side, 2), (ss.planted(small_side, G, ss.SEED + 1), small_side, 1),
            (pkg.synth.t1_counts(G, 8, SEED), small_side, 0)]
    mats.append(mats[0])
    with pkg.Context(device=0, seed=SEED) as ctx:
        for X, side, sides in mats:
            gid = sc.gid_of(side, 0)
            ctx.set_matrix(np.asfortranarray(X))
            ctx.set_groups(gid, 2)
            ctx.compute_thresholds(0.3)
            assert ctx.info()["k1_slot_sides"] == 0 and ctx.info()["k1_half_tiles_separated"] == 0   # (nothing built yet)
            thr = ctx.get_thresholds()
            ctx.build_pairs(0)
            info = ctx.info()
            assert (info["k1_slot_order"], info["k1_slot_sides"], info["has_ties"]) == (int(sides > 0), sides, int(sides == 0)), info
            if sides:
                assert info["k1_half_tiles_separated"] == 2 * (ss.model_count if sides == 2 else sc.model_count)(X, side)
            code = oracle.build_codes(np.asfortranarray(X.astype(np.float64)), gid, 2, 0, thr[:, 0].tolist(), SEED)
            assert np.array_equal(ctx.get_codes(0, G, 0, G), code), f"k1_slot_sides {sides}: class table differs from the oracle's"


# ---- e. the planes stay in gene order

def test_pair_counts_after_a_per_side_build(pkg, oracle, monkeypatch):
    """pair_counts reads c->pos and c->lo, which the slot front only gathers FROM: two blocks after a per-side build are the oracle's"""
    X, side, gid, k = ss.case("2049x66")
    G = X.shape[0]
    Xf = np.asfortranarray(X.astype(np.float64))

    def read(ctx, info):
        return [ctx.pair_counts(*b) for b in ((0, 40, G - 300, G), (G - 33, G, 0, 64))]

    got, _ = _build(pkg, monkeypatch, X, gid, k, dict(slot_sides=2), (1, 2, None), read)
    for (gt, eq), b in zip(got, ((0, 40, G - 300, G), (G - 33, G, 0, 64))):
        egt, eeq = oracle.pair_counts(Xf, gid, 2, *b)
        assert np.array_equal(gt, egt) and np.array_equal(eq, eeq), b
