"""The word forms of the column un-permute behind a slot build (kernels.hip: k1_unslot_words<8>, <4>; index rules and host model:
csrc/k1_slots.h, tests/test_unslot_cpu.py) against the bit form, k1_unslot_columns, which REO_K1_UNSLOT=0 still runs.

Levelled data from tests/slot_cases.py (planted: separated items with both constants exist from 257 genes on).  Every case asserts
info()["k1_slot_order"] == 1, info()["has_ties"] == 0 and the expected info()["k1_unslot_form"] (8 / 4: the word forms, 1: the bit form).
REO_K1_UNSLOT=8 / 4 forces that form at any gene count whose table T fits a workgroup's LDS, so that the narrow form, which the rule
takes up to 25 600 genes and from 38 913 on, and the wide form, which it takes in between, both run at small sizes."""
import functools

import numpy as np
import pytest

import slot_cases as sc
from test_gpu_slot_matrix import _host, _open, _where

pytestmark = pytest.mark.gpu

ENV = ("REO_K1_SLOTS", "REO_K1_WORKERS", "REO_K1_QUEUE", "REO_ROWMAJOR", "REO_K1_UNSLOT")
SEED = 3


def _env(monkeypatch, unslot=None):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    if unslot is not None:
        monkeypatch.setenv("REO_K1_UNSLOT", str(unslot))


@functools.lru_cache(maxsize=2)
def _case(G, n0, n1):
    """planted levels, n0 + n1 samples, comparison 0; the arrays are shared between tests and never written"""
    side = sc.layout_side(n0, n1, "contiguous", 0)
    X = sc.planted(side, G, sc.PLANTED_SEED)
    X.setflags(write=False)
    return X, side, sc.gid_of(side, 0)


def _build(pkg, monkeypatch, X, gid, unslot, form, read):
    """a slot build under REO_K1_UNSLOT = unslot (None: unset) that must report `form`; read(ctx) -> what the case compares"""
    _env(monkeypatch, unslot)
    with _open(pkg, _host(X), gid, 2, 0.01, SEED) as ctx:
        thr = ctx.get_thresholds()
        ctx.build_pairs(0)
        info = ctx.info()
        assert info["k1_slot_order"] == 1 and info["has_ties"] == 0, info
        assert info["k1_unslot_form"] == form, info
        out = read(ctx)
    _env(monkeypatch)
    return out, thr


def _ref_masks(pkg, G):
    return [np.ones(G, dtype=bool), pkg.synth.ref_mask(G, G // 7, SEED)]


_BIT = {}


def _bit_form(pkg, monkeypatch, G, n0, n1):
    """whole table and both tallies under REO_K1_UNSLOT=0, once per size"""
    if G not in _BIT:
        X, side, gid = _case(G, n0, n1)
        masks = _ref_masks(pkg, G)
        (codes, tallies), thr = _build(pkg, monkeypatch, X, gid, 0, 1, lambda ctx: (ctx.get_codes(0, G, 0, G), [ctx.tally(m) for m in masks]))
        codes.setflags(write=False)
        _BIT.clear()   # (one size at a time: the tests of a size run together)
        _BIT[G] = (codes, tallies, thr)
    return _BIT[G]


# ---- a. both forms forced at small sizes: whole table and tallies against the bit form and the oracle

@pytest.mark.parametrize("form", [8, 4])
@pytest.mark.parametrize("G", [2, 33, 257, 1000, 1001])
def test_forced_forms_at_small_sizes(pkg, oracle, monkeypatch, form, G):
    """4 + 4 samples.  The last workgroup holds 2 of 8 rows (G = 2), 1 of 8 and 1 of 4 (33, 257), a full group (1 000) and one row past
    a full group (1 001); every G but 2 ends in a word with padded columns, which come out zero (the oracle's table has none)."""
    X, side, gid = _case(G, 4, 4)
    masks = _ref_masks(pkg, G)
    want, want_tallies, _ = _bit_form(pkg, monkeypatch, G, 4, 4)
    (got, tallies), thr = _build(pkg, monkeypatch, X, gid, form, form, lambda ctx: (ctx.get_codes(0, G, 0, G), [ctx.tally(m) for m in masks]))
    assert np.array_equal(got, want), "class table differs from the bit form's: " + _where(got, want, X, side)
    for t, w in zip(tallies, want_tallies):
        assert np.array_equal(t, w), "tallies differ from the bit form's"
    if G <= 1000:
        code = oracle.build_codes(np.asfortranarray(X.astype(np.float64)), gid, 2, 0, thr[:, 0].tolist(), SEED)
        assert np.array_equal(got, code), "class table differs from the oracle's: " + _where(got, code, X, side)
        for m, t in zip(masks, tallies):
            assert np.array_equal(t, oracle.tally(code, m)), "tallies differ from the oracle's"


# ---- b. the word loops walked twice, the second trip partial

@pytest.mark.parametrize("form", [8, 4])
def test_two_trips_with_a_partial_second(pkg, monkeypatch, form):
    """33 000 genes: 1 056 words per bit row, unslot_threads(1 056) = 576 threads, so a thread walks the in and the out loop twice and
    threads 480 .. 575 only once (both forms fit: T = 139 392 and 71 808 bytes).  Whole table against the bit form's, 3 000 rows at a
    time from two contexts that are open together."""
    G = 33000
    X, side, gid = _case(G, 4, 4)
    _env(monkeypatch, form)
    with _open(pkg, _host(X), gid, 2, 0.01, SEED) as ctx:
        ctx.build_pairs(0)
        _env(monkeypatch, 0)
        with _open(pkg, _host(X), gid, 2, 0.01, SEED) as bit:
            bit.build_pairs(0)
            _env(monkeypatch)
            for c, f in ((ctx, form), (bit, 1)):
                info = c.info()
                assert (info["k1_slot_order"], info["has_ties"], info["k1_unslot_form"], info["Gp"]) == (1, 0, f, 33792), info
            for r0 in range(0, G, 3000):
                r1 = min(G, r0 + 3000)
                got, want = ctx.get_codes(r0, r1, 0, G), bit.get_codes(r0, r1, 0, G)
                assert np.array_equal(got, want), f"rows {r0}..{r1}: {int((got != want).sum())} codes differ from the bit form's"


# ---- c. the rule's own limits, unforced

@pytest.mark.parametrize("G,Gp,form", [(25600, 25600, 4), (25601, 26624, 8), (38912, 38912, 8), (38913, 39936, 4), (65535, 65536, 4)])
def test_forms_at_the_limits_of_the_rule(pkg, monkeypatch, G, Gp, form):
    """25 600 genes: the last size at which three narrow workgroups share a CU's LDS (3 x 54 400 bytes), no tail; 25 601 (Gp 26 624): the
    first of the wide form, last workgroup 1 row of 8; 38 912: the last of the wide form (T = 160 512 bytes of the 163 840), no tail; 38 913 (Gp 39 936): the first of the
    narrow form, last workgroup 1 row of 4; 65 535 (Gp 65 536): the largest slot build, T = 139 264 bytes, last workgroup 3 rows of 4.
    4 + 4 samples.  Sampled blocks -- first and last rows and columns, the diagonal, the padded tail, the last workgroup's rows over the
    first, a middle and the last 256 columns -- and both tallies against the bit form's."""
    X, side, gid = _case(G, 4, 4)
    tail = G % form or form
    blocks = [(0, 48, 0, 256), (0, 32, G - 256, G), (G - 40, G, 0, 128), (G - 64, G, G - 64, G), (16000, 16040, 16000, 16200), (20000, 20032, 300, 428),
              (5000, 5032, G - 3000, G - 2872), (G - tail, G, 0, 256), (G - tail, G, G // 2, G // 2 + 256), (G - tail, G, G - 256, G)]
    masks = _ref_masks(pkg, G)

    def read(ctx):
        assert ctx.info()["Gp"] == Gp
        return [ctx.get_codes(*b) for b in blocks], [ctx.tally(m) for m in masks]

    (got, tallies), _ = _build(pkg, monkeypatch, X, gid, None, form, read)
    (want, want_tallies), _ = _build(pkg, monkeypatch, X, gid, 0, 1, read)
    for b, g, w in zip(blocks, got, want):
        assert np.array_equal(g, w), b
    for t, w in zip(tallies, want_tallies):
        assert np.array_equal(t, w), "tallies differ from the bit form's"
    assert tallies[0].sum() == G * (G - 1)   # (every ordered pair has one class)


# ---- d. end to end

def test_identify_degs_equal_under_both(pkg, monkeypatch):
    """identify_degs at 3 000 x (6 + 6), 16 forced passes: result, trace and iterations byte-equal with the word form (unset) and the bit form"""
    G = 3000
    X, side, gid = _case(G, 6, 6)
    ref0 = pkg.synth.ref_mask(G, 300, SEED)
    out = {}
    for unslot, form in ((None, 4), (0, 1)):
        out[form], _ = _build(pkg, monkeypatch, X, gid, unslot, form, lambda ctx: ctx.identify_degs(ref0, 1.0, 0.05, 16, 0))
    (rw, iw, tw), (r1, i1, t1) = out[4], out[1]
    assert iw == i1
    assert np.asarray(tw).tobytes() == np.asarray(t1).tobytes()
    assert np.asarray(rw).tobytes() == np.asarray(r1).tobytes()
