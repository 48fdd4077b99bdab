"""What the cases of tests/test_gpu_slot_matrix.py are there for, asserted on the CPU from the rule in numpy (tests/slot_cases.py): a case
that stops separating anything, or that loses one of the two constants on a side, would leave the GPU test green and empty.  Also pins
the convention of comparison 1 on two groups -- group 1 is the control side, thresholds thr[:, 1] -- in both oracles."""
import numpy as np
import pytest

import slot_cases as sc


@pytest.mark.parametrize("k", [0, 1])
@pytest.mark.parametrize("lay", sc.LAYOUTS, ids=sc.layout_id)
def test_planted_layouts_have_both_constants_on_both_sides(lay, k):
    X, side, gid = sc.planted_case(lay, k)
    G = X.shape[0]
    assert G == 1013 and X.shape[1] == lay[0] + lay[1] and (side == 0).sum() == lay[0]
    assert gid[0] == 0 and (gid == k).sum() == lay[0]                 # ids in order of first appearance; group k is side 0
    assert 0 <= X.min() and X.max() < 2 ** 24                         # exact as Float32 ...
    assert all(np.diff(np.sort(X[:, s])).min() >= 1 for s in range(X.shape[1]))   # ... and tie-free under the 0.1 band
    is_live, sep = sc.masks(X, side)
    live, counts = sc.model(X, side)
    assert live == 160 and counts == {0: [15, 21], 1: [7, 23]}, (live, counts)
    NT, NQ = is_live.shape
    anysep = sep[0][0] | sep[0][1] | sep[1][0] | sep[1][1]
    assert anysep[:, NQ - 1].any(), "a separated item in the last chunk (padding columns)"
    assert not anysep[NT - 1, :].any()                                # a tile inside its chunk never qualifies: none with rows beyond G


def test_planted_at_a_multiple_of_the_chunk():
    for lay in sc.LAYOUTS:
        X, side, _ = sc.planted_case(lay, 0, G=1024)
        assert sc.model(X, side) == (160, {0: [16, 24], 1: [16, 24]}), lay


def test_layouts_are_what_their_names_say():
    by = {sc.layout_id(lay): lay for lay in sc.LAYOUTS}
    assert len(by) == 8 and sc.FORM_LAYOUT in sc.LAYOUTS
    for k in (0, 1):
        side = sc.layout_side(20, 44, "shuffled", k, seed=12)
        assert side[0] == k and np.count_nonzero(np.diff(side)) > 10              # interleaved
        side = sc.layout_side(40, 24, "split", k)
        gid = sc.gid_of(side, k)
        first, n_first = (0, 40) if k == 0 else (1, 24)                           # the side of group 0 and its size
        assert gid[0] == 0 and (gid[1:1 + 64 - n_first] == 1).all() and (gid[1 + 64 - n_first:] == 0).all() and side[0] == first
        side = sc.layout_side(2, 62, "contiguous", k)
        assert np.count_nonzero(np.diff(side)) == 1 and side[0] == k
    assert sc.layout_side(2, 62, "contiguous", 1)[-2:].tolist() == [0, 0]           # comparison 1: the two control samples lie behind 62 others


def test_same_order_keys_and_counts():
    G = 1000
    X = sc.same_order(G, 12, 5)
    side = np.array([0] * 5 + [1] * 7)
    key, ext = sc.extremes(X, side)
    assert sorted(key.tolist()) == [4 * p for p in range(G)]                      # all keys different
    assert all(np.array_equal(mn, mx) for mn, mx in ext)                          # min == max on both sides
    assert sc.model(X, side) == (160, {0: [0, 48], 1: [0, 48]})
    want = {2: 0, 31: 0, 33: 0, 256: 0, 257: 16}                                  # 257: the one-gene last tile's chunk lies above the tiles of the first
    for g in sc.TINY_G:
        X = sc.same_order(g, 6, 5)
        assert sc.model_count(X, np.array([0] * 3 + [1] * 3)) == want[g], g
        assert len(set(sc.extremes(X, np.array([0] * 3 + [1] * 3))[0].tolist())) == g


def test_mirrored_has_one_key_and_separates_nothing():
    G = 1000
    X, side = sc.mirrored(G, 5, 7, 5)
    key, _ = sc.extremes(X, side)
    assert set(key.tolist()) == {2 * (G - 1)}
    assert sc.model(X, side) == (160, {0: [0, 0], 1: [0, 0]})
    assert all(sorted(X[:, s].tolist()) == list(range(G)) for s in range(X.shape[1]))


def test_sweep_separates_in_most_cases_and_spans_every_choice():
    cases = sc.sweep()
    assert len(cases) == sc.SWEEP_CASES == 24
    with_sep = sum(cs["separated"] > 0 for cs in cases)
    print("cases with separated items", with_sep, [cs["separated"] for cs in cases])
    assert with_sep >= sc.SWEEP_MIN_SEPARATED == 16
    assert sum(np.count_nonzero(np.diff(cs["side"])) > 1 for cs in cases) == 12   # shuffled labels: half of the cases
    for name, n in (("k", 2), ("pval_reo", 3), ("dtype", 4), ("workers", 4), ("queue", 2)):
        assert len({cs[name] for cs in cases}) == n, name
    for cs in cases:
        assert 257 <= cs["G"] <= 1499 and 2 <= cs["n0"] <= 69 and 2 <= cs["n1"] <= 69 and 2 <= cs["levels"] <= 8
        assert cs["X"].max() < 2 ** 24 and sc.gid_of(cs["side"], cs["k"])[0] == 0
    again = sc.random_levels(np.random.default_rng(sc.SWEEP_SEED), shuffled=False)
    assert np.array_equal(again["X"], cases[0]["X"])                             # one fixed seed: the same cases every time


def test_thresholds_leave_no_count_between_the_classes_unreached(oracle):
    """emit_constant's third branch (neither n >= hi_thr nor n <= n_side - hi_thr) needs a constant count, 0 or n_side, that is neither:
    hi_thr > n_side or hi_thr <= 0.  For every side size and pval_reo of these tests the threshold lies above n / 2 and at most at n, so
    0 <= n - thr < thr <= n: a separated item always has a class, and no case can pretend otherwise."""
    for p in (0.01, 0.05, 0.3):
        for n in range(2, 140):
            t = oracle.threshold(n, p)
            assert n / 2 < t <= n, (n, p, t)


@pytest.mark.parametrize("k", [0, 1])
def test_numpy_and_c_oracle_agree_on_comparison_k(oracle, rn, k):
    """planted, 300 genes in 4 classes of 75, sides of 3 and 5 samples: reo_numpy.build_codes (written from the reference's text) and the C
    oracle give the same table for k = 0 and k = 1 -- group k's counts against thr[0] and its size, the rest's against thr[1]."""
    G = 300
    side = sc.layout_side(3, 5, "contiguous", k)
    gid = sc.gid_of(side, k)
    X = sc.planted(side, G, 7)
    sizes = np.bincount(gid, minlength=2)
    assert sizes[k] == 3 and sizes[1 - k] == 5
    thr = [rn.threshold(int(sizes[k]), 0.01), rn.threshold(8 - int(sizes[k]), 0.01)]
    assert thr == [oracle.threshold(3, 0.01), oracle.threshold(5, 0.01)]
    a = rn.build_codes(X.astype(np.float64), gid, 2, k, thr, 3)
    b = oracle.build_codes(X.astype(np.float64), gid, 2, k, thr, 3)
    assert np.array_equal(a, b)
    assert len(set(np.unique(a).tolist()) - {255}) >= 4                           # not one class everywhere
    if k == 1:   # the other comparison of the same labels is another table: the sides are not interchangeable here
        thr0 = [oracle.threshold(5, 0.01), oracle.threshold(3, 0.01)]
        assert not np.array_equal(b, oracle.build_codes(X.astype(np.float64), gid, 2, 0, thr0, 3))
