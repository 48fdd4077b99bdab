"""The thin reference of tests/big_plane_cases.py held to the whole-table oracle at a few hundred genes, with the recipes that
tests/test_gpu_big_planes.py runs at 131 584; and every comparison of that file shown to fail on one planted error.  No GPU."""
import numpy as np
import pytest

import big_plane_cases as bp
from test_gpu_parity import P_ATOL, STAT_RTOL, _check_result

SEED = 0x5EED0B18


def _problem(oracle, name, G, ngroups=2, S=bp.S):
    gid = bp.labels(S, ngroups)
    fn = bp.MATRICES[name][0]
    X = fn(G, SEED, S, gid) if name != "band" else fn(G, SEED, S)
    Xf = np.asfortranarray(X.astype(np.float64))
    return X, Xf, gid, bp.thresholds(oracle, gid, ngroups)


@pytest.fixture(scope="module")
def counts600(oracle):
    """counts at 600 genes: the whole table, the four column strips, the reference set"""
    G = 600
    X, Xf, gid, thr = _problem(oracle, "counts", G)
    code = oracle.build_codes(Xf, gid, 2, 0, thr[:, 0], SEED)
    strips = bp.column_strips(oracle, Xf, gid, thr, SEED, G)
    for c in (code, *strips.values()):
        c.setflags(write=False)
    return G, Xf, gid, thr, code, strips, bp.ref_set(G)


def test_coins_equal_the_oracles_tie_wins(oracle, rn):
    rng = np.random.default_rng(1)
    n = 4000
    i = rng.integers(0, 262143, size=n)
    j = rng.integers(0, 262143, size=n)
    i[:50], j[:50] = 0, np.arange(50)                    # small keys, and the largest
    i[50:60], j[50:60] = 262141, 262142
    g = rng.integers(0, 3, size=n)
    n_eq = rng.integers(0, 65, size=n)
    n_eq[:8] = [0, 1, 63, 64, 64, 0, 32, 33]
    for seed in (0, 77, 0x5EED0B18, (1 << 64) - 1):
        got = bp.coins(seed, i, j, g, n_eq)
        assert got.dtype == np.int64
        exp = np.array([oracle.tie_wins(seed, int(a), int(b), int(c), int(e)) for a, b, c, e in zip(i, j, g, n_eq)])
        assert np.array_equal(got, exp), seed
        assert all(int(got[q]) == rn.tie_wins(seed, int(i[q]), int(j[q]), int(g[q]), int(n_eq[q])) for q in range(0, n, 16))
    assert (bp.coins(5, i, j, g, np.zeros(n, dtype=int)) == 0).all() and (bp.coins(5, i, j, g, np.full(n, 64)) > 0).all()
    with pytest.raises(AssertionError):
        bp.coins(5, i, j, g, np.full(n, 65))                # (more than one word of the stream: not restated)
    # a scalar group and two-dimensional keys, as expected_codes calls it
    ii, jj = np.arange(40)[:, None], np.arange(100, 140)[None, :]
    e2 = rng.integers(0, 9, size=(40, 40))
    got = bp.coins(9, *np.broadcast_arrays(ii, jj), 1, e2)
    assert all(int(got[a, b]) == oracle.tie_wins(9, a, 100 + b, 1, int(e2[a, b])) for a in range(40) for b in range(40))


@pytest.mark.parametrize("name,G,ngroups,S", [("free", 300, 2, 16), ("counts", 700, 2, 16), ("band", 500, 2, 16),
                                              ("free", 450, 3, 9), ("counts", 450, 3, 9), ("band", 333, 3, 9)])
def test_expected_codes_equal_the_whole_table(oracle, name, G, ngroups, S):
    X, Xf, gid, thr = _problem(oracle, name, G, ngroups, S)
    for k in range(ngroups):
        code = oracle.build_codes(Xf, gid, ngroups, k, thr[:, k], SEED)
        assert np.array_equal(bp.expected_codes(oracle, Xf, gid, thr, SEED, 0, G, 0, G, ngroups, k), code), k
        # strips as the GPU file cuts them: G x 32 and 32 x G, each on its own
        for a in (0, G // 3 - 16, G - 32):
            assert np.array_equal(bp.expected_codes(oracle, Xf, gid, thr, SEED, 0, G, a, a + 32, ngroups, k), code[:, a:a + 32])
            assert np.array_equal(bp.expected_codes(oracle, Xf, gid, thr, SEED, a, a + 32, 0, G, ngroups, k), code[a:a + 32, :])
        assert np.array_equal(bp.mirror(code[:, 7:39]), code[7:39, :])


def test_strip_tallies_equal_the_oracles_tally(oracle, counts600):
    G, Xf, gid, thr, code, strips, ref0 = counts600
    for j0, c in strips.items():
        m = np.zeros(G, dtype=bool)
        m[j0:j0 + bp.STRIP] = True
        assert np.array_equal(bp.strip_tally(c), oracle.tally(code, m)), j0
    assert list(strips) == bp.ref_runs(G) and ref0.sum() == 4 * bp.STRIP
    assert np.array_equal(bp.ref_set_tally(strips), oracle.tally(code, ref0))
    # the tallies over ALL genes of the strips' own genes, through the mirror rule
    full = oracle.tally(code, np.ones(G, dtype=bool))
    for j0, c in strips.items():
        assert np.array_equal(bp.column_histogram(c), full[j0:j0 + bp.STRIP]), j0


def test_reference_runs_sit_where_they_should():
    assert bp.ref_runs(131584) == [0, 65520, 131056, 131552] and bp.ref_runs(196700) == [0, 65520, 131056, 196668]
    assert bp.ref_runs(600) == [0, 184, 384, 568]
    m = bp.ref_set(131584)
    assert m.sum() == 128 and m[65535] and m[65536] and m[131071] and m[131072] and m[131583] and m[0] and not m[32]


@pytest.mark.parametrize("name,G,n_iter,n_conv,passes", [("counts", 600, 1, 3, 1), ("counts", 700, 5, 1, 5), ("counts", 400, 5, 3, 3),
                                                         ("counts", 600, 5, 1, 4), ("free", 600, 5, 3, 5), ("band", 500, 5, 3, 2),
                                                         ("counts", 400, 0, 3, 0)])
def test_reference_run_equals_the_oracles_iteration(oracle, name, G, n_iter, n_conv, passes):
    """bit for bit: a run of one pass, runs that converge (in the second, third and fourth pass) and runs that the pass limit cuts off
    (five passes that still change the reference set)"""
    X, Xf, gid, thr = _problem(oracle, name, G)
    code = oracle.build_codes(Xf, gid, 2, 0, thr[:, 0], SEED)
    ref0 = bp.ref_set(G)
    exp, eit, etr = oracle.iterate(code, ref0, 1.0, 0.05, n_iter, n_conv)
    seen = []
    res, it, tr = bp.reference_run(lambda ref: (seen.append(ref.copy()), oracle.tally(code, ref))[1], G, ref0, 1.0, 0.05, n_iter, n_conv)
    assert (it, tr) == (eit, etr) and it == passes
    assert np.array_equal(res, exp)                       # every column, bit for bit
    assert len(seen) == passes and (passes == 0 or np.array_equal(seen[0], ref0))
    if passes == 5:                                       # cut off, not converged: the last pass still moved the set
        assert abs(int(seen[-1].sum()) - tr[-1][1]) >= n_conv
    if passes in (2, 3, 4):
        assert abs(int(seen[-1].sum()) - tr[-1][1]) < n_conv


def test_iter_stats_is_one_pass_of_the_iteration(oracle, counts600):
    G, Xf, gid, thr, code, strips, ref0 = counts600
    res, inds, nn = oracle.iter_stats(bp.ref_set_tally(strips), 1.0, 0.05)
    exp, it, tr = oracle.iterate(code, ref0, 1.0, 0.05, 1, 3)
    assert np.array_equal(res, exp) and tr == [(G - nn, nn)] and int(inds.sum()) == nn and 0 < nn < G
    assert np.array_equal(inds == 0, (res[:, 0] <= 1.0) & (res[:, 1] <= 0.05))
    with pytest.raises(IndexError):                        # the reference's BoundsError: round(Int, 5 * 0.05) = 0
        oracle.iter_stats(np.ones((5, 9), dtype=np.int32), 1.0, 0.05)


def test_the_recipes_tie_where_they_claim_to(oracle):
    G = 700
    gid = bp.labels()
    assert gid.tolist() == [0, 1] * 8                    # interleaved: the transform re-orders the samples
    Xfree, Xcounts, Xband = bp.free(G, SEED), bp.counts(G, SEED), bp.band(G, SEED)
    assert Xfree.dtype == np.int64 and Xcounts.dtype == np.int64 and Xband.dtype == np.float64
    assert (np.sort(Xfree, axis=0) == np.arange(G)[:, None]).all()          # a permutation per sample: no tie anywhere
    assert Xcounts.min() == 0 and Xcounts.max() == 39
    for name, X in (("free", Xfree), ("counts", Xcounts), ("band", Xband)):
        gt, eq = oracle.pair_counts(np.asfortranarray(X.astype(np.float64)), gid, 2, 0, 64, 64, G)
        ties = eq.reshape(-1, 2).sum(axis=0)
        assert ((ties > 0).all() if bp.MATRICES[name][1] else (ties == 0).all()), (name, ties)
    # the band ties values that differ (an Int64 matrix cannot)
    d = np.abs(Xband[:64, None, :] - Xband[None, 64:, :])
    assert ((d < 0.1) & (d > 0)).any(axis=(0, 1)).all()
    # the top value of counts is a tie group in every sample: its high position is the gene count
    assert ((Xcounts == 39).sum(axis=0) > 1).all()
    # the effects make genes that the passes can call: in both recipes a tenth of the genes is shifted in group 1, up and down
    eff = bp._effects(SEED, G)
    assert (eff > 0).sum() > G // 40 and (eff < 0).sum() > G // 40
    for X in (Xfree, Xcounts):
        shift = X[:, gid == 1].mean(axis=1) - X[:, gid == 0].mean(axis=1)
        assert (np.sign(shift[eff != 0]) == np.sign(eff[eff != 0])).mean() > 0.9


def test_thresholds_leave_room_for_all_nine_classes(oracle, counts600):
    assert oracle.threshold(8, 0.1) == 7 and oracle.threshold(8, 0.01) == 8
    G, Xf, gid, thr, code, strips, ref0 = counts600
    assert thr.tolist() == [[7, 7], [7, 7]]
    seen = np.zeros(9, dtype=np.int64)
    for c in strips.values():
        seen += np.bincount(c[c < 9], minlength=9)
    assert (seen > 0).all(), seen


# ------------------------------------------------------------------------------------------- planted errors: every comparison can fail

def test_one_flipped_code_fails_the_code_comparison(counts600):
    G, Xf, gid, thr, code, strips, ref0 = counts600
    j0 = bp.ref_runs(G)[1]
    exp = strips[j0]
    bp.check_codes(exp.copy(), exp, 0, j0)
    for (a, b) in ((0, 0), (G - 1, 31), (j0 + 3, 3), (311, 17)):    # (j0 + 3, 3) is on the diagonal
        bad = exp.copy()
        bad[a, b] = 4 if exp[a, b] != 4 else 5
        with pytest.raises(AssertionError, match=rf"first \({a}, {j0 + b}\)"):
            bp.check_codes(bad, exp, 0, j0, "planted")
    with pytest.raises(AssertionError):
        bp.check_codes(exp.astype(np.int16), exp, 0, j0)
    blk = code[40:80, 300:340]
    bp.check_mirror(blk, code[300:340, 40:80], 40, 300)
    bp.check_mirror(code[40:80, 40:80], code[40:80, 40:80], 40, 40)
    bad = blk.copy()
    bad[5, 6] = 8 - bad[5, 6] if bad[5, 6] != 4 else 3
    with pytest.raises(AssertionError):
        bp.check_mirror(bad, code[300:340, 40:80], 40, 300)
    bad = code[40:80, 40:80].copy()
    bad[7, 7] = 4                                          # a class on the diagonal
    with pytest.raises(AssertionError):
        bp.check_mirror(bad, code[40:80, 40:80], 40, 40)


def test_one_tally_off_by_one_fails_the_tally_comparisons(oracle, counts600):
    G, Xf, gid, thr, code, strips, ref0 = counts600
    exp = bp.ref_set_tally(strips)
    bp.check_tally(oracle.tally(code, ref0), exp)
    for (gene, c) in ((0, 0), (G - 1, 8), (299, 4)):
        bad = exp.copy()
        bad[gene, c] += 1
        with pytest.raises(AssertionError, match=rf"first gene {gene}:"):
            bp.check_tally(bad, exp, what="planted")
    # ... and the row form: tally(ones) at a strip's own genes against its column histogram
    full = oracle.tally(code, np.ones(G, dtype=bool))
    j0 = bp.ref_runs(G)[2]
    rows = np.arange(j0, j0 + bp.STRIP)
    bp.check_tally(full[rows], bp.column_histogram(strips[j0]), rows)
    bad = full[rows].copy()
    bad[31, 2] -= 1
    with pytest.raises(AssertionError, match=rf"first gene {j0 + 31}:"):
        bp.check_tally(bad, bp.column_histogram(strips[j0]), rows, "planted")
    # one code wrong in a strip moves a unit between two tallies: the sums see it
    wrong = {k: v.copy() for k, v in strips.items()}
    wrong[j0][100, 9] = (wrong[j0][100, 9] + 1) % 9
    with pytest.raises(AssertionError, match="first gene 100:"):
        bp.check_tally(oracle.tally(code, ref0), bp.ref_set_tally(wrong))


def test_one_inverted_coin_fails_the_code_comparison(oracle, counts600, monkeypatch):
    """the coin of one key turned round (n_eq - wins for wins): the pair's class moves, expected_codes no longer equals the table"""
    G, Xf, gid, thr, code, strips, ref0 = counts600
    j0 = bp.ref_runs(G)[1]
    gt, eq = oracle.pair_counts(Xf, gid, 2, 0, G, j0, j0 + bp.STRIP)
    real = bp.coins
    hit = 0
    for a, b in np.argwhere(eq[:, :, 0] % 2 == 1):         # an odd n_eq: the inverted coin differs from the coin
        i, j = int(a), j0 + int(b)
        if i == j:
            continue
        lo, hi = min(i, j), max(i, j)

        def inverted(seed, ii, jj, g, n_eq, lo=lo, hi=hi):
            w = real(seed, ii, jj, g, n_eq)
            flip = (np.asarray(ii) == lo) & (np.asarray(jj) == hi) & (np.asarray(g) == 0)
            return np.where(flip, np.asarray(n_eq) - w, w)

        monkeypatch.setattr(bp, "coins", inverted)
        got = bp.expected_codes(oracle, Xf, gid, thr, SEED, 0, G, j0, j0 + bp.STRIP)
        monkeypatch.setattr(bp, "coins", real)
        diff = np.argwhere(got != strips[j0])
        if diff.size:                                     # (a coin far from both thresholds moves no class: try the next key)
            assert diff.tolist() == [[a, b]]
            with pytest.raises(AssertionError, match=rf"first \({i}, {j}\)"):
                bp.check_codes(code[:, j0:j0 + bp.STRIP], got, 0, j0)
            hit += 1
            if hit == 3:
                break
    assert hit == 3


def test_one_flipped_deg_call_fails_the_run_comparison(oracle, counts600):
    G, Xf, gid, thr, code, strips, ref0 = counts600
    exp = oracle.iterate(code, ref0, 1.0, 0.05, 5, 3)
    got = bp.reference_run(lambda ref: oracle.tally(code, ref), G, ref0, 1.0, 0.05, 5, 3)
    bp.check_run(got, exp, _check_result)
    res, it, tr = got
    deg = np.flatnonzero(res[:, 1] <= 0.05)
    non = np.flatnonzero(res[:, 1] > 0.05 + 10 * P_ATOL)
    assert deg.size and non.size
    for gene, padj in ((deg[0], 0.05 + 2 * P_ATOL), (non[0], 0.05)):       # one call across the cut
        bad = res.copy()
        bad[gene, 1] = padj
        with pytest.raises(AssertionError):
            bp.check_run((bad, it, tr), exp, _check_result)
    with pytest.raises(AssertionError):                                    # ... as the trace counts it
        bp.check_run((res, it, tr[:-1] + [(tr[-1][0] + 1, tr[-1][1] - 1)]), exp, _check_result)
    with pytest.raises(AssertionError):
        bp.check_run((res, it - 1, tr[:-1]), exp, _check_result)
    bad = res.copy()
    bad[5, 2 + 4] += 1                                                      # a tally
    with pytest.raises(AssertionError, match="tallies differ"):
        bp.check_run((bad, it, tr), exp, _check_result)
    bad = res.copy()
    bad[7, 11] *= 1 + 10 * STAT_RTOL                                        # delta1 of one gene
    if abs(res[7, 11]) > 1e-3:
        with pytest.raises(AssertionError):
            bp.check_run((bad, it, tr), exp, _check_result)
    # a reference whose tallies come from a wrong scan gives another run: one unit in one pass
    n = [0]

    def off_by_one(ref):
        cont = oracle.tally(code, ref)
        n[0] += 1
        if n[0] == 2:
            cont[17, 0] += 1
            cont[17, 4] -= 1
        return cont
    with pytest.raises(AssertionError):
        bp.check_run(bp.reference_run(off_by_one, G, ref0, 1.0, 0.05, 5, 3), exp, _check_result)


def test_half_height_items_at_18_planes(tmp_path):
    """Which cells of the 131 584-gene table a half-height item of the pair kernel writes: csrc/k1_items.h run on the host for that launch
    (two sides, one 32-sample block each, the 256 compute units of an MI355X).  The blocks that tests/test_gpu_big_planes.py compares for
    them, and the rows that its column strips cross, lie in halved items; the last 64 rows of the table do not."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "k1_halves_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(root, "rankcompv3.jl_amd", "csrc"),
                           "-o", exe, os.path.join(root, "tests", "k1_halves_driver.cpp")])
    G = 131584
    lines = subprocess.run([exe, str(G), "1", "256"], capture_output=True, text=True, check=True).stdout.split("\n")
    n_items, n_halved = (int(v) for v in lines[0].split())
    halved = {tuple(int(v) for v in l.split()) for l in lines[1:] if l}
    assert n_halved == len(halved) == 48 and n_items == 2117680 and n_items % 2048 == 48   # 2 048 wave slots: the last round has 48 items
    assert {s for s, c, t in halved} == {1}                                                 # the treat side's
    assert max(32 * t + 31 for s, c, t in halved) < G - 64                                  # none in the last 64 rows
    for i0, j0 in bp.HALF_ITEMS:
        assert i0 % 32 == 0 and (1, j0 // 256, i0 // 32) in halved and (j0 + 63) // 256 == j0 // 256, (i0, j0)
        assert j0 + 63 > i0                                                                 # pairs i < j of the item are in the block
    for j0, rows in bp.HALF_ITEM_ROWS_IN_STRIPS.items():
        assert j0 in bp.ref_runs(G)
        cols = {c for c in range(j0, j0 + bp.STRIP) if any((1, c // 256, i0 // 32) in halved for i0 in rows)}
        assert cols and all((1, c // 256, i0 // 32) in halved for c in cols for i0 in rows), (j0, rows)
    # the other gene counts of the GPU file: nothing halved at the plane boundary, eight items at 196 700 genes x 8 samples
    for G2, want in ((131071, 0), (131072, 0), (196700, 8)):
        out = subprocess.run([exe, str(G2), "1", "256"], capture_output=True, text=True, check=True).stdout.split("\n")
        assert int(out[0].split()[1]) == want, (G2, out[0])
