"""Cells to DEGs with the profiles resident, on the GPU: reo_set_matrix_pseudobulk_* against Context.pseudobulk and numpy, bit for bit;
reo_filter_matrix (masks, G', S', the compacted matrix) against the numpy statement of src/RankCompV3.jl:618 / :626; identify_degs_cells
against today's route, Context.pseudobulk -> numpy filters -> run_identify_degs, bit for bit.  Every case is small; the one large case is the
index-width case, which lives on the device only."""
import importlib

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

NP = {"f64": np.float64, "i64": np.int64, "f32": np.float32}


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.asfortranarray(a).tobytes(order="F") == np.asfortranarray(b).tobytes(order="F")


def filters_numpy(X, min_profiles, min_features):
    """src/RankCompV3.jl:618 then :626 as reoa.prepare writes them."""
    with np.errstate(invalid="ignore"):
        s_inds = (X > 0).sum(axis=0) > min_profiles
        kept = X[:, s_inds]
        inds = (kept > 0).sum(axis=1) > min_features
    return s_inds, inds, kept[inds, :]


# ---- resident pseudo-bulk ---------------------------------------------------------------------------------------------------------

PB_G, PB_C = 16384 + 37, 300      # crosses the kPbRows tile of pb_csc


def _pb_case(kind):
    """16 421 genes x 300 cells, about 2 % filled, one cell with 5 000 entries (more than 2 x 1024: the slow loop of pb_csc), entries in
    the rows on both sides of row 16 384; 9 profiles over a shuffled subset of the cells, the fifth one empty."""
    rng = np.random.default_rng(0x5EED0C31)
    D = np.zeros((PB_G, PB_C), dtype=NP[kind])
    fill = rng.random((PB_G, PB_C)) < 0.02
    fill[:, 41] = False
    fill[rng.choice(PB_G, 5000, replace=False), 41] = True
    fill[16383:16386, 7] = True
    fill[PB_G - 1, 299] = True
    n = int(fill.sum())
    D[fill] = rng.integers(1, 60, n) if kind == "i64" else rng.random(n) * 10.0 + 0.1
    order = rng.permutation(PB_C)[:280].astype(np.int32)
    if 41 not in order:
        order[3] = 41
    ptr = np.array([0, 40, 41, 100, 140, 140, 200, 230, 279, 280], dtype=np.int32)
    exp = np.zeros((PB_G, 9), dtype=NP[kind])
    for o in range(9):
        for c in order[ptr[o]:ptr[o + 1]]:
            exp[:, o] = exp[:, o] + D[:, c]      # left to right, as the reference sums (:63)
    return D, order, ptr, exp


_PB_CACHE = {}


def pb_case(kind):
    if kind not in _PB_CACHE:
        _PB_CACHE[kind] = _pb_case(kind)
    return _PB_CACHE[kind]


@pytest.mark.parametrize("form", ["dense", "csc"])
@pytest.mark.parametrize("kind", ["i64", "f64"])
def test_resident_pseudobulk_equals_the_host_one_and_numpy(pkg, form, kind):
    D, order, ptr, exp = pb_case(kind)
    cells = sp.csc_matrix(D) if form == "csc" else D
    if form == "csc":
        assert int(np.diff(cells.indptr).max()) > 2 * 1024
    with pkg.Context(device=0, seed=1) as ctx:
        host = ctx.pseudobulk(cells, order, ptr)
        ctx.set_matrix_pseudobulk(cells, order, ptr)
        info = ctx.info()
        got = ctx.get_matrix()
        assert (info["G"], info["S"], info["resident_dtype"]) == (PB_G, 9, 2 if kind == "i64" else 1)
        assert (info["upload_link_bytes"], info["rowmajor_upload"], info["csc_upload"], info["csc_nnz"]) == (0, 0, 0, 0)
        assert (ctx.G, ctx.S) == (PB_G, 9)
    assert same_bits(host, exp)
    assert same_bits(got, exp) and same_bits(got, host)
    assert not got[:, 4].any()                              # the empty profile


def test_resident_pseudobulk_refuses_a_bad_row_index_and_the_context_lives_on(pkg):
    D, order, ptr, exp = pb_case("i64")
    m = sp.csc_matrix(D)
    colptr, val = m.indptr.astype(np.int64), m.data.astype(np.int64)
    rowidx = m.indices.astype(np.int32).copy()
    rowidx[rowidx.size // 2] = PB_G                          # one past the last row
    with pkg.Context(device=0, seed=1) as ctx:
        ctx.set_matrix(np.asfortranarray(D[:50, :20]))
        assert ctx.info()["resident_dtype"] == 2
        rc = ctx._L.reo_set_matrix_pseudobulk_csc_i64(ctx._h, PB_G, PB_C, colptr.ctypes.data, rowidx.ctypes.data, val.ctypes.data,
                                                      order.ctypes.data, order.size, ptr.ctypes.data, 9)
        assert rc == pkg._ffi.REO_EINVAL and "row index" in ctx._L.reo_last_error().decode()
        assert ctx.info()["resident_dtype"] == 0            # no matrix after a failure
        with pytest.raises(pkg.DimensionMismatch):
            ctx.get_matrix()
        with pytest.raises(pkg.DimensionMismatch):
            ctx.filter_matrix()
        with pytest.raises(pkg.DimensionMismatch):          # a shape that reo_set_matrix_* would not take: one profile
            ctx.set_matrix_pseudobulk(m, order, np.array([0, order.size], dtype=np.int32))
        ctx.set_matrix_pseudobulk(m, order, ptr)             # ... and usable
        assert same_bits(ctx.get_matrix(), exp)
        with pytest.raises(pkg.DimensionMismatch):          # reo_get_matrix wants the exact size
            pkg._ffi.check(ctx._L.reo_get_matrix(ctx._h, exp.ctypes.data, exp.nbytes - 8))


# ---- the filters -------------------------------------------------------------------------------------------------------------------

def filter_table(G, S, kind, seed):
    """About 45 % positive values, the rest zeros and negatives (signed zeros among the floats); thresholds at the medians of the counts,
    so that counts equal to a threshold occur and are dropped, something goes and at least two of each stay."""
    rng = np.random.default_rng(seed)
    u = rng.random((G, S))
    pos = u < 0.25 + 0.4 * rng.random((1, S)) * rng.random((G, 1)) * 2
    X = np.where(pos, rng.integers(1, 9, (G, S)), 0).astype(NP[kind])
    neg = (u > 0.9)
    X[neg] = -X[neg] - 1
    if kind != "i64":
        X[(u > 0.85) & ~neg] = -0.0
        X[pos] += NP[kind](0.25)
    cc = (X > 0).sum(axis=0)
    mp = int(np.sort(cc)[S // 2 - 1]) if S > 8 else int(np.sort(cc)[1])
    gc = (X[:, cc > mp] > 0).sum(axis=1)
    mf = int(np.sort(gc)[G // 2 - 1]) if G > 8 else int(np.sort(gc)[1])
    return np.asfortranarray(X), mp, mf


def check_filter(ctx, X, mp, mf):
    pk, gk, exp = filters_numpy(X, mp, mf)
    got_pk, got_gk = ctx.filter_matrix(mp, mf)
    assert got_pk.dtype == np.bool_ and got_gk.dtype == np.bool_
    assert np.array_equal(got_pk, pk) and np.array_equal(got_gk, gk)
    info = ctx.info()
    assert (info["G"], info["S"]) == exp.shape == (ctx.G, ctx.S)
    assert same_bits(ctx.get_matrix(), np.asfortranarray(exp))
    return pk, gk, exp


@pytest.mark.parametrize("shape", [(5, 4099), (4099, 5), (257, 65)])
@pytest.mark.parametrize("kind", ["f64", "i64", "f32"])
def test_filter_matches_numpy(pkg, kind, shape):
    G, S = shape
    X, mp, mf = filter_table(G, S, kind, 0x5EED0C40 + G)
    pk, gk, exp = filters_numpy(X, mp, mf)
    cc = (X > 0).sum(axis=0)
    assert 2 <= pk.sum() < S and 2 <= gk.sum() < G                       # something goes, enough stays
    assert (cc == mp).any() and not pk[cc == mp].any()                   # a count equal to the threshold is dropped
    gc = (X[:, pk] > 0).sum(axis=1)
    assert (gc == mf).any() and not gk[gc == mf].any()
    with pkg.Context(device=0, seed=1) as ctx:
        ctx.set_matrix(X)
        assert ctx.info()["resident_dtype"] == {"f64": 1, "i64": 2, "f32": 3}[kind]
        check_filter(ctx, X, mp, mf)
        ctx.set_profiling(True)
        # a second filter on what is left, with nothing to drop: masks all true, the matrix stays
        pk2, gk2 = ctx.filter_matrix(-1, -1)
        assert pk2.all() and gk2.all() and pk2.size == exp.shape[1] and gk2.size == exp.shape[0]
        assert same_bits(ctx.get_matrix(), np.asfortranarray(exp))
        assert ctx.timings()["pseudobulk_ms"] > 0                        # stage timer 7 covers the filter's kernels


def test_filter_on_a_device_buffer_with_a_leading_dimension_leaves_it_alone(pkg):
    import torch
    G, S = 257, 65
    X, mp, mf = filter_table(G, S, "f64", 0x5EED0C51)
    tall = torch.full((S, G + 3), 99.0, dtype=torch.float64, device="cuda:0")   # (a positive pad: a read past G would count it)
    tall[:, :G] = torch.from_numpy(np.ascontiguousarray(X.T)).to("cuda:0")
    before = tall.clone()
    t = tall[:, :G].t()
    assert t.stride() == (1, G + 3)
    with pkg.Context(device=0, seed=1) as ctx:
        ctx.set_matrix_tensor(t)
        assert same_bits(ctx.get_matrix(), X)                             # ld removed
        check_filter(ctx, X, mp, mf)
        torch.cuda.synchronize()
        assert torch.equal(tall, before)                                  # the caller's buffer has not been written
        # nothing dropped: the caller's buffer stays the matrix, unchanged
        ctx.set_matrix_tensor(t)
        pk, gk = ctx.filter_matrix(-1, -1)
        assert pk.all() and gk.all() and same_bits(ctx.get_matrix(), X)
        assert torch.equal(tall, before)


SUB64, SUB32 = 5e-324, np.float32(1e-45)


@pytest.mark.parametrize("kind", ["f64", "f32"])
def test_filter_special_values_dropped_column_genes_and_thresholds(pkg, kind):
    """-0.0, negatives, -Inf and NaN do not count, +Inf and subnormals do; g3 is expressed only in s3, which (1 positive = min_profiles) is
    dropped, so g3 goes too; with min_features = 1, g1 (1 positive among the kept = the threshold) goes as well.  The table reaches the
    device as a tensor: its bits are the test's."""
    import torch
    sub = SUB64 if kind == "f64" else SUB32
    nan, inf = np.nan, np.inf
    X = np.array([
        [-0.0, 1.0, 2.0, 0.0, nan],
        [-1.0, inf, 0.0, 0.0, nan],
        [0.0,  sub, sub, 0.0, -inf],
        [-0.0, 0.0, -3.0, 7.0, nan],
        [nan,  0.0, -0.0, 0.0, 0.0],
    ], dtype=NP[kind])
    X[2, 1] = X[2, 2] = sub
    assert 0 < X[2, 1] < np.finfo(NP[kind]).tiny
    for mp, mf, want_pk, want_gk in [(1, 0, [0, 1, 1, 0, 0], [1, 1, 1, 0, 0]), (1, 1, [0, 1, 1, 0, 0], [1, 0, 1, 0, 0]),
                                     (0, 0, [0, 1, 1, 1, 0], [1, 1, 1, 1, 0])]:
        pk, gk, exp = filters_numpy(X, mp, mf)
        assert pk.tolist() == [bool(v) for v in want_pk] and gk.tolist() == [bool(v) for v in want_gk]
        t = torch.from_numpy(np.ascontiguousarray(X.T)).to("cuda:0").t()
        assert t.stride() == (1, 5)
        with pkg.Context(device=0, seed=1) as ctx:
            ctx.set_matrix_tensor(t)
            assert same_bits(ctx.get_matrix(), np.asfortranarray(X))
            check_filter(ctx, X, mp, mf)


def test_filter_all_dropped_is_refused_and_the_context_lives_on(pkg):
    X, _, _ = filter_table(257, 65, "i64", 0x5EED0C52)
    with pkg.Context(device=0, seed=1) as ctx:
        ctx.set_matrix(X)
        with pytest.raises(pkg.DimensionMismatch) as e:
            ctx.filter_matrix(257, 0)                                     # no profile has more than G positives
        assert "0 of 65 profiles" in e.value.message and "of 257 genes" in e.value.message
        assert ctx.info()["resident_dtype"] == 0
        with pytest.raises(pkg.DimensionMismatch):
            ctx.get_matrix()
        cc = (X > 0).sum(axis=0)
        top = int(np.sort(cc)[-2])                                        # leaves one profile (or none): S' < 2
        ctx.set_matrix(X)
        with pytest.raises(pkg.DimensionMismatch) as e:
            ctx.filter_matrix(top, 0)
        assert "profiles are left" in e.value.message
        ctx.set_matrix(X)                                                 # set_matrix works again
        assert same_bits(ctx.get_matrix(), X)
        gid, lev = pkg.encode_groups(pkg.synth.groups(65))
        ctx.set_groups(gid, 2); ctx.compute_thresholds(0.01); ctx.build_pairs(0)
        res, it, tr = ctx.identify_degs(pkg.synth.ref_mask(257, 60, 3), 1.0, 0.05, 3, 1)
        assert it >= 1


def test_filter_invalidates_and_stale_groups_fail_like_the_reference(pkg):
    G, S = 257, 65
    X, mp, mf = filter_table(G, S, "i64", 0x5EED0C53)
    gid, lev = pkg.encode_groups(pkg.synth.groups(S))
    ref0 = pkg.synth.ref_mask(G, 60, 3)
    with pkg.Context(device=0, seed=5) as ctx:
        ctx.set_groups(gid, 2); ctx.compute_thresholds(0.01)
        ctx.set_matrix(X)                                                 # (ranked by the pipelined upload: done again below)
        ctx.build_pairs(0)
        pk, gk, exp = check_filter(ctx, X, mp, mf)
        with pytest.raises(pkg.DimensionMismatch) as e:
            ctx.build_pairs(0)
        assert "compatible sizes" in e.value.message
        gid2, lev2 = pkg.encode_groups(np.asarray(pkg.synth.groups(S))[pk])
        ctx.set_groups(gid2, len(lev2)); ctx.compute_thresholds(0.01); ctx.build_pairs(0)
        got = ctx.identify_degs(ref0[gk], 1.0, 0.05, 4, 1)
    with pkg.Context(device=0, seed=5) as ctx:                            # the same problem from the host copy
        ctx.set_groups(gid2, len(lev2)); ctx.compute_thresholds(0.01)
        ctx.set_matrix(np.asfortranarray(exp)); ctx.build_pairs(0)
        want = ctx.identify_degs(ref0[gk], 1.0, 0.05, 4, 1)
    assert got[1:] == want[1:] and np.array_equal(got[0], want[0], equal_nan=True)


def test_multi_context_refuses_the_filter_and_the_resident_pseudobulk(pkg, monkeypatch):
    monkeypatch.setenv("REO_MULTI_ONE_DEVICE", "1")
    X, mp, mf = filter_table(257, 65, "i64", 0x5EED0C54)
    with pkg.Context(seed=1, n_gpus=2) as ctx:
        ctx.set_matrix(X)
        with pytest.raises(pkg.DimensionMismatch) as e:
            ctx.filter_matrix(mp, mf)
        assert "reo_create_multi" in e.value.message
        with pytest.raises(pkg.DimensionMismatch) as e:
            ctx.set_matrix_pseudobulk(X, np.arange(65, dtype=np.int32), np.array([0, 30, 65], dtype=np.int32))
        assert "reo_create_multi" in e.value.message
        assert same_bits(ctx.get_matrix(), X)                             # the matrix it had is still there


def test_filter_offsets_are_64_bit(pkg):
    """262 143 x 8 200 Float32 zeros made on the device (2.15e9 elements, past 2^31; 8.6 GB), a handful of positives at the far corners."""
    import torch
    G, S = 262143, 8200
    assert G * S > 2 ** 31
    tall = torch.zeros((S, G), dtype=torch.float32, device="cuda:0")
    t = tall.t()
    assert t.stride() == (1, G)
    put = {(0, 0): 1.5, (G - 1, 0): 2.5, (0, S - 1): 3.5, (G - 1, S - 1): 4.5, (131071, 4100): 5.5, (G - 1, 4100): 6.5,
           (5, 17): -1.0, (G - 2, S - 2): -2.0}                          # (the negatives keep nothing)
    for (g, s), v in put.items():
        t[g, s] = v
    cols, genes = [0, 4100, S - 1], [0, 131071, G - 1]
    exp = np.zeros((3, 3), dtype=np.float32, order="F")
    for (g, s), v in put.items():
        if v > 0:
            exp[genes.index(g), cols.index(s)] = v
    with pkg.Context(device=0, seed=1) as ctx:
        ctx.set_matrix_tensor(t)
        pk, gk = ctx.filter_matrix(0, 0)
        assert np.flatnonzero(pk).tolist() == cols and np.flatnonzero(gk).tolist() == genes
        assert (ctx.info()["G"], ctx.info()["S"]) == (3, 3)
        assert same_bits(ctx.get_matrix(), exp)
    del t, tall
    torch.cuda.empty_cache()


# ---- end to end --------------------------------------------------------------------------------------------------------------------

E2E_G, E2E_C = 300, 900


def e2e_cells(ngroups):
    """300 genes x 900 cells of Poisson counts, about 6 % filled: gene rates spread over two decades (rare genes fall to min_features),
    cell depths over one (shallow profiles fall to min_profiles), a third of the genes up in the second group.  Cells of the groups are
    interleaved."""
    rng = np.random.default_rng(0x5EED0C60 + ngroups)
    labels = [f"grp{t % ngroups}" for t in range(E2E_C)]
    rate = 10.0 ** rng.uniform(-3.0, -0.45, E2E_G)
    depth = 10.0 ** rng.uniform(-0.7, 0.3, E2E_C)
    lam = rate[:, None] * depth[None, :]
    up = rng.random(E2E_G) < 0.33
    second = np.array([l == "grp1" for l in labels])
    lam[np.ix_(up, second)] *= 4.0
    X = rng.poisson(lam).astype(np.int64)
    return X, labels


def e2e_thresholds(pkg, X, labels, n_pseudo, seed):
    """Thresholds from the data: the second smallest profile count (so at least two profiles go) and the gene count at the lower fifth."""
    R = importlib.import_module(pkg.__name__ + ".reoa")
    order, ptr, names, groups = pkg.cells_partition(labels, n_pseudo, seed)
    pb = R.host_sums(X, order, ptr)
    cc = (pb > 0).sum(axis=0)
    mp = int(np.sort(cc)[1])
    gc = (pb[:, cc > mp] > 0).sum(axis=1)
    mf = int(np.sort(gc)[E2E_G // 5])
    return mp, mf, pb


_OLD = {}


def old_route(pkg, ngroups, n_pseudo, mp, mf, refkind, seed):
    """Today's three steps: Context.pseudobulk -> numpy filters and a contiguous copy -> run_identify_degs."""
    key = (ngroups, mp, mf, refkind)
    if key in _OLD:
        return _OLD[key]
    X, labels = e2e_cells(ngroups)
    order, ptr, names, groups = pkg.cells_partition(labels, n_pseudo, seed)
    with pkg.Context(device=0, seed=seed) as ctx:
        pb = ctx.pseudobulk(sp.csc_matrix(X), order, ptr)
    pk, gk, pbk = filters_numpy(pb, mp, mf)
    pbk = np.ascontiguousarray(pbk)
    gnames = [f"gene{i}" for i in range(E2E_G)]
    Gk = int(gk.sum())
    ref = e2e_ref(pkg, seed)[gk] if refkind == "mask" else pkg.synth.ref_mask(Gk, min(Gk, 3000), seed)
    run = pkg.run_identify_degs(pbk, [g for g, k in zip(groups, pk) if k], [n for n, k in zip(gnames, gk) if k], 0.01, 1.0, 0.05, ref, 8, 1,
                                seed=seed, device=0)
    _OLD[key] = (run, pk, gk, pb, [n for n, k in zip(names, pk) if k], [g for g, k in zip(groups, pk) if k])
    return _OLD[key]


def e2e_ref(pkg, seed):
    return pkg.synth.ref_mask(E2E_G, 120, seed ^ 0x77)


def same_run(a, b):
    assert a.iters_run == b.iters_run and a.trace == b.trace and a.levels == b.levels
    assert np.array_equal(a.thresholds, b.thresholds)
    assert list(a.gene_names) == list(b.gene_names)
    assert len(a.comparisons) == len(b.comparisons)
    for ca, cb in zip(a.comparisons, b.comparisons):
        assert ca["k"] == cb["k"] and ca["iters_run"] == cb["iters_run"] and ca["trace"] == cb["trace"]
        assert ca["result"].tobytes(order="F") == cb["result"].tobytes(order="F")
        assert list(ca["labels"]) == list(cb["labels"])
    assert np.array_equal(a.res[:, 0], b.res[:, 0])


@pytest.mark.parametrize("refkind", ["mask", "none"])
@pytest.mark.parametrize("form", ["sparse", "dense"])
@pytest.mark.parametrize("ngroups,n_pseudo", [(2, 7), (3, 5)])
def test_cells_to_degs_equals_the_three_step_route(pkg, ngroups, n_pseudo, form, refkind):
    seed = 0x5EED0C70
    X, labels = e2e_cells(ngroups)
    assert 0.05 < (X > 0).mean() < 0.075
    mp, mf, pb_host = e2e_thresholds(pkg, X, labels, n_pseudo, seed)
    old, pk, gk, pb, names, groups = old_route(pkg, ngroups, n_pseudo, mp, mf, refkind, seed)
    assert same_bits(pb, pb_host)
    assert 0 < (~gk).sum() and 0 < (~pk).sum() and gk.sum() >= 10
    assert len(set(groups)) == ngroups
    cells = sp.csr_matrix(X) if form == "sparse" else X
    gnames = [f"gene{i}" for i in range(E2E_G)]
    got = pkg.identify_degs_cells(cells, labels, gnames, n_pseudo, 0.01, 1.0, 0.05, e2e_ref(pkg, seed) if refkind == "mask" else None, 8, 1,
                                  min_profiles=mp, min_features=mf, seed=seed, device=0)
    assert np.array_equal(got.gene_kept, gk) and np.array_equal(got.profile_kept, pk)
    assert got.profile_names == names and got.profile_groups == groups
    assert got.run.gene_names == [n for n, k in zip(gnames, gk) if k]
    same_run(got.run, old)
    assert (got.run.info["G"], got.run.info["S"]) == (int(gk.sum()), int(pk.sum()))
    assert old.iters_run >= 1 and len(old.comparisons) == (1 if ngroups == 2 else 3)


def test_cells_to_degs_with_the_filters_at_zero_keeps_the_profiles_resident(pkg):
    seed = 0x5EED0C70
    X, labels = e2e_cells(2)
    old, pk, gk, pb, names, groups = old_route(pkg, 2, 7, 0, 0, "none", seed)
    assert pk.all()                                                       # (genes that no profile expresses go even at 0)
    gnames = [f"gene{i}" for i in range(E2E_G)]
    got = pkg.identify_degs_cells(sp.csc_matrix(X), labels, gnames, 7, 0.01, 1.0, 0.05, None, 8, 1, seed=seed, device=0)
    assert np.array_equal(got.gene_kept, gk) and got.profile_kept.all()
    same_run(got.run, old)
    # the same steps by hand: after the pair table and the iteration the resident matrix is still the (filtered) host pseudo-bulk
    order, ptr, _, _ = pkg.cells_partition(labels, 7, seed)
    with pkg.Context(device=0, seed=seed) as ctx:
        ctx.set_matrix_pseudobulk(sp.csc_matrix(X), order, ptr)
        assert same_bits(ctx.get_matrix(), pb)
        pk2, gk2 = ctx.filter_matrix(0, 0)
        gid, lev = pkg.encode_groups(groups)
        ctx.set_groups(gid, len(lev)); thr = ctx.compute_thresholds(0.01); ctx.build_pairs(0)
        Gk = int(gk2.sum())
        res, it, tr = ctx.identify_degs(pkg.synth.ref_mask(Gk, min(Gk, 3000), seed), 1.0, 0.05, 8, 1)
        assert same_bits(ctx.get_matrix(), np.asfortranarray(pb[gk]))
    assert it == old.iters_run and tr == old.trace and np.array_equal(thr, old.thresholds)
    assert res.tobytes(order="F") == old.result.tobytes(order="F")
