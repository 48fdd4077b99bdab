"""Sparse host matrices on the GPU (reo_set_matrix_csc_*): CSC columns checked and narrowed by the host threads, made dense on the device
by t_csc_columns.  The yardstick in every case is the column-major entry on the densified array (Fortran order) in the same process and
under the same settings (that path is pinned against the oracle by test_gpu_parity.py / test_gpu_float32.py): class table, tallies,
identify_degs and has_ties must be equal bit for bit.  Every sparse run asserts info()["csc_upload"] == 1 and csc_nnz == M.nnz (or calls
the _csc_ symbol itself), so nothing passes by a quiet toarray()."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

P_ATOL = 1e-6      # the tolerances of test_gpu_parity.py (oracle comparison only; everything else is bit-equality)
STAT_RTOL = 1e-7
T = 2048           # kCscTile of csrc/transform.hip: the gene rows of one workgroup's tile
ENV = ("REO_EAGER_UPLOAD", "REO_UPLOAD_THREADS", "REO_EAGER_CHUNK", "REO_EAGER_RANGES", "REO_ROWMAJOR", "REO_ROWMAJOR_COPY")


def _setenv(monkeypatch, **kw):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    for name, val in kw.items():
        if val is not None:
            monkeypatch.setenv(name, str(val))


def _csc_of(D, mask):
    """the CSC matrix that stores exactly the positions of `mask` (zeros among them stay stored), built from its three arrays"""
    G, S = D.shape
    cols, rows = np.nonzero(mask.T)                                             # column by column, rows ascending
    indptr = np.concatenate([[0], np.cumsum(mask.sum(axis=0))]).astype(np.int32)
    M = sp.csc_matrix((np.zeros(rows.size, dtype=np.float64), rows.astype(np.int32), indptr), shape=(G, S))
    M.data = np.ascontiguousarray(D.T[mask.T])                                  # (set afterwards: any dtype, -0.0 and explicit zeros as they are)
    assert M.has_canonical_format and M.nnz == int(mask.sum()) and M.dtype == D.dtype
    return M


def _thin(X, seed, density=0.1, force=()):
    """(sparse M, dense D): X thinned to about `density` by a seeded mask; always an empty column (1), a full column (2), a gene row
    without a value (the last: its entry in the full column is an explicitly stored zero) and one more stored zero; force: (row,
    column, value) entries stored on top of that"""
    G, S = X.shape
    rng = np.random.default_rng(seed)
    mask = rng.random((G, S)) < density
    mask[:, 1] = False
    mask[:, 2] = True
    D = np.where(mask, X, np.zeros((), dtype=X.dtype)).astype(X.dtype)
    D[G - 1, :] = 0
    mask[0, 0] = True; D[0, 0] = 0                                              # an explicitly stored zero
    for g, c, v in force:
        mask[g, c] = True; D[g, c] = v
    M = _csc_of(D, mask)
    assert np.array_equal(M.astype(np.float64).toarray(), D.astype(np.float64)) and (M.data == 0).sum() >= 2
    assert M.indptr[2] == M.indptr[1] and M.indptr[3] - M.indptr[2] == G
    return M, D


def _data(pkg, kind, G, S, seed):
    if kind == "i64": return pkg.synth.t1_counts(G, S, seed)
    if kind == "i32": return pkg.synth.t1_counts(G, S, seed).astype(np.int32)
    if kind == "f64": return pkg.synth.float_expr(G, S, seed)
    if kind == "f32": return pkg.synth.float_expr(G, S, seed).astype(np.float32)
    if kind == "f16": return pkg.synth.float_expr(G, S, seed).astype(np.float16)
    raise ValueError(kind)


def _run(pkg, X, group, seed, order, ref0=None, degs=True, n_gpus=None):
    """codes, tally, identify_degs, has_ties, link bytes of one context; a sparse X must take the CSC route, a dense one must not"""
    gid, lev = pkg.encode_groups(group)
    G = X.shape[0]
    kw = dict(seed=seed, n_gpus=n_gpus) if n_gpus else dict(device=0, seed=seed)
    with pkg.Context(**kw) as ctx:
        if order == "matrix_first":
            ctx.set_matrix(X)
        ctx.set_groups(gid, len(lev)); ctx.compute_thresholds(0.01)
        if order != "matrix_first":
            ctx.set_matrix(X)
        info = ctx.info()
        if sp.issparse(X):
            assert info["csc_upload"] == 1 and info["csc_nnz"] == X.nnz, (order, info["csc_upload"], info["csc_nnz"], X.nnz)
        else:
            assert info["csc_upload"] == 0 and info["csc_nnz"] == 0
        out = dict(link=info["upload_link_bytes"], ranges=info["eager_range_launches"], per_k=[])
        for k in range(1 if len(lev) == 2 else len(lev)):
            ctx.build_pairs(k)
            code = ctx.get_codes(0, G, 0, G)
            tal = ctx.tally(ref0) if ref0 is not None else None
            deg = ctx.identify_degs(ref0, 1.0, 0.05, 6, 0) if (degs and ref0 is not None) else None
            out["per_k"].append((code, tal, deg, ctx.info()["has_ties"]))
    return out


def _same(a, b, what):
    assert len(a["per_k"]) == len(b["per_k"])
    for (c0, t0, d0, h0), (c1, t1, d1, h1) in zip(a["per_k"], b["per_k"]):
        assert np.array_equal(c0, c1), (what, "class table")
        assert h0 == h1, (what, "has_ties")
        if t0 is not None:
            assert np.array_equal(t0, t1), (what, "tallies")
        if d0 is not None:
            assert d0[1] == d1[1] and d0[2] == d1[2], (what, "iterations / trace")
            assert np.array_equal(d0[0], d1[0], equal_nan=True), (what, "statistics")


SETTINGS = [  # (REO_EAGER_UPLOAD, REO_UPLOAD_THREADS, REO_EAGER_CHUNK): those of test_gpu_rowmajor.py
    (None, None, None), ("1", None, None), ("0", None, None), ("2", "0", None), ("2", "3", "37"), ("2", None, "37"), ("1", "0", "37"), ("0", "3", None),
    ("0", "0", None),
]


@pytest.mark.parametrize("kind", ["i64", "f64", "f32", "i32", "f16"])
@pytest.mark.parametrize("G", [2, 63, 65, 700, T - 1, T, T + 1])
def test_tile_and_chunk_edges(pkg, monkeypatch, kind, G):
    """G below, at and on both sides of the kernel's row tile (an odd G: every second column starts 8 bytes behind a 16-byte boundary),
    S = 41, chunks of 37 + 4 columns, every way off the host, both call orders, every element type (float16 through the cast)"""
    S, seed = 41, 0x5EED0C00 + G
    M, D = _thin(_data(pkg, kind, G, S, seed), seed)
    group = pkg.synth.groups(S)
    ref0 = np.arange(G) % 3 != 1 if G < 10 else pkg.synth.ref_mask(G, max(2, G // 5), seed)
    for eager, threads, chunk in SETTINGS:
        _setenv(monkeypatch, REO_EAGER_UPLOAD=eager, REO_UPLOAD_THREADS=threads, REO_EAGER_CHUNK=chunk)
        for order in ("matrix_first", "groups_first"):
            want = _run(pkg, np.asfortranarray(D), group, seed, order, ref0, degs=G >= 10)
            got = _run(pkg, M, group, seed, order, ref0, degs=G >= 10)
            _same(want, got, (kind, G, eager, threads, chunk, order))
            assert got["link"] >= 8 * (S + 1) + 4 * M.nnz


def test_no_entries_and_every_entry(pkg, monkeypatch):
    """nnz = 0 (null rowidx / val: identify_degs on an all-tied matrix) and a CSC matrix that stores every element"""
    _setenv(monkeypatch)
    G, S, seed = 300, 41, 0x5EED0C10
    group = pkg.synth.groups(S)
    ref0 = pkg.synth.ref_mask(G, 60, seed)
    X = pkg.synth.t1_counts(G, S, seed)
    for M, D in ((sp.csc_matrix((G, S), dtype=np.int64), np.zeros((G, S), dtype=np.int64)), (_csc_of(X, np.ones((G, S), dtype=bool)), X),
                 (sp.csc_matrix((G, S), dtype=np.float32), np.zeros((G, S), dtype=np.float32))):
        assert M.nnz in (0, G * S)
        for threads in (None, "0"):
            _setenv(monkeypatch, REO_UPLOAD_THREADS=threads)
            for order in ("groups_first", "matrix_first"):
                want = _run(pkg, np.asfortranarray(D), group, seed, order, ref0)
                _same(want, _run(pkg, M, group, seed, order, ref0), ("nnz", M.nnz, threads, order))


@pytest.mark.parametrize("kind", ["growing", "float_mixed"])
def test_the_ladder_changes_on_the_way(pkg, monkeypatch, kind):
    """G = 1100, S = 96, chunks of 32: the values' form on the link climbs at columns 40 and 70 -- Int64 from 16 over 32 to 64 bits,
    Float64 from integers over float32 numbers (+ 0.25) to rng.normal, with one stored -0.0 -- beside 16-bit row indices"""
    G, S, seed = 1100, 96, 0x5EED0C20
    rng = np.random.default_rng(12)
    if kind == "growing":
        X = rng.integers(1, 30000, size=(G, S)); X[:, 40:] += 40000; X[:, 70:] += 2 ** 40
    else:
        X = rng.integers(1, 900, size=(G, S)).astype(np.float64); X[:, 40:70] += 0.25; X[:, 70:] = rng.normal(8, 2, size=(G, S - 70))
    M, D = _thin(X, seed)
    if kind == "float_mixed":
        at = M.indptr[50] + 1                                                   # a stored -0.0 in column 50
        M.data[at] = -0.0; D[M.indices[at], 50] = -0.0
        assert np.signbit(M.data[at]) and np.signbit(D[M.indices[at], 50])
    group = pkg.synth.groups(S)
    ref0 = pkg.synth.ref_mask(G, G // 5, seed)
    for eager, threads, chunk in (("2", None, "32"), ("2", "3", "32"), ("0", None, None), ("1", "0", "32"), ("2", None, None)):
        _setenv(monkeypatch, REO_EAGER_UPLOAD=eager, REO_UPLOAD_THREADS=threads, REO_EAGER_CHUNK=chunk)
        for order in ("groups_first", "matrix_first"):
            want = _run(pkg, np.asfortranarray(D), group, seed, order, ref0)
            got = _run(pkg, M, group, seed, order, ref0)
            _same(want, got, (kind, eager, threads, chunk, order))
            link = got["link"] - 8 * (S + 1)
            assert 4 * M.nnz <= link <= 12 * M.nnz, (kind, link, M.nnz)
            assert got["link"] < want["link"], (kind, got["link"], want["link"])
            if threads == "0":
                assert link == 12 * M.nnz                                       # the arrays as they are
            elif chunk == "32" and order == "groups_first":
                assert 4 * M.nnz < link < 10 * M.nnz, (kind, link, M.nnz)      # chunk by chunk: the narrowest form that fits


@pytest.mark.parametrize("kind", ["unequal", "interleaved", "three_groups"])
def test_groups(pkg, monkeypatch, kind):
    G, S, seed = 700, 41, 0x5EED0C30
    rng = np.random.default_rng(13)
    M, D = _thin(pkg.synth.t1_counts(G, S, seed), seed)
    group = {"unequal": ["u"] * 9 + ["v"] * (S - 9), "interleaved": [("u", "v")[int(b)] for b in rng.integers(0, 2, S)],
             "three_groups": ["a"] * 12 + ["b"] * 15 + ["c"] * 14}[kind]
    ref0 = pkg.synth.ref_mask(G, 140, seed)
    for chunk in (None, "16"):
        _setenv(monkeypatch, REO_EAGER_CHUNK=chunk)
        for order in ("groups_first", "matrix_first"):
            want = _run(pkg, np.asfortranarray(D), group, seed, order, ref0)
            _same(want, _run(pkg, M, group, seed, order, ref0), (kind, chunk, order))


def test_ranges(pkg, monkeypatch):
    """the pair kernel's sides over ranges of blocks, fed by densified chunks"""
    G, S, seed = 1100, 300, 0x5EED0C40
    M, D = _thin(pkg.synth.t1_counts(G, S, seed), seed)
    group = pkg.synth.groups(S)
    ref0 = pkg.synth.ref_mask(G, 220, seed)
    _setenv(monkeypatch, REO_EAGER_RANGES="4", REO_EAGER_CHUNK="32")
    want = _run(pkg, np.asfortranarray(D), group, seed, "groups_first", ref0)
    got = _run(pkg, M, group, seed, "groups_first", ref0)
    _same(want, got, "ranges")
    assert got["ranges"] >= 4 and got["ranges"] == want["ranges"]


def test_above_65536_genes(pkg, monkeypatch):
    """G = 66 000: 32-bit row indices, 33 tiles per column, the plain upload; an entry in row 65 999 and one in row 0 of the last column;
    pair counts on the corner blocks and three random ones against the dense run (no class table: 66 000^2 pairs)"""
    G, S, seed = 66000, 64, 0x5EED0C50
    rng = np.random.default_rng(14)
    X = rng.integers(1, 50000, size=(G, S))
    M, D = _thin(X, seed, force=((65999, S - 1, 7), (0, S - 1, 9)))
    assert M.indices[-1] == 65999 and M.indices[M.indptr[S - 1]] == 0 and M.nnz < 2 ** 21
    Mfull = _csc_of(X, np.ones((G, S), dtype=bool))                            # 4.2 M entries: a chunk crosses the link in pieces of columns
    gid, lev = pkg.encode_groups(pkg.synth.groups(S))
    blocks = [(0, 40, 0, 40), (0, 40, G - 40, G), (G - 40, G, G - 40, G)]
    for _ in range(3):
        i, j = (int(v) for v in rng.integers(0, G - 48, 2))
        blocks.append((i, i + 48, j, j + 48))
    for threads in (None, "0"):
        _setenv(monkeypatch, REO_UPLOAD_THREADS=threads)
        out = []
        for A in (np.asfortranarray(D), M, np.asfortranarray(X), Mfull):
            with pkg.Context(device=0, seed=seed) as ctx:
                ctx.set_matrix(A)
                assert ctx.info()["csc_upload"] == (1 if sp.issparse(A) else 0)
                ctx.set_groups(gid, 2)
                out.append(([ctx.pair_counts(*b) for b in blocks], ctx.info()["upload_link_bytes"]))
        for dense, sparse, A in ((out[0], out[1], M), (out[2], out[3], Mfull)):
            assert sparse[1] == 8 * (S + 1) + A.nnz * (12 if threads == "0" else 8)   # 32-bit row indices + I32 values
            for (g0, e0), (g1, e1) in zip(dense[0], sparse[0]):
                assert np.array_equal(g0, g1) and np.array_equal(e0, e1)
        assert out[1][1] < out[0][1]


def test_infinities_and_nan(pkg, monkeypatch):
    _setenv(monkeypatch)
    G, S, seed = 300, 41, 0x5EED0C60
    X = pkg.synth.float_expr(G, S, seed)
    group = pkg.synth.groups(S)
    ref0 = pkg.synth.ref_mask(G, 60, seed)
    M, D = _thin(X, seed)
    for s, v in ((2, np.inf), (2, -np.inf), (30, np.inf), (40, -np.inf), (40, np.inf)):    # stored +-Inf (two pairs share a column)
        at = M.indptr[s] + (0 if v > 0 else 1)
        M.data[at] = v; D[M.indices[at], s] = v
    for order in ("groups_first", "matrix_first"):
        for Ms, Ds in ((M, D), (M.astype(np.float32), D.astype(np.float32))):
            want = _run(pkg, np.asfortranarray(Ds), group, seed, order, ref0)
            _same(want, _run(pkg, Ms, group, seed, order, ref0), ("inf", order, Ds.dtype))
    # a stored NaN is refused by the call that reads the values: set_matrix when the groups are known, build_pairs otherwise
    Mn, _ = _thin(X, seed)
    Mn.data[Mn.indptr[5] + 1] = np.nan
    gid, lev = pkg.encode_groups(group)
    for A in (Mn, Mn.astype(np.float32)):
        with pkg.Context(device=0, seed=seed) as ctx:
            ctx.set_groups(gid, 2); ctx.compute_thresholds(0.01)
            with pytest.raises(pkg.DimensionMismatch, match="contains NaN") as e:
                ctx.set_matrix(A)
            assert e.value.status == pkg._ffi.REO_EINVAL
        with pkg.Context(device=0, seed=seed) as ctx:
            ctx.set_matrix(A)
            assert ctx.info()["csc_upload"] == 1
            ctx.set_groups(gid, 2); ctx.compute_thresholds(0.01)
            with pytest.raises(pkg.DimensionMismatch, match="contains NaN"):
                ctx.build_pairs(0)


def test_arguments(pkg, monkeypatch):
    """every faulty container is REO_EINVAL with a message that names the fault, and the same context then runs a good matrix"""
    L = pkg._ffi.lib()
    G, S, seed = 300, 24, 0x5EED0C70
    M, D = _thin(pkg.synth.t1_counts(G, S, seed), seed)
    group = pkg.synth.groups(S)
    gid, lev = pkg.encode_groups(group)
    ref0 = pkg.synth.ref_mask(G, 60, seed)
    _setenv(monkeypatch)
    want = _run(pkg, np.asfortranarray(D), group, seed, "groups_first", ref0)
    colptr, rowidx = M.indptr.astype(np.int64), M.indices.astype(np.int32)
    starts_at_1 = colptr.copy(); starts_at_1[0] = 1
    decreasing = colptr.copy(); decreasing[10] = decreasing[9] - 1
    row_G = rowidx.copy(); row_G[colptr[7] + 2] = G
    repeated = rowidx.copy(); repeated[colptr[3] + 1] = repeated[colptr[3]]                  # (column 2 is full: 300 entries)
    for name, dtype in (("i64", np.int64), ("f64", np.float64), ("f32", np.float32), ("i32", np.int32)):
        fn = getattr(L, "reo_set_matrix_csc_" + name)
        val = M.data.astype(dtype)
        for threads, groups_first in ((None, True), ("0", True), (None, False)):
            _setenv(monkeypatch, REO_UPLOAD_THREADS=threads)
            with pkg.Context(device=0, seed=seed) as ctx:
                if groups_first:
                    ctx.set_groups(gid, 2); ctx.compute_thresholds(0.01)
                for (g, s, cp, ri, va), words in (((G, S, starts_at_1, rowidx, val), ("colptr", "start at 0")),
                                                  ((G, S, decreasing, rowidx, val), ("colptr", "non-decreasing", "column 9")),
                                                  ((G, S, colptr, row_G, val), ("row index", "outside [0,300)")),
                                                  ((G, S, colptr, repeated, val), ("strictly increasing",)),
                                                  ((G, S, colptr, rowidx, None), ("val is null",)),
                                                  ((1, S, colptr, rowidx, val), ("1 x",)), ((G, 1, colptr, rowidx, val), ("x 1",))):
                    rc = fn(ctx._h, g, s, cp.ctypes.data, ri.ctypes.data, ctypes.c_void_p(va.ctypes.data if va is not None else None))
                    assert rc == pkg._ffi.REO_EINVAL, (name, words)
                    msg = L.reo_last_error().decode()
                    assert msg and all(w in msg for w in words), (name, words, msg)
                # the context is still usable
                pkg._ffi.check(fn(ctx._h, G, S, colptr.ctypes.data, rowidx.ctypes.data, val.ctypes.data))
                ctx.G, ctx.S = G, S
                assert ctx.info()["csc_upload"] == 1 and ctx.info()["csc_nnz"] == M.nnz
                if not groups_first:
                    ctx.set_groups(gid, 2); ctx.compute_thresholds(0.01)
                ctx.build_pairs(0)
                assert np.array_equal(ctx.get_codes(0, G, 0, G), want["per_k"][0][0]), name
                if name in ("i64", "i32"):
                    assert np.array_equal(ctx.tally(ref0), want["per_k"][0][1])


def test_against_the_oracle(pkg, oracle, monkeypatch):
    """not only self-referential: G = 300, S = 40 counts at 10 % density against oracle.build_codes / tally / iterate on the densified matrix"""
    _setenv(monkeypatch)
    G, S, seed = 300, 40, 0x5EED0C80
    M, D = _thin(pkg.synth.t1_counts(G, S, seed), seed)
    gid, lev = pkg.encode_groups(pkg.synth.groups(S))
    ref0 = pkg.synth.ref_mask(G, 60, seed)
    for order in ("matrix_first", "groups_first"):
        with pkg.Context(device=0, seed=seed) as ctx:
            if order == "matrix_first": ctx.set_matrix(M)
            ctx.set_groups(gid, 2); ctx.compute_thresholds(0.01)
            if order != "matrix_first": ctx.set_matrix(M)
            assert ctx.info()["csc_upload"] == 1 and ctx.info()["csc_nnz"] == M.nnz
            ctx.build_pairs(0)
            thr = ctx.get_thresholds()[:, 0]
            code = oracle.build_codes(D.astype(np.float64), gid, 2, 0, thr, seed)
            assert np.array_equal(ctx.get_codes(0, G, 0, G), code)
            assert np.array_equal(ctx.tally(ref0), oracle.tally(code, ref0))
            res, it, tr = ctx.identify_degs(ref0, 1.0, 0.05, 4, 5)
            exp, eit, etr = oracle.iterate(code, ref0, 1.0, 0.05, 4, 5)
            assert it == eit and tr == etr
            assert np.array_equal(res[:, 2:11], exp[:, 2:11])
            assert np.allclose(res[:, :2], exp[:, :2], rtol=0, atol=P_ATOL)
            assert np.allclose(res[:, 11:], exp[:, 11:], rtol=STAT_RTOL, atol=1e-9)


def test_two_shards_on_one_device(pkg, monkeypatch):
    _setenv(monkeypatch)
    monkeypatch.setenv("REO_MULTI_ONE_DEVICE", "1")
    G, S, seed = 3300, 72, 0x5EED0C90
    M, D = _thin(pkg.synth.float_expr(G, S, seed).astype(np.float32), seed)
    group = pkg.synth.groups(S)
    ref0 = pkg.synth.ref_mask(G, 700, seed)
    for order in ("matrix_first", "groups_first"):
        want = _run(pkg, np.asfortranarray(D), group, seed, order, ref0)
        _same(want, _run(pkg, M, group, seed, order, ref0), ("one context", order))
        _same(want, _run(pkg, M, group, seed, order, ref0, n_gpus=2), ("two shards", order))


def test_second_matrix_on_the_same_context(pkg, monkeypatch):
    """sparse, then dense of another shape and type, then sparse again (and the other way round)"""
    _setenv(monkeypatch)
    seed = 0x5EED0CA0
    A, DA = _thin(pkg.synth.t1_counts(500, 41, seed), seed)
    B = np.asfortranarray(pkg.synth.float_expr(333, 50, seed + 1))
    refA, refB = pkg.synth.ref_mask(500, 100, seed), pkg.synth.ref_mask(333, 60, seed)
    wantA = _run(pkg, np.asfortranarray(DA), pkg.synth.groups(41), seed, "groups_first", refA)
    wantB = _run(pkg, B, pkg.synth.groups(50), seed, "groups_first", refB)
    for first in ("csc", "dense"):
        with pkg.Context(device=0, seed=seed) as ctx:
            for which in (first, "dense" if first == "csc" else "csc", first):
                X, S, ref, want = (A, 41, refA, wantA) if which == "csc" else (B, 50, refB, wantB)
                gid, lev = pkg.encode_groups(pkg.synth.groups(S))
                ctx.set_groups(gid, 2); ctx.compute_thresholds(0.01)
                ctx.set_matrix(X)
                info = ctx.info()
                assert (info["csc_upload"], info["csc_nnz"]) == ((1, A.nnz) if which == "csc" else (0, 0))
                ctx.build_pairs(0)
                G = X.shape[0]
                assert np.array_equal(ctx.get_codes(0, G, 0, G), want["per_k"][0][0]), (first, which)
                assert np.array_equal(ctx.tally(ref), want["per_k"][0][1]), (first, which)
                r = ctx.identify_degs(ref, 1.0, 0.05, 6, 0)
                assert r[1] == want["per_k"][0][2][1] and np.array_equal(r[0], want["per_k"][0][2][0], equal_nan=True)


def test_public_call(pkg, monkeypatch):
    """pkg.identify_degs on a csr_matrix equals pkg.identify_degs on its toarray() and leaves the matrix as it was"""
    _setenv(monkeypatch)
    G, S, seed = 900, 41, 0x5EED0CB0
    group = pkg.synth.groups(S)
    names = [f"g{i}" for i in range(G)]
    ref0 = pkg.synth.ref_mask(G, 150, seed)
    for X in (pkg.synth.t1_counts(G, S, seed), pkg.synth.float_expr(G, S, seed).astype(np.float32)):
        Mc, D = _thin(X, seed)
        M = Mc.tocsr()
        before = (M.data.tobytes(), M.indices.tobytes(), M.indptr.tobytes())
        run = pkg.run_identify_degs(M, group, names, 0.01, 1.0, 0.05, ref0, 6, 1, seed=seed, device=0)
        assert run.info["csc_upload"] == 1 and run.info["csc_nnz"] == M.nnz
        a = pkg.identify_degs(M, group, names, 0.01, 1.0, 0.05, ref0, 6, 1, seed=seed)
        b = pkg.identify_degs(M.toarray(), group, names, 0.01, 1.0, 0.05, ref0, 6, 1, seed=seed)
        assert a.shape == b.shape == (G, 17) and list(a[:, 0]) == list(b[:, 0]) and list(a[:, 16]) == list(b[:, 16])
        assert np.array_equal(a[:, 1:16].astype(np.float64), b[:, 1:16].astype(np.float64), equal_nan=True)
        assert np.array_equal(run.result, a[:, 1:16].astype(np.float64), equal_nan=True)
        assert (M.data.tobytes(), M.indices.tobytes(), M.indptr.tobytes()) == before and M.format == "csr"
