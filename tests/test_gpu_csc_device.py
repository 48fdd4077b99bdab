"""Sparse matrices that already live on the GPU (reo_set_matrix_csc_dev_*, reo_set_matrix_pseudobulk_csc_dev_* / _dense_dev_*): index arrays
checked by a kernel, then t_csc_columns / pb_csc / pb_dense straight from the caller's device arrays.  The yardstick in every case is the
host entry on the same values in the same process (reo_set_matrix_csc_* on the scipy matrix, Context.pseudobulk on the scipy / numpy
cells; those are pinned against the oracle and numpy by test_gpu_csc.py and test_gpu_cells.py): everything must be equal bit for bit.
Every device run asserts info()["csc_device"] (or calls the _dev symbol itself), so nothing passes by a quiet trip through the host."""
import ctypes
import importlib

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KINDS = ("f64", "i64", "f32", "i32")
NP = {"f64": np.float64, "i64": np.int64, "f32": np.float32, "i32": np.int32}
WIDE = {"f64": np.float64, "i64": np.int64, "f32": np.float64, "i32": np.int64}   # what float32 / int32 CELLS are summed in
T = 2048           # kCscTile of csrc/transform.hip: the gene rows of one workgroup's tile
PB_ROWS = 16384    # kPbRows of csrc/pseudobulk.hip


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.asfortranarray(a).tobytes(order="F") == np.asfortranarray(b).tobytes(order="F")


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
    X = pkg.synth.t1_counts(G, S, seed) if kind in ("i64", "i32") else pkg.synth.float_expr(G, S, seed)
    return X.astype(NP[kind])


def _arrays(M, bits):
    """the three arrays of a scipy CSC / CSR matrix as device tensors, indices of the given width"""
    import torch
    idx = np.int32 if bits == 32 else np.int64
    return (torch.from_numpy(M.indptr.astype(idx)).to(DEV), torch.from_numpy(M.indices.astype(idx)).to(DEV),
            torch.from_numpy(np.ascontiguousarray(M.data)).to(DEV))


def _tensor(M, bits):
    """(sparse_csc tensor on the device that shares the three arrays, the three arrays)"""
    import torch
    cp, ri, va = _arrays(M, bits)
    t = torch.sparse_csc_tensor(cp, ri, va, size=M.shape)
    assert t.ccol_indices().data_ptr() == cp.data_ptr() and t.row_indices().data_ptr() == ri.data_ptr() and (va.numel() == 0 or t.values().data_ptr() == va.data_ptr())
    return t, (cp, ri, va)


def _run(pkg, X, group, seed, order, ref0, degs=True):
    """codes, tally, identify_degs, has_ties per comparison and the resident matrix of one context; X: a scipy matrix (the host CSC entry)
    or a device sparse tensor (the device CSC entry)"""
    gid, lev = pkg.encode_groups(group)
    G = X.shape[0]
    on_device = pkg._ffi.is_device_sparse(X)
    with pkg.Context(device=0, seed=seed) as ctx:
        put = ctx.set_matrix_tensor if on_device else ctx.set_matrix
        if order == "matrix_first":
            put(X)
        ctx.set_groups(gid, len(lev)); ctx.compute_thresholds(0.01)
        if order != "matrix_first":
            put(X)
        info = ctx.info()
        out = dict(info=info, matrix=ctx.get_matrix(), per_k=[])
        for k in range(1 if len(lev) == 2 else len(lev)):
            ctx.build_pairs(k)
            code = ctx.get_codes(0, G, 0, G)
            tal = ctx.tally(ref0)
            deg = ctx.identify_degs(ref0, 1.0, 0.05, 6, 0) if degs else None
            out["per_k"].append((code, tal, deg, ctx.info()["has_ties"]))
    return out


def _same(a, b, what):
    assert len(a["per_k"]) == len(b["per_k"])
    for (c0, t0, d0, h0), (c1, t1, d1, h1) in zip(a["per_k"], b["per_k"]):
        assert np.array_equal(c0, c1), (what, "class table")
        assert h0 == h1, (what, "has_ties")
        assert np.array_equal(t0, t1), (what, "tallies")
        if d0 is not None:
            assert d0[1] == d1[1] and d0[2] == d1[2], (what, "iterations / trace")
            assert np.array_equal(d0[0], d1[0], equal_nan=True), (what, "statistics")
    assert same_bits(a["matrix"], b["matrix"]), (what, "resident matrix")        # bytes: the sign of a stored -0.0 counts


# ---- dense parity -------------------------------------------------------------------------------------------------------------------

_YARD = {}


def _parity_case(pkg, kind, G):
    """the thinned matrix of (kind, G) and the host entry's results for both call orders, computed once"""
    if (kind, G) not in _YARD:
        S, seed = 41, 0x5EED0D00 + G
        force = ((G // 2, 5, -0.0),) if kind in ("f64", "f32") else ()
        M, D = _thin(_data(pkg, kind, G, S, seed), seed, force=force)
        if force:
            at = M.indptr[5] + int(np.searchsorted(M.indices[M.indptr[5]:M.indptr[6]], G // 2))
            assert M.data[at] == 0 and np.signbit(M.data[at])                    # a stored -0.0
        group = pkg.synth.groups(S)
        ref0 = np.arange(G) % 3 != 1 if G < 10 else pkg.synth.ref_mask(G, max(2, G // 5), seed)
        want = {order: _run(pkg, M, group, seed, order, ref0, degs=G >= 10) for order in ("matrix_first", "groups_first")}
        for w in want.values():
            assert w["info"]["csc_upload"] == 1 and w["info"]["csc_device"] == 0
        _YARD[(kind, G)] = (M, group, seed, ref0, want)
    return _YARD[(kind, G)]


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("G", [2, 63, T - 1, T, T + 1])
@pytest.mark.parametrize("kind", KINDS)
def test_device_csc_equals_the_host_csc_entry(pkg, kind, G, bits):
    """G below, at and on both sides of t_csc_columns' row tile, S = 41; an empty and a full column, an all-zero gene row, stored zeros and
    a stored -0.0; both index widths, both call orders; the caller's three tensors are left as they were"""
    import torch
    M, group, seed, ref0, want = _parity_case(pkg, kind, G)
    for order in ("matrix_first", "groups_first"):
        t, arrays = _tensor(M, bits)
        before = [a.clone() for a in arrays]
        got = _run(pkg, t, group, seed, order, ref0, degs=G >= 10)
        info = got["info"]
        assert info["csc_device"] == 1 and info["csc_nnz"] == M.nnz and info["csc_upload"] == 0 and info["upload_link_bytes"] == 0
        assert info["resident_dtype"] == {"f64": 1, "i64": 2, "f32": 3, "i32": 2}[kind] and (info["G"], info["S"]) == M.shape
        _same(want[order], got, (kind, G, bits, order))
        torch.cuda.synchronize()
        for a, b in zip(arrays, before):
            assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8) if a.numel() else a, b.view(torch.uint8) if b.numel() else b)


def test_other_set_matrix_calls_reset_the_device_slot(pkg):
    M, group, seed, ref0, want = _parity_case(pkg, "i64", 63)
    t, _ = _tensor(M, 64)
    with pkg.Context(device=0, seed=seed) as ctx:
        ctx.set_matrix_tensor(t)
        assert (ctx.info()["csc_device"], ctx.info()["csc_nnz"]) == (1, M.nnz)
        ctx.set_matrix(M)
        assert (ctx.info()["csc_device"], ctx.info()["csc_upload"]) == (0, 1)
        ctx.set_matrix_tensor(t)
        ctx.set_matrix(np.asfortranarray(M.toarray()))
        assert (ctx.info()["csc_device"], ctx.info()["csc_nnz"]) == (0, 0)
        ctx.set_matrix_tensor(t)
        ctx.set_matrix_pseudobulk(M, np.arange(41, dtype=np.int32), np.array([0, 20, 41], dtype=np.int32))
        assert (ctx.info()["csc_device"], ctx.info()["csc_nnz"]) == (0, 0)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [32, 64])
def test_faulty_containers_are_refused_and_the_context_lives_on(pkg, bits):
    """G = 63, S = 5, arrays sized exactly: every fault is REO_EINVAL with a message that names its class, the context then holds no
    matrix, and a valid call on the same context gives the host entry's table"""
    import torch
    L = pkg._ffi.lib()
    G, S, seed = 63, 5, 0x5EED0D10
    M, D = _thin(pkg.synth.t1_counts(G, S, seed), seed, density=0.3)
    group = ["u", "u", "v", "v", "v"]
    gid, lev = pkg.encode_groups(group)
    ref0 = pkg.synth.ref_mask(G, 12, seed)
    want = _run(pkg, M, group, seed, "groups_first", ref0)
    cp, ri, va = _arrays(M, bits)
    nnz = M.nnz
    c = [int(v) for v in M.indptr]
    assert c[1] == c[2] and c[3] - c[2] == G and c[4] - c[3] >= 3 and c[5] - c[4] >= 1 and ri.numel() == nnz and cp.numel() == S + 1

    def put(t, i, v):
        t = t.clone(); t[i] = v
        return t
    swapped = ri.clone(); swapped[c[3]], swapped[c[3] + 1] = ri[c[3] + 1], ri[c[3]]
    cases = [  # (colptr, rowidx, values, nnz argument, index_bits, words of the message)
        (cp, put(ri, c[3] + 1, G), va, nnz, bits, ("row index", "column 3", "outside [0,63)")),
        (cp, put(ri, c[4], -1), va, nnz, bits, ("row index", "column 4", "outside [0,63)")),
        (cp, put(ri, c[3] + 1, int(ri[c[3]])), va, nnz, bits, ("column 3", "not strictly increasing")),
        (cp, swapped, va, nnz, bits, ("column 3", "not strictly increasing")),
        (put(cp, 0, 1), ri, va, nnz, bits, ("colptr", "column 0", "start at 0")),
        (put(cp, 4, c[3] - 1), ri, va, nnz, bits, ("colptr", "column 3", "non-decreasing")),
        (put(cp, S, nnz + 5), ri, va, nnz, bits, ("colptr", "column 4", "nnz")),
        (put(cp, 3, c[3] + 1), ri, va, nnz, bits, ("colptr", "column 2", "more than G = 63")),
        (cp, ri, va, nnz - 1, bits, ("colptr", "column 4", "end at nnz")),
        (cp, ri, va, nnz, 16, ("index_bits",)),
        (cp, ri, None, nnz, bits, ("val is null",)),
    ]
    fn = L.reo_set_matrix_csc_dev_i64
    ptr = lambda t: ctypes.c_void_p(int(t.data_ptr())) if t is not None else None
    with pkg.Context(device=0, seed=seed) as ctx:
        ctx.set_groups(gid, 2); ctx.compute_thresholds(0.01)
        for cpx, rix, vax, n, b, words in cases:
            rc = fn(ctx._h, G, S, n, ptr(cpx), ptr(rix), b, ptr(vax))
            msg = L.reo_last_error().decode()
            assert rc == pkg._ffi.REO_EINVAL, (words, rc, msg)
            assert msg and all(w in msg for w in words), (words, msg)
            assert ctx.info()["resident_dtype"] == 0 and ctx.info()["csc_device"] == 0
            with pytest.raises(pkg.DimensionMismatch, match="no expression matrix set"):
                ctx.build_pairs(0)
            pkg._ffi.check(fn(ctx._h, G, S, nnz, ptr(cp), ptr(ri), bits, ptr(va)))          # ... and the context is usable
            assert ctx.info()["csc_device"] == 1
            ctx.build_pairs(0)
            assert np.array_equal(ctx.get_codes(0, G, 0, G), want["per_k"][0][0]), words
        torch.cuda.synchronize()
    assert torch.equal(cp.cpu(), torch.from_numpy(M.indptr.astype(np.int32 if bits == 32 else np.int64)))


def test_multi_context_refuses_the_device_entries(pkg, monkeypatch):
    import torch
    monkeypatch.setenv("REO_MULTI_ONE_DEVICE", "1")
    M, group, seed, ref0, want = _parity_case(pkg, "i64", 63)
    t, _ = _tensor(M, 64)
    X = np.asfortranarray(M.toarray())
    order, ptr = np.arange(41, dtype=np.int32), np.array([0, 20, 41], dtype=np.int32)
    with pkg.Context(seed=1, n_gpus=2) as ctx:
        ctx.set_matrix(X)
        for call in (lambda: ctx.set_matrix_tensor(t), lambda: ctx.set_matrix_pseudobulk(t, order, ptr),
                     lambda: ctx.set_matrix_pseudobulk(torch.from_numpy(X).to(DEV), order, ptr)):
            with pytest.raises(pkg.DimensionMismatch) as e:
                call()
            assert "reo_create_multi" in e.value.message
        assert same_bits(ctx.get_matrix(), X)                                     # the matrix it had is still there


# ---- pseudo-bulk from device cells -------------------------------------------------------------------------------------------------

PB_C = 37
_PB = {}


def _pb_case(pkg, kind, G):
    """G genes x 37 cells at about 3 %: cell 11 full (at G = 16 385 more than kPbPer x kPbThreads = 2 048 entries: pb_csc's slow loop), cell
    23 empty, entries on rows 16 383 and 16 384 (both sides of the kPbRows tile border); 6 profiles of 1, 3, 4, 5, 0 and 9 cells (the edges
    of kPbDepth = 4) over a permutation that leaves 15 cells out; the host entry's sums, computed once"""
    if (kind, G) not in _PB:
        rng = np.random.default_rng(0x5EED0D20 + G)
        X = _data(pkg, kind, G, PB_C, 0x5EED0D20 + G)
        if kind in ("i64", "i32"):
            X = X + 1                                                           # (no accidental zeros: the fill decides what is stored)
        fill = rng.random((G, PB_C)) < 0.03
        fill[:, 11] = True
        fill[:, 23] = False
        if G > PB_ROWS:
            fill[PB_ROWS - 1:PB_ROWS + 1, 7] = True
        D = np.where(fill, X, np.zeros((), dtype=X.dtype)).astype(NP[kind])
        M = _csc_of(D, fill)
        others = [c for c in rng.permutation(PB_C) if c not in (11, 23, 7)]
        order = np.array([11] + others[:2] + [23] + others[2:4] + [7] + others[4:19], dtype=np.int32)
        ptr = np.array([0, 1, 4, 8, 13, 13, 22], dtype=np.int32)
        assert order.size == 22 == len(set(order.tolist())) and np.diff(ptr).tolist() == [1, 3, 4, 5, 0, 9]
        with pkg.Context(device=0, seed=1) as ctx:
            host = ctx.pseudobulk(M, order, ptr)
            host_dense = ctx.pseudobulk(D, order, ptr)
        exp = np.zeros((G, 6), dtype=WIDE[kind])
        for o in range(6):
            for c in order[ptr[o]:ptr[o + 1]]:
                exp[:, o] = exp[:, o] + D[:, c].astype(WIDE[kind])               # left to right, as the reference sums (:63)
        assert same_bits(host, np.asfortranarray(exp)) and same_bits(host_dense, host)
        _PB[(kind, G)] = (M, D, order, ptr, host)
    return _PB[(kind, G)]


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("G", [63, PB_ROWS + 1])
@pytest.mark.parametrize("kind", KINDS)
def test_pseudobulk_from_a_device_csc_tensor(pkg, kind, G, bits):
    import torch
    M, D, order, ptr, host = _pb_case(pkg, kind, G)
    if G > PB_ROWS:
        assert int(np.diff(M.indptr).max()) > 2 * 1024
    t, arrays = _tensor(M, bits)
    before = [a.clone() for a in arrays]
    with pkg.Context(device=0, seed=1) as ctx:
        ctx.set_matrix_pseudobulk(t, order, ptr)
        info = ctx.info()
        got = ctx.get_matrix()
        assert (info["G"], info["S"], info["resident_dtype"]) == (G, 6, 2 if kind in ("i64", "i32") else 1) and (ctx.G, ctx.S) == (G, 6)
        assert (info["upload_link_bytes"], info["csc_upload"], info["csc_nnz"], info["csc_device"]) == (0, 0, 0, 0)
    assert same_bits(got, host)
    assert not got[:, 4].any()                                                   # the empty profile
    torch.cuda.synchronize()
    for a, b in zip(arrays, before):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.mark.parametrize("G", [63, 257])
@pytest.mark.parametrize("kind", KINDS)
def test_pseudobulk_from_dense_device_cells_with_a_leading_dimension(pkg, kind, G):
    import torch
    M, D, order, ptr, host = _pb_case(pkg, kind, 63) if G == 63 else (None,) + _dense_case(pkg, kind, G)
    tall = torch.full((PB_C, G + 3), 99, dtype=getattr(torch, np.dtype(NP[kind]).name), device=DEV)   # (a pad that a read past G would add)
    tall[:, :G] = torch.from_numpy(np.ascontiguousarray(D.T)).to(DEV)
    before = tall.clone()
    t = tall[:, :G].t()
    assert t.stride() == (1, G + 3)
    with pkg.Context(device=0, seed=1) as ctx:
        ctx.set_matrix_pseudobulk(t, order, ptr)
        info = ctx.info()
        assert (info["G"], info["S"], info["resident_dtype"]) == (G, 6, 2 if kind in ("i64", "i32") else 1)
        assert same_bits(ctx.get_matrix(), host)
    torch.cuda.synchronize()
    assert torch.equal(tall, before)


def _dense_case(pkg, kind, G):
    """G x 37 dense cells (floats: pkg.synth.float_expr, so the summation order shows) and Context.pseudobulk's sums of the host array"""
    if ("dense", kind, G) not in _PB:
        D = _data(pkg, kind, G, PB_C, 0x5EED0D30 + G)
        _, _, order, ptr, _ = _pb_case(pkg, kind, 63)
        with pkg.Context(device=0, seed=1) as ctx:
            host = ctx.pseudobulk(D, order, ptr)
        _PB[("dense", kind, G)] = (D, order, ptr, host)
    return _PB[("dense", kind, G)]


@pytest.mark.parametrize("fault", ["row_range", "row_order"])
def test_a_bad_cell_matrix_is_refused_and_the_context_holds_no_matrix(pkg, fault):
    import torch
    M, D, order, ptr, host = _pb_case(pkg, "i64", 63)
    cp, ri, va = _arrays(M, 64)
    at = int(M.indptr[11]) + 5                                                   # inside the full cell
    ri = ri.clone()
    ri[at] = 63 if fault == "row_range" else ri[at - 1]
    bad = torch.sparse_csc_tensor(cp, ri, va, size=M.shape)
    with pkg.Context(device=0, seed=1) as ctx:
        ctx.set_matrix(np.asfortranarray(D[:, :20]))
        assert ctx.info()["resident_dtype"] == 2
        with pytest.raises(pkg.DimensionMismatch) as e:
            ctx.set_matrix_pseudobulk(bad, order, ptr)
        assert e.value.status == pkg._ffi.REO_EINVAL and "column 11" in e.value.message
        assert ("outside [0,63)" if fault == "row_range" else "not strictly increasing") in e.value.message
        assert ctx.info()["resident_dtype"] == 0
        with pytest.raises(pkg.DimensionMismatch):
            ctx.get_matrix()
        good, _ = _tensor(M, 64)
        ctx.set_matrix_pseudobulk(good, order, ptr)                              # ... and usable
        assert same_bits(ctx.get_matrix(), host)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------

E2E_G, E2E_C = 300, 400


def e2e_cells(ngroups):
    """300 genes x 400 cells of Poisson counts: gene rates over two decades (rare genes fall to min_features), cell depths over one
    (shallow profiles fall to min_profiles), a third of the genes up in the second group; cells of the groups interleaved"""
    rng = np.random.default_rng(0x5EED0D40 + ngroups)
    labels = [f"grp{t % ngroups}" for t in range(E2E_C)]
    rate = 10.0 ** rng.uniform(-3.0, -0.2, E2E_G)
    depth = 10.0 ** rng.uniform(-0.7, 0.3, E2E_C)
    lam = rate[:, None] * depth[None, :]
    up = rng.random(E2E_G) < 0.33
    second = np.array([l == "grp1" for l in labels])
    lam[np.ix_(up, second)] *= 4.0
    return rng.poisson(lam).astype(np.int64), labels


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


@pytest.mark.parametrize("ngroups", [2, 3])
def test_cells_to_degs_from_device_sparse_tensors(pkg, ngroups):
    import torch
    seed, n_pseudo = 0x5EED0D50, 8
    X, labels = e2e_cells(ngroups)
    R = importlib.import_module(pkg.__name__ + ".reoa")
    order, ptr, names, groups = pkg.cells_partition(labels, n_pseudo, seed)
    pb = R.host_sums(X, order, ptr)                                              # numpy: what the filters will see
    cc = (pb > 0).sum(axis=0)
    mp = int(np.sort(cc)[1])
    gc = (pb[:, cc > mp] > 0).sum(axis=1)
    mf = int(np.sort(gc)[E2E_G // 5])
    pk, gk = cc > mp, gc > mf
    assert 0 < (~pk).sum() and 0 < (~gk).sum() and gk.sum() >= 10 and len({g for g, k in zip(groups, pk) if k}) == ngroups
    gnames = [f"gene{i}" for i in range(E2E_G)]
    ref = pkg.synth.ref_mask(E2E_G, 120, seed ^ 0x77)
    args = (labels, gnames, n_pseudo, 0.01, 1.0, 0.05, ref, 8, 1)
    kw = dict(min_profiles=mp, min_features=mf, seed=seed, device=0)
    want = pkg.identify_degs_cells(sp.csc_matrix(X), *args, **kw)
    assert np.array_equal(want.gene_kept, gk) and np.array_equal(want.profile_kept, pk)
    csc, _ = _tensor(sp.csc_matrix(X), 64)
    cr, co, va = _arrays(sp.csr_matrix(np.ascontiguousarray(X.T)), 32)           # cells x genes, AnnData's orientation
    csr_t = torch.sparse_csr_tensor(cr, co, va, size=(E2E_C, E2E_G)).t()
    assert csr_t.layout == torch.sparse_csc and pkg._ffi.is_device_sparse(csr_t)
    for cells in (csc, csr_t):
        got = pkg.identify_degs_cells(cells, *args, **kw)
        assert np.array_equal(got.gene_kept, want.gene_kept) and np.array_equal(got.profile_kept, want.profile_kept)
        assert got.profile_names == want.profile_names and got.profile_groups == want.profile_groups
        same_run(got.run, want.run)
        assert (got.run.info["G"], got.run.info["S"]) == (int(gk.sum()), int(pk.sum()))
    assert want.run.iters_run >= 1 and len(want.run.comparisons) == (1 if ngroups == 2 else 3)


def test_run_identify_degs_on_a_device_sparse_tensor(pkg):
    G, S, seed = 300, 41, 0x5EED0D60
    names = [f"g{i}" for i in range(G)]
    ref0 = pkg.synth.ref_mask(G, 60, seed)
    for kind, bits, group in (("i64", 64, pkg.synth.groups(S)), ("f32", 32, ["a"] * 12 + ["b"] * 15 + ["c"] * 14)):
        M, D = _thin(_data(pkg, kind, G, S, seed), seed)
        t, _ = _tensor(M, bits)
        want = pkg.run_identify_degs(M, group, names, 0.01, 1.0, 0.05, ref0, 6, 1, seed=seed, device=0)
        got = pkg.run_identify_degs(t, group, names, 0.01, 1.0, 0.05, ref0, 6, 1, seed=seed)
        assert want.info["csc_upload"] == 1 and got.info["csc_device"] == 1 and got.info["csc_nnz"] == M.nnz and got.info["csc_upload"] == 0
        same_run(got, want)
