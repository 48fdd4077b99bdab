"""Cases for the sample counts (reo_sample_counts): the numpy restatement of the per-sample comparator and of the partner selection.  No
fixtures, no GPU.

For one sample (a column x of the matrix) and a query gene i, every other gene j is in exactly one of three states: i above j, tied, i below
j.  The rule is that of the matrix's element type (include/reo_hip.h):
  float64   tied when abs(x_i - x_j) < 0.1 in Float64 arithmetic, else x_i > x_j;
  float32   tied when abs(x_i - x_j), formed in Float32, widened, is < 0.1 (tests/float32_cases.py, f32_ties);
  int64     tied when equal (Int32 matrices are widened: the same rule);
  infinities: abs(Inf - Inf) is NaN, not < 0.1, so equal infinities are not tied; the rank rule places them in gene
            order, the gene with the larger index above.  An infinity against anything else compares as usual.
The partner set of a query comes from a row of class codes (Context.get_codes, 255 on the diagonal), the partner mask and the class mask,
as tests/test_gpu_pair_list.py selects it.
"""
from __future__ import annotations

import numpy as np

from float32_cases import f32_ties


def sample_states(x: np.ndarray, i: int):
    """(gt, eq) of gene i against every gene of one sample x (1-D, float64 / float32 / int64): bool arrays over j; the entry j = i is
    meaningless (the diagonal is no pair)."""
    x = np.asarray(x)
    G = x.size
    if x.dtype == np.float32:
        eq = f32_ties(x)[i]
    elif x.dtype == np.float64:
        with np.errstate(invalid="ignore"):
            eq = np.abs(x[i] - x) < 0.1
    else:
        assert x.dtype == np.int64, x.dtype
        eq = x == x[i]
    gt = (x[i] > x) & ~eq
    if x.dtype.kind == "f" and np.isinf(x[i]):
        gt |= (x == x[i]) & (np.arange(G) < i)   # equal infinities: the larger index is the greater one, nothing is tied
    return gt, eq


def selection(code_row: np.ndarray, class_mask: int, partner_mask) -> np.ndarray:
    """bool over j: the partners that reo_pair_list lists for a row of class codes (255 on the diagonal)"""
    c = code_row.astype(np.int64)
    sel = (c < 9) & np.asarray(partner_mask, dtype=bool)
    sel[sel] = ((class_mask >> c[sel]) & 1) == 1
    return sel


def states(X: np.ndarray, genes):
    """(gt, eq), bool arrays queries x genes x samples: sample_states of every query gene in every column of X"""
    X = np.asarray(X)
    G, S = X.shape
    genes = np.asarray(genes, dtype=np.int64).reshape(-1)
    gt = np.zeros((genes.size, G, S), dtype=bool)
    eq = np.zeros((genes.size, G, S), dtype=bool)
    for s in range(S):
        x = np.ascontiguousarray(X[:, s])
        for q, i in enumerate(genes):
            gt[q, :, s], eq[q, :, s] = sample_states(x, int(i))
    return gt, eq


def counts_of(gt: np.ndarray, eq: np.ndarray, sel: np.ndarray):
    """(n_sel, n_gt, n_eq), int32, of the states above under a selection (bool, queries x genes)"""
    n_gt = np.einsum("qjs,qj->qs", gt.astype(np.int32), sel.astype(np.int32))
    n_eq = np.einsum("qjs,qj->qs", eq.astype(np.int32), sel.astype(np.int32))
    return sel.sum(axis=1).astype(np.int32), n_gt.astype(np.int32), n_eq.astype(np.int32)


def expected_counts(X: np.ndarray, codes_of_row, genes, class_mask: int, partner_mask, st=None):
    """(n_sel, n_gt, n_eq) as reo_sample_counts defines them, int32: codes_of_row(i) is row i of get_codes; columns in X's own order.
    st: states(X, genes), when the caller has them already."""
    genes = np.asarray(genes, dtype=np.int64).reshape(-1)
    gt, eq = st if st is not None else states(X, genes)
    sel = np.stack([selection(codes_of_row(int(i)), class_mask, partner_mask) for i in genes])
    assert not sel[np.arange(genes.size), genes].any()
    return counts_of(gt, eq, sel)


def plane_case_data(G, marks, seed, X=None, S=8):
    """the matrix and partner mask of the plane-layout cases (tests/test_gpu_sample_counts.py, plane_case): Int64 below 30 000, Fortran
    order, unless X is given; 1 000 random partners and `marks`"""
    rng = np.random.default_rng(seed)
    if X is None:
        X = np.asfortranarray(rng.integers(0, 30000, size=(G, S)).astype(np.int64))
    pm = np.zeros(G, dtype=bool)
    pm[rng.choice(G, 1000, replace=False)] = True
    pm[list(marks)] = True
    return X, pm
