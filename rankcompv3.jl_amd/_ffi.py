"""ctypes binding of libreo_hip.so (include/reo_hip.h).

There is no CPU fallback: if the shared library is missing or no MI355X is
visible the calls raise, they never route anywhere else.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
from typing import NamedTuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("REO_LIB_PATH") or os.path.join(_HERE, "libreo_hip.so")  # (REO_LIB_PATH: an instrumented build, tools/asan_host.sh)
CSRC = os.path.join(_HERE, "csrc")

REO_OK, REO_EINVAL, REO_EHIP, REO_ECOMM, REO_ENOMEM = 0, -1, -2, -3, -4
NTIMINGS = 12
CALL_BINS = 8192   # kCallBins of csrc/sample_calls.h: ranks per histogram tile of k_call_cut (tests place their rows either side of it)

# every symbol include/reo_hip.h declares
SYMBOLS = [
    "reo_version", "reo_last_error", "reo_create", "reo_destroy", "reo_trim_memory", "reo_set_shard", "reo_set_allreduce", "reo_set_allgather",
    "reo_create_multi", "reo_comm_unique_id", "reo_comm_init_rank",
    "reo_set_matrix_f64", "reo_set_matrix_i64", "reo_set_matrix_dev_f64", "reo_set_matrix_dev_i64",
    "reo_set_matrix_f32", "reo_set_matrix_i32", "reo_set_matrix_dev_f32", "reo_set_matrix_dev_i32",
    "reo_set_matrix_rm_f64", "reo_set_matrix_rm_i64", "reo_set_matrix_rm_f32", "reo_set_matrix_rm_i32",
    "reo_set_matrix_csc_f64", "reo_set_matrix_csc_i64", "reo_set_matrix_csc_f32", "reo_set_matrix_csc_i32",
    "reo_set_groups", "reo_compute_thresholds", "reo_set_thresholds", "reo_get_thresholds", "reo_threshold",
    "reo_build_pairs", "reo_build_pairs_contrast", "reo_pair_counts", "reo_get_codes", "reo_tally", "reo_identify_degs", "reo_mccullagh",
    "reo_set_profiling", "reo_reset_timings", "reo_get_timings", "reo_get_info",
    "reo_pseudobulk_dense_f64", "reo_pseudobulk_dense_i64", "reo_pseudobulk_csc_f64", "reo_pseudobulk_csc_i64",
    "reo_set_matrix_pseudobulk_dense_f64", "reo_set_matrix_pseudobulk_dense_i64", "reo_set_matrix_pseudobulk_csc_f64", "reo_set_matrix_pseudobulk_csc_i64",
    "reo_filter_matrix", "reo_get_matrix", "reo_get_ref_mask", "reo_pair_list", "reo_sample_counts", "reo_pair_support",
    "reo_sample_tests", "reo_sample_calls", "reo_set_valid_mask", "reo_build_pairs_masked", "reo_pair_counts_masked",
    "reo_perm_null", "reo_perm_codes", "reo_rank_shift", "reo_top_pairs", "reo_top_pairs_null", "reo_top_pairs_loo",
    "reo_top_partners", "reo_top_partners_null",
] +[f"reo_set_matrix_{form}_{t}" for form in ("csc_dev", "pseudobulk_csc_dev", "pseudobulk_dense_dev") for t in ("f64", "i64", "f32", "i32")]

ALLREDUCE_FN = ctypes.CFUNCTYPE(ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p)
ALLGATHER_FN = ctypes.CFUNCTYPE(ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p)


class LibraryMissing(RuntimeError):
    """libreo_hip.so has not been built (run __graft_entry__.build())."""


class ReoError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"libreo_hip status {status}: {message}")
        self.status = status
        self.message = message


class DimensionMismatch(ReoError, ValueError):
    """REO_EINVAL: the reference's DimensionMismatch / ArgumentError / BoundsError paths."""


def build_library(force: bool = False) -> str:
    """Compile libreo_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    args = ["make", "-C", CSRC, "-j4"]
    if force:
        args.append("-B")
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    return LIB_PATH


_LIB = None
SIGNATURES = {}   # name -> (restype, argtypes) of every bound entry point, filled by lib()


def lib() -> ctypes.CDLL:
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise LibraryMissing(f"{LIB_PATH} not found: build it with __graft_entry__.build(); there is no CPU fallback")
    try:
        # torch ships its own copy of the HIP runtime; two copies in one process do not share the GPU
        # (the second one reports "no HIP GPUs").  Importing torch first makes libreo_hip.so bind to
        # the copy torch already loaded, so both see the same devices and streams.
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    vp, i32, i64, u64, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_double
    sig = {
        "reo_version": (i32, []),
        "reo_last_error": (ctypes.c_char_p, []),
        "reo_create": (i32, [ctypes.POINTER(vp), i32, u64]),
        "reo_destroy": (None, [vp]),
        "reo_trim_memory": (i32, []),
        "reo_set_shard": (i32, [vp, i32, i32]),
        "reo_create_multi": (i32, [ctypes.POINTER(vp), i32, u64]),
        "reo_comm_unique_id": (i32, [vp]),
        "reo_comm_init_rank": (i32, [vp, vp, i32, i32]),
        "reo_set_allreduce": (i32, [vp, ALLREDUCE_FN, vp]),
        "reo_set_allgather": (i32, [vp, ALLGATHER_FN, vp]),
        "reo_set_matrix_f64": (i32, [vp, vp, i64, i64, i64]),
        "reo_set_matrix_i64": (i32, [vp, vp, i64, i64, i64]),
        "reo_set_matrix_dev_f64": (i32, [vp, vp, i64, i64, i64]),
        "reo_set_matrix_dev_i64": (i32, [vp, vp, i64, i64, i64]),
        "reo_set_matrix_f32": (i32, [vp, vp, i64, i64, i64]),
        "reo_set_matrix_i32": (i32, [vp, vp, i64, i64, i64]),
        "reo_set_matrix_dev_f32": (i32, [vp, vp, i64, i64, i64]),
        "reo_set_matrix_dev_i32": (i32, [vp, vp, i64, i64, i64]),
        "reo_set_matrix_rm_f64": (i32, [vp, vp, i64, i64, i64]),
        "reo_set_matrix_rm_i64": (i32, [vp, vp, i64, i64, i64]),
        "reo_set_matrix_rm_f32": (i32, [vp, vp, i64, i64, i64]),
        "reo_set_matrix_rm_i32": (i32, [vp, vp, i64, i64, i64]),
        "reo_set_matrix_csc_f64": (i32, [vp, i64, i64, vp, vp, vp]),
        "reo_set_matrix_csc_i64": (i32, [vp, i64, i64, vp, vp, vp]),
        "reo_set_matrix_csc_f32": (i32, [vp, i64, i64, vp, vp, vp]),
        "reo_set_matrix_csc_i32": (i32, [vp, i64, i64, vp, vp, vp]),
        "reo_set_groups": (i32, [vp, vp, i64, i32]),
        "reo_compute_thresholds": (i32, [vp, f64]),
        "reo_set_thresholds": (i32, [vp, vp]),
        "reo_get_thresholds": (i32, [vp, vp]),
        "reo_threshold": (i32, [i32, f64]),
        "reo_build_pairs": (i32, [vp, i32]),
        "reo_build_pairs_contrast": (i32, [vp, i32, i32]),
        "reo_pair_counts": (i32, [vp, i64, i64, i64, i64, vp, vp]),
        "reo_get_codes": (i32, [vp, i64, i64, i64, i64, vp]),
        "reo_tally": (i32, [vp, vp, vp]),
        "reo_identify_degs": (i32, [vp, vp, f64, f64, i32, i32, vp, vp, vp]),
        "reo_mccullagh": (i32, [vp, vp, i64, vp]),
        "reo_set_profiling": (i32, [vp, i32]),
        "reo_reset_timings": (i32, [vp]),
        "reo_get_timings": (i32, [vp, vp, i32]),
        "reo_get_info": (i32, [vp, vp, i32]),
        "reo_pseudobulk_dense_f64": (i32, [vp, vp, i64, i64, i64, vp, i64, vp, i32, vp]),
        "reo_pseudobulk_dense_i64": (i32, [vp, vp, i64, i64, i64, vp, i64, vp, i32, vp]),
        "reo_pseudobulk_csc_f64": (i32, [vp, i64, i64, vp, vp, vp, vp, i64, vp, i32, vp]),
        "reo_pseudobulk_csc_i64": (i32, [vp, i64, i64, vp, vp, vp, vp, i64, vp, i32, vp]),
        "reo_set_matrix_pseudobulk_dense_f64": (i32, [vp, vp, i64, i64, i64, vp, i64, vp, i32]),
        "reo_set_matrix_pseudobulk_dense_i64": (i32, [vp, vp, i64, i64, i64, vp, i64, vp, i32]),
        "reo_set_matrix_pseudobulk_csc_f64": (i32, [vp, i64, i64, vp, vp, vp, vp, i64, vp, i32]),
        "reo_set_matrix_pseudobulk_csc_i64": (i32, [vp, i64, i64, vp, vp, vp, vp, i64, vp, i32]),
        "reo_filter_matrix": (i32, [vp, i64, i64, vp, vp, vp, vp]),
        "reo_get_matrix": (i32, [vp, vp, i64]),
        "reo_get_ref_mask": (i32, [vp, vp, vp]),
        "reo_pair_list": (i32, [vp, vp, i64, vp, ctypes.c_uint32, vp, vp, vp, i64]),
        "reo_sample_counts": (i32, [vp, vp, i64, vp, ctypes.c_uint32, vp, vp, vp]),
        "reo_pair_support": (i32, [vp, vp, i64, vp, vp, vp, vp, vp]),
        "reo_sample_tests": (i32, [vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp]),
        "reo_sample_calls": (i32, [vp, vp, i64, vp, f64, f64, vp, vp, vp, vp]),
        "reo_set_valid_mask": (i32, [vp, vp, i64, i64, i64]),
        "reo_build_pairs_masked": (i32, [vp, i32, f64, vp]),
        "reo_pair_counts_masked": (i32, [vp, i64, i64, i64, i64, vp, vp, vp]),
        "reo_perm_null": (i32, [vp, i32, vp, i64, vp, f64, f64, vp, vp, vp, vp, vp, vp]),
        "reo_perm_codes": (i32, [vp, i32, vp, i64, i64, i64, i64, vp]),
        "reo_rank_shift": (i32, [vp, i32, i32, vp]),
        "reo_top_pairs": (i32, [vp, i32, i32, vp, i64, vp, vp, vp, vp, vp, vp]),
        "reo_top_pairs_null": (i32, [vp, i32, i32, vp, i64, vp, vp, i32, vp, vp, vp, vp]),
        "reo_top_pairs_loo": (i32, [vp, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp]),
        "reo_top_partners": (i32, [vp, i32, i32, vp, i64, vp, i32, vp, vp, vp, vp]),
        "reo_top_partners_null": (i32, [vp, i32, i32, vp, i64, vp, i64, vp, vp, vp, vp, vp]),
    }
    for t in ("f64", "i64", "f32", "i32"):   # SPARSE ON THE DEVICE
        sig["reo_set_matrix_csc_dev_" + t] = (i32, [vp, i64, i64, i64, vp, vp, i32, vp])
        sig["reo_set_matrix_pseudobulk_csc_dev_" + t] = (i32, [vp, i64, i64, i64, vp, vp, i32, vp, vp, i64, vp, i32])
        sig["reo_set_matrix_pseudobulk_dense_dev_" + t] = (i32, [vp, vp, i64, i64, i64, vp, i64, vp, i32])
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    global SIGNATURES
    SIGNATURES = sig
    _LIB = L
    return L


def check(status: int) -> None:
    if status == REO_OK:
        return
    msg = lib().reo_last_error().decode("utf-8", "replace")
    if status == REO_EINVAL:
        raise DimensionMismatch(status, msg)
    raise ReoError(status, msg)


def trim_memory() -> None:
    """reo_trim_memory: give the cached device and pinned blocks of destroyed contexts back to the driver (other allocators of the
    process -- PyTorch's -- cannot see what the library's block cache holds; REO_DEVICE_CACHE_MB bounds it)."""
    check(lib().reo_trim_memory())


def threshold(sample_size: int, pval_reo: float = 0.01) -> int:
    """get_major_reo_lower_count (src/RankCompV3.jl:81-92) as the library computes it (host arithmetic)."""
    return int(lib().reo_threshold(int(sample_size), float(pval_reo)))


def _ptr(a: np.ndarray) -> int:
    return a.ctypes.data


def _opt(a):
    return None if a is None else _ptr(a)


def _genes(genes):
    """(pointer, count) of a query's gene (or partner) array: null for None or an empty one."""
    return (_ptr(genes) if genes is not None and genes.size else None, 0 if genes is None else genes.size)


# element types with an entry point of their own; every other integer type (and bool) goes to Int64, every other float type to Float64
_NATIVE = {np.dtype(np.float64): "f64", np.dtype(np.int64): "i64", np.dtype(np.float32): "f32", np.dtype(np.int32): "i32"}


def matrix_entry(X):
    """(symbol name, array, ld) for a host expression matrix (genes x samples): which reo_set_matrix_* takes it, the column-major array
    that is handed over and its leading dimension in elements.  Pure: no library, no GPU.  A column-major array (or view with
    ld >= G, like a Julia view of rows of a taller matrix) of Float64 / Int64 / Float32 / Int32 is passed as it is, WITHOUT a copy; a
    Float32 matrix is then compared in Float32 arithmetic, as the reference compares a Matrix{Float32} (X.astype(np.float64) asks for
    the Float64 rule).  Narrower integers and bool are converted to Int64, every other float type to Float64, on the host."""
    X = np.asarray(X)
    if X.ndim != 2:
        raise DimensionMismatch(REO_EINVAL, "expression matrix must be 2-D (genes x samples)")
    if X.dtype in _NATIVE:
        want = X.dtype
    else:
        want = np.dtype(np.int64) if (np.issubdtype(X.dtype, np.integer) or X.dtype == np.bool_) else np.dtype(np.float64)
    G, S = X.shape
    sz = want.itemsize
    if X.dtype == want and G > 0 and S > 1 and X.strides[0] == sz and X.strides[1] % sz == 0 and X.strides[1] >= sz * G:
        Xf, ld = X, X.strides[1] // sz
    else:
        Xf = np.asfortranarray(X, dtype=want)
        ld = max(G, 1)
    return "reo_set_matrix_" + _NATIVE[want], Xf, ld


def host_matrix_entry(X):
    """(symbol name, array, ld) for a host expression matrix in EITHER layout: matrix_entry's answer for a column-major array, and for a
    row-major one -- numpy's default -- a reo_set_matrix_rm_* symbol, the array ITSELF and its row pitch in elements: a 2-D array of
    Float64 / Int64 / Float32 / Int32 with strides (ld * itemsize, itemsize), ld >= S (C-contiguous, or a column slice of a wider
    C-ordered array) is read in place, without the transposing host copy of np.asfortranarray; the library transposes on the device.
    Column-major wins where both descriptions hold.  A C-contiguous array of another dtype is cast in C order (the casts of matrix_entry)
    and routed row-major; every other stride pattern goes through matrix_entry.  The route is OPT-IN until tools/rowmajor_ab.py has been
    run on the GPU host: REO_ROWMAJOR=1 in the environment (read per call) takes it; unset or 0, everything goes
    through matrix_entry as before.  Pure: no library, no GPU."""
    if os.environ.get("REO_ROWMAJOR", "0") != "1":
        return matrix_entry(X)
    X = np.asarray(X)
    if X.ndim != 2:
        raise DimensionMismatch(REO_EINVAL, "expression matrix must be 2-D (genes x samples)")
    G, S = X.shape
    if G < 1 or S < 2:
        return matrix_entry(X)
    if X.dtype in _NATIVE:
        sz = X.dtype.itemsize
        if X.strides[0] == sz and X.strides[1] % sz == 0 and X.strides[1] >= sz * G:
            return matrix_entry(X)   # column-major as it is
        if X.strides[1] == sz and X.strides[0] % sz == 0 and X.strides[0] >= sz * S:
            return "reo_set_matrix_rm_" + _NATIVE[X.dtype], X, X.strides[0] // sz
        return matrix_entry(X)
    if X.flags.c_contiguous and not X.flags.f_contiguous:
        want = np.dtype(np.int64) if (np.issubdtype(X.dtype, np.integer) or X.dtype == np.bool_) else np.dtype(np.float64)
        return "reo_set_matrix_rm_" + _NATIVE[want], np.ascontiguousarray(X, dtype=want), S
    return matrix_entry(X)


def is_sparse(X) -> bool:
    """A scipy.sparse matrix (or anything else that converts itself with .tocsc()): never handed to np.asarray."""
    return hasattr(X, "tocsc") and not isinstance(X, np.ndarray)


def csc_entry(M):
    """(symbol name, colptr int64, rowidx int32, val, G, S) for a sparse expression matrix (genes x samples; anything with .tocsc():
    CSR, COO and CSC alike): which reo_set_matrix_csc_* takes it and the three arrays that are handed over.  Pure: no library, no GPU.
    The library wants the row indices of a column strictly increasing, so a matrix that is not in canonical format (unsorted indices or
    duplicates) is COPIED and sum_duplicates()-ed; the caller's matrix is never modified.  A canonical CSC matrix is handed over without
    copying `data`; `indices` is copied only if it is not int32, `indptr` is cast to int64.  Value dtypes follow matrix_entry's rule:
    Float64 / Int64 / Float32 / Int32 as they are, narrower integers and bool to Int64, every other float type to Float64."""
    if len(M.shape) != 2:
        raise DimensionMismatch(REO_EINVAL, "expression matrix must be 2-D (genes x samples)")
    m = M.tocsc()   # (a CSC matrix answers with itself)
    if not m.has_canonical_format:
        if m is M or np.shares_memory(m.data, getattr(M, "data", m.data)):
            m = m.copy()
        m.sum_duplicates()   # sorts the indices of every column and adds up repeated entries, in place (on the copy)
    G, S = m.shape
    if m.dtype in _NATIVE:
        want = m.dtype
    else:
        want = np.dtype(np.int64) if (np.issubdtype(m.dtype, np.integer) or m.dtype == np.bool_) else np.dtype(np.float64)
    val = np.ascontiguousarray(m.data, dtype=want)
    rowidx = np.ascontiguousarray(m.indices, dtype=np.int32)
    colptr = np.ascontiguousarray(m.indptr, dtype=np.int64)
    return "reo_set_matrix_csc_" + _NATIVE[want], colptr, rowidx, val, int(G), int(S)


def valid_mask_bytes(valid, shape) -> np.ndarray:
    """A validity mask as the column-major uint8 array (0 / 1) that reo_set_valid_mask reads.  Pure: no library, no GPU.  Anything
    np.asarray takes; nonzero / True = observed.  A mask whose shape is not `shape` (genes x samples) raises DimensionMismatch."""
    v = np.asarray(valid)
    if v.ndim != 2 or tuple(v.shape) != tuple(int(n) for n in shape):
        raise DimensionMismatch(REO_EINVAL, f"valid mask has shape {tuple(v.shape)}, the matrix is {tuple(int(n) for n in shape)} (genes x samples)")
    return np.asfortranarray(v != 0, dtype=np.uint8)


def first_informative_n(pval_reo: float) -> int:
    """The smallest n with min(1, 2 * 0.5**n) < pval_reo: the first sample count at which reo_threshold leaves its fallback branch
    (8 at 0.01).  Pure."""
    p = float(pval_reo)
    if not 0.0 < p <= 1.0:
        raise DimensionMismatch(REO_EINVAL, f"pval_reo = {pval_reo!r} is outside (0, 1]")
    n = 1
    while n < 2000 and not min(1.0, 2.0 * 0.5 ** n) < p:
        n += 1
    return n


def resolve_min_complete(min_complete, side_sizes, pval_reo: float):
    """The two integers of reo_build_pairs_masked.  Pure.  None: per side min(side size, first_informative_n(pval_reo)), at least 1; an
    int applies to both sides; a pair is taken as it is.  Anything below 1 raises DimensionMismatch."""
    if min_complete is None:
        n = first_informative_n(pval_reo)
        return tuple(max(1, min(int(s), n)) for s in side_sizes)
    if isinstance(min_complete, (int, np.integer)) and not isinstance(min_complete, (bool, np.bool_)):
        mc = (int(min_complete), int(min_complete))
    else:
        mc = tuple(int(m) for m in min_complete)
        if len(mc) != 2:
            raise DimensionMismatch(REO_EINVAL, f"min_complete = {min_complete!r}: None, an int or one int per side")
    if mc[0] < 1 or mc[1] < 1:
        raise DimensionMismatch(REO_EINVAL, f"min_complete = {mc}: each side needs at least 1 jointly observed sample")
    return mc


# the nine classes of an ordered pair in the order of their codes 3*(ic-1)+(it-1): the tally columns of the result (hotpath.HEADER[2:11])
CLASS_NAMES = ("n11", "n12", "n13", "n21", "n22", "n23", "n31", "n32", "n33")
CLASS_ALL = 0x1FF


def class_mask(classes) -> int:
    """The class_mask of reo_pair_list from a selection.  Pure: no library, no GPU.  An int is the mask itself (bit c selects class code c);
    "reversed" is {n13, n31}, the pairs whose order is stable one way in one group and the other way in the other; a name "n11" .. "n33" or
    an iterable of names and / or codes 0 .. 8 selects those.  Anything that selects no class, an unknown name, a code outside 0 .. 8 and a mask
    outside 1 .. 0x1FF raise DimensionMismatch."""
    def bad(why):
        return DimensionMismatch(REO_EINVAL, f"pair classes {classes!r}: {why}")
    if isinstance(classes, (bool, np.bool_)) or classes is None:
        raise bad("a mask, \"reversed\", or names / codes are needed")
    if isinstance(classes, (int, np.integer)):
        m = int(classes)
        if m < 1 or m > CLASS_ALL:
            raise bad("a mask lies in 1 .. 0x1FF (bit c selects class code c)")
        return m
    if isinstance(classes, str):
        classes = [classes]
    m = 0
    for c in classes:
        if isinstance(c, str):
            if c == "reversed":
                m |= (1 << 2) | (1 << 6)
            elif c in CLASS_NAMES:
                m |= 1 << CLASS_NAMES.index(c)
            else:
                raise bad(f"{c!r} is not one of {', '.join(CLASS_NAMES)} or \"reversed\"")
        elif isinstance(c, (int, np.integer)) and not isinstance(c, (bool, np.bool_)) and 0 <= int(c) <= 8:
            m |= 1 << int(c)
        else:
            raise bad(f"{c!r} is not a class code 0 .. 8")
    if m == 0:
        raise bad("no class selected")
    return m


class PairList(NamedTuple):
    """reo_pair_list's CSR: partner[rowptr[q]:rowptr[q + 1]] are the partners of genes[q], ascending, and code[...] their class codes."""
    genes: np.ndarray      # int32, the queries as given
    rowptr: np.ndarray     # int64, len(genes) + 1
    partner: np.ndarray    # int32
    code: np.ndarray       # uint8, index into CLASS_NAMES

    def row(self, q: int):
        a, b = int(self.rowptr[q]), int(self.rowptr[q + 1])
        return self.partner[a:b], self.code[a:b]


class SampleCounts(NamedTuple):
    """reo_sample_counts: per query gene (row) and sample (column, the caller's order), among the n_sel selected partners, in how many pairs
    the gene lies above its partner (n_gt), level with it (n_eq; None when the call was made with ties=False) or below it (n_lt)."""
    genes: np.ndarray      # int32, the queries as given
    n_sel: np.ndarray      # int32, len(genes): selected partners per query
    n_gt: np.ndarray       # int32, len(genes) x S
    n_eq: np.ndarray | None

    @property
    def n_lt(self) -> np.ndarray:
        """n_sel - n_gt - n_eq; needs the tied counts (ties=True)."""
        if self.n_eq is None:
            raise DimensionMismatch(REO_EINVAL, "n_lt needs the tied counts: call sample_counts with ties=True")
        return (self.n_sel[:, None] - self.n_gt - self.n_eq).astype(np.int32)


class PairSupport(NamedTuple):
    """reo_pair_support: how strongly every listed pair supports a call.  The CSR is the one that was handed in (entry e of row q: gene
    genes[q] against partner[e]); per entry and group, in how many of the group's samples the gene lies above its partner (n_gt) or level
    with it (n_eq; None when the call was made with ties=False), and optionally the outcome in every sample."""
    genes: np.ndarray        # int32, the rows as given
    rowptr: np.ndarray       # int64, len(genes) + 1
    partner: np.ndarray      # int32
    code: np.ndarray | None  # uint8, the list's class codes; None for pairs that came without
    n_gt: np.ndarray         # int32, entries x ngroups
    n_eq: np.ndarray | None  # int32, entries x ngroups
    outcome: np.ndarray | None   # uint8, entries x S in the caller's column order: 0 below, 1 tied, 2 above
    group_sizes: np.ndarray  # int64, ngroups: the samples of every group

    def row(self, q: int):
        """(partner, n_gt, n_eq) of row q."""
        a, b = int(self.rowptr[q]), int(self.rowptr[q + 1])
        return self.partner[a:b], self.n_gt[a:b], None if self.n_eq is None else self.n_eq[a:b]

    @property
    def entry_genes(self) -> np.ndarray:
        """The gene of every entry (genes[q] repeated over row q), int32."""
        return np.repeat(self.genes, np.diff(self.rowptr)).astype(np.int32)

    @property
    def n_lt(self) -> np.ndarray:
        """group size - n_gt - n_eq; needs the tied counts (ties=True)."""
        if self.n_eq is None:
            raise DimensionMismatch(REO_EINVAL, "n_lt needs the tied counts: call pair_support with ties=True")
        return (np.asarray(self.group_sizes, dtype=np.int64)[None, :] - self.n_gt - self.n_eq).astype(np.int32)

    @property
    def frac_gt(self) -> np.ndarray:
        """n_gt / group size, float64, entries x ngroups."""
        return self.n_gt.astype(np.float64) / np.asarray(self.group_sizes, dtype=np.float64)[None, :]

    def delta(self, k: int = 0, other=None) -> np.ndarray:
        """Per entry: the fraction of group k's samples with the gene above its partner minus that fraction over all other samples -- the
        two sides that reo_build_pairs(k) compares.  With `other` (a group id): minus that fraction in group `other` alone -- the two sides
        that reo_build_pairs_contrast(k, other) compares.  float64."""
        sizes = np.asarray(self.group_sizes, dtype=np.int64)
        if not 0 <= int(k) < sizes.size:
            raise DimensionMismatch(REO_EINVAL, f"delta: group {k} is outside [0, {sizes.size})")
        k = int(k)
        if other is not None:
            if not 0 <= int(other) < sizes.size or int(other) == k:
                raise DimensionMismatch(REO_EINVAL, f"delta: other = {other} must be a group in [0, {sizes.size}) different from k = {k}")
            o = int(other)
            return self.n_gt[:, k].astype(np.float64) / float(sizes[k]) - self.n_gt[:, o].astype(np.float64) / float(sizes[o])
        rest = self.n_gt.sum(axis=1, dtype=np.int64) - self.n_gt[:, k]
        return self.n_gt[:, k].astype(np.float64) / float(sizes[k]) - rest.astype(np.float64) / float(sizes.sum() - sizes[k])

    def top(self, n: int, k: int = 0) -> np.ndarray:
        """The indices of the n entries with the largest |delta(k)|, largest first; equal |delta| in ascending (gene, partner) order."""
        d = np.abs(self.delta(k))
        order = np.lexsort((self.partner, self.entry_genes, -d))   # (the last key is the primary one)
        return order[: max(int(n), 0)]


class TopPairs(NamedTuple):
    """reo_top_pairs: the n best of all gene pairs i < j for side A (group a) against side B (group b, or every other sample for b None),
    in the order |num| descending, rank_num descending, gene_i ascending, gene_j ascending.  Per pair and side, n_gt = samples with gene_i
    above gene_j and not tied, n_eq = tied samples; with w = n_gt - n_lt per side, num = w_A S_B - w_B S_A and score = |num| / (2 S_A S_B)
    (tie-free: |gt_A / S_A - gt_B / S_B|, Geman's Delta; in general num / (S_A S_B) = 2 delta + eq_A / S_A - eq_B / S_B, ties count half to
    each side).  rank_num = |D_i - D_j| of Context.rank_shift breaks equal scores (tie-free: rank_score is Tan's gamma)."""
    gene_i: np.ndarray       # int32, gene_i < gene_j
    gene_j: np.ndarray       # int32
    n_gt: np.ndarray         # int32, n x 2: side A, side B
    n_eq: np.ndarray         # int32, n x 2
    num: np.ndarray          # int64, N (signed)
    rank_num: np.ndarray     # int64, Gamma
    side_sizes: np.ndarray   # int64, 2: S_A, S_B
    a: int
    b: int | None
    passes: int              # histogram passes of the selection

    @property
    def score(self) -> np.ndarray:
        """|num| / (2 S_A S_B), float64 in [0, 1]."""
        return np.abs(self.num).astype(np.float64) / (2.0 * float(self.side_sizes[0]) * float(self.side_sizes[1]))

    @property
    def rank_score(self) -> np.ndarray:
        """rank_num / (2 S_A S_B), float64."""
        return self.rank_num.astype(np.float64) / (2.0 * float(self.side_sizes[0]) * float(self.side_sizes[1]))

    @property
    def direction(self) -> np.ndarray:
        """int8: +1 where gene_i lies above gene_j more often in A than in B, -1 the other way, 0 at num = 0."""
        return np.sign(self.num).astype(np.int8)

    def disjoint(self, k: int) -> np.ndarray:
        """The indices of the greedy k-TSP selection: the list in order, a pair taken when neither of its genes is used yet, up to k pairs."""
        used: set = set()
        out = []
        for e, (i, j) in enumerate(zip(self.gene_i.tolist(), self.gene_j.tolist())):
            if len(out) >= int(k):
                break
            if i in used or j in used:
                continue
            used.update((i, j))
            out.append(e)
        return np.asarray(out, dtype=np.int64)

    def csr(self):
        """The (genes, rowptr, partner) triple that Context.pair_support takes: one row per pair, gene_i against gene_j, in list order."""
        n = self.gene_i.size
        return self.gene_i.astype(np.int32), np.arange(n + 1, dtype=np.int64), self.gene_j.astype(np.int32)

    def votes(self, support) -> np.ndarray:
        """Per sample, the sum over the pairs of direction * (outcome - 1), int32: positive means A-like.  `support` is the PairSupport of
        csr() made with outcomes=True."""
        if support.outcome is None:
            raise DimensionMismatch(REO_EINVAL, "votes needs the outcome of every sample: call pair_support(csr(), outcomes=True)")
        out = np.asarray(support.outcome)
        if out.shape[0] != self.gene_i.size:
            raise DimensionMismatch(REO_EINVAL, f"votes: the support lists {out.shape[0]} pairs, this object {self.gene_i.size}")
        return (self.direction.astype(np.int32)[:, None] * (out.astype(np.int32) - 1)).sum(axis=0, dtype=np.int64).astype(np.int32)


class TopPartners(NamedTuple):
    """reo_top_partners: per query gene (row) its best m partner genes for side A (group a) against side B (group b, or every other sample
    for b None), in the order |num| descending, rank_num descending, partner ascending -- the subsequence of TopPairs' order over the pairs
    that contain the gene.  Per cell and side, n_gt = samples with the QUERY gene above the partner and not tied, n_eq = tied samples; num
    = N of (query, partner), signed: positive where the query lies above the partner more often in A than in B.  Cells beyond n_found of a
    row are padding: partner -1, everything else 0."""
    genes: np.ndarray        # int32, Q: the query genes
    partner: np.ndarray      # int32, Q x m
    n_gt: np.ndarray         # int32, Q x m x 2: side A, side B
    n_eq: np.ndarray         # int32, Q x m x 2
    num: np.ndarray          # int64, Q x m, N (signed)
    rank_num: np.ndarray     # int64, Q x m, Gamma
    n_found: np.ndarray      # int32, Q
    side_sizes: np.ndarray   # int64, 2: S_A, S_B
    a: int
    b: int | None

    @property
    def score(self) -> np.ndarray:
        """|num| / (2 S_A S_B), float64 in [0, 1], Q x m; 0 in padded cells."""
        return np.abs(self.num).astype(np.float64) / (2.0 * float(self.side_sizes[0]) * float(self.side_sizes[1]))

    @property
    def rank_score(self) -> np.ndarray:
        """rank_num / (2 S_A S_B), float64, Q x m; 0 in padded cells."""
        return self.rank_num.astype(np.float64) / (2.0 * float(self.side_sizes[0]) * float(self.side_sizes[1]))

    @property
    def direction(self) -> np.ndarray:
        """int8, Q x m: +1 where the query gene lies above the partner more often in A than in B, -1 the other way, 0 at num = 0 and in
        padded cells."""
        return np.sign(self.num).astype(np.int8)

    def best(self):
        """(partner, score) per row: the first partner (int32) and its score (float64); -1 / 0.0 where a row found none.  With all genes as
        queries: the best pair score every gene can reach."""
        if self.partner.shape[1] == 0:
            return np.full(self.genes.size, -1, dtype=np.int32), np.zeros(self.genes.size, dtype=np.float64)
        none = self.n_found == 0
        return np.where(none, -1, self.partner[:, 0]).astype(np.int32), np.where(none, 0.0, self.score[:, 0])

    def csr(self):
        """The (genes, rowptr, partner) triple that Context.pair_support takes: one row per query gene with its found partners in order,
        the padding dropped."""
        rowptr = np.zeros(self.genes.size + 1, dtype=np.int64)
        np.cumsum(self.n_found, out=rowptr[1:])
        keep = np.arange(self.partner.shape[1])[None, :] < self.n_found[:, None]
        return self.genes.astype(np.int32), rowptr, self.partner[keep].astype(np.int32)

    def pairs(self) -> TopPairs:
        """The distinct unordered pairs of the table as a TopPairs (passes = 0): re-oriented to gene_i < gene_j -- where the query is the
        larger gene, n_gt becomes S_side - n_gt - n_eq and num changes its sign -- and sorted in TopPairs' order, so that disjoint, csr
        and votes work on it unchanged."""
        keep = np.arange(self.partner.shape[1])[None, :] < self.n_found[:, None]
        q = np.broadcast_to(self.genes[:, None], self.partner.shape)[keep].astype(np.int64)
        p = self.partner[keep].astype(np.int64)
        gt, eq = self.n_gt[keep].astype(np.int64), self.n_eq[keep].astype(np.int64)
        num, gam = self.num[keep].astype(np.int64), self.rank_num[keep].astype(np.int64)
        flip = q > p
        gt = np.where(flip[:, None], self.side_sizes[None, :] - gt - eq, gt)
        num = np.where(flip, -num, num)
        gi, gj = np.minimum(q, p), np.maximum(q, p)
        order = np.lexsort((gj, gi, -gam, -np.abs(num)))                         # (the last key is the primary one)
        first = np.ones(order.size, dtype=bool)
        first[1:] = (gi[order][1:] != gi[order][:-1]) | (gj[order][1:] != gj[order][:-1])   # (the two listings of a pair share every key)
        order = order[first]
        return TopPairs(gi[order].astype(np.int32), gj[order].astype(np.int32), gt[order].astype(np.int32).reshape(-1, 2),
                        eq[order].astype(np.int32).reshape(-1, 2), num[order], gam[order], self.side_sizes, self.a, self.b, 0)


class TopPairsNull(NamedTuple):
    """reo_top_pairs_null: per label permutation (row of `sides`) the best score that the labelling reaches over all gene pairs -- the null of
    the maximum of Context.top_pairs for side A (group a) against side B (group b, or every other sample for b None).  max_num[p] = max |N_p|
    over the eligible pairs, (arg_i[p], arg_j[p]) the pair that attains it (the smallest (i, j) among equals; the rank shift is no
    tie-break here), n_reach[p, t] = the pairs with |N_p| >= cuts[t]; -1, -1, -1 and 0 when no pair is eligible."""
    max_num: np.ndarray      # int64, B
    arg_i: np.ndarray        # int32, B
    arg_j: np.ndarray        # int32, B
    n_reach: np.ndarray      # int64, B x len(cuts)
    cuts: np.ndarray         # int64
    side_sizes: np.ndarray   # int64, 2: S_A, S_B
    a: int
    b: int | None

    @property
    def max_score(self) -> np.ndarray:
        """max_num / (2 S_A S_B), float64: the best score of every permutation."""
        return self.max_num.astype(np.float64) / (2.0 * float(self.side_sizes[0]) * float(self.side_sizes[1]))

    def p_max(self, tp) -> np.ndarray:
        """(1 + #{p : max_num[p] >= |tp.num[e]|}) / (1 + B) per pair e of a TopPairs: the single-step maxT (Westfall-Young) adjusted
        p-value, the observed labelling counted among the permutations.  Non-decreasing down the list, because |num| is non-increasing."""
        obs = np.abs(np.asarray(tp.num, dtype=np.int64))
        ge = (self.max_num[None, :] >= obs[:, None]).sum(axis=1)
        return (1.0 + ge) / (1.0 + self.max_num.size)

    def expected_reach(self) -> np.ndarray:
        """The mean of n_reach over the permutations, one value per cut: with cuts = |tp.num[n - 1]| the expected number of chance pairs at
        least as good as the n-th listed one."""
        return self.n_reach.astype(np.float64).mean(axis=0) if self.n_reach.shape[0] else np.zeros(self.cuts.size)


class TopPartnersNull(NamedTuple):
    """reo_top_partners_null: per label permutation (row of `sides`) and query gene (column) the best score that the labelling reaches over
    the gene's partners -- the null of the first column of Context.top_partners for side A (group a) against side B (group b, or every
    other sample for b None).  max_num[b, r] = max |N_b| over the eligible partners of genes[r], arg_partner[b, r] the smallest partner
    that attains it (the rank shift is no tie-break here), n_reach[b, r] = the partners with |N_b| >= cuts[r]; -1, -1 and 0 where a gene
    has no eligible partner.  The null is single-step (maxT over a gene's partners), not step-down.  A query gene that was selected with
    the same labels (a DEG) gets a permutation p-value of the partner search, not of its selection."""
    genes: np.ndarray        # int32, Q: the query genes
    max_num: np.ndarray      # int64, B x Q
    arg_partner: np.ndarray  # int32, B x Q
    n_reach: np.ndarray      # int32, B x Q, or B x 0 without cuts
    cuts: np.ndarray         # int64, Q, or 0 without cuts
    side_sizes: np.ndarray   # int64, 2: S_A, S_B
    a: int
    b: int | None

    @property
    def max_score(self) -> np.ndarray:
        """max_num / (2 S_A S_B), float64, B x Q: the best partner score of every gene under every permutation."""
        return self.max_num.astype(np.float64) / (2.0 * float(self.side_sizes[0]) * float(self.side_sizes[1]))

    def _same_genes(self, tp, what):
        if not np.array_equal(np.asarray(tp.genes), self.genes):
            raise ValueError(f"{what}: the TopPartners lists other query genes than the null (the rows must be the same genes in the same order)")
        keep = np.arange(tp.partner.shape[1])[None, :] < np.asarray(tp.n_found)[:, None]
        return np.abs(np.asarray(tp.num, dtype=np.int64)), keep

    def p_row(self, tp) -> np.ndarray:
        """(1 + #{b : max_num[b, r] >= |tp.num[r, e]|}) / (1 + B) per cell of a TopPartners of the same genes (ValueError otherwise): the
        single-step maxT adjusted p-value over the partners of the row's gene, the observed labelling counted among the permutations.
        Non-decreasing along a row, because |num| is non-increasing; 1.0 in padded cells."""
        obs, keep = self._same_genes(tp, "p_row")
        ge = (self.max_num.T[:, None, :] >= obs[:, :, None]).sum(axis=2)
        return np.where(keep, (1.0 + ge) / (1.0 + self.max_num.shape[0]), 1.0)

    def p_max(self, tp) -> np.ndarray:
        """As p_row with the maximum over ALL rows in place of the row's own: adjusted for the search over genes and partners.  With all
        genes as queries it equals TopPairsNull.p_max.  1.0 in padded cells."""
        obs, keep = self._same_genes(tp, "p_max")
        top = self.max_num.max(axis=1) if self.max_num.shape[1] else np.full(self.max_num.shape[0], -1, dtype=np.int64)
        ge = (top[None, None, :] >= obs[:, :, None]).sum(axis=2)
        return np.where(keep, (1.0 + ge) / (1.0 + self.max_num.shape[0]), 1.0)

    def expected_reach(self) -> np.ndarray:
        """The mean of n_reach over the permutations, one value per query gene with a cut: with cuts[r] = |tp.num[r, m - 1]| the expected
        number of chance partners at least as good as the row's m-th listed one."""
        return self.n_reach.astype(np.float64).mean(axis=0) if self.n_reach.shape[0] else np.zeros(self.n_reach.shape[1])

    def overall(self):
        """(max_num, gene_i, gene_j) per permutation: the largest max_num over the rows and the smallest (min(q, p), max(q, p)) among the
        rows that attain it; -1, -1, -1 where no row has a partner.  With all genes as queries (and the mask, if any, over queries and
        partners alike) these are max_num, arg_i, arg_j of TopPairsNull."""
        B, Q = self.max_num.shape
        top = self.max_num.max(axis=1) if Q else np.full(B, -1, dtype=np.int64)
        gi, gj = np.full(B, -1, dtype=np.int32), np.full(B, -1, dtype=np.int32)
        for p in range(B):
            if top[p] < 0:
                continue
            at = np.flatnonzero(self.max_num[p] == top[p])
            q, w = self.genes[at].astype(np.int64), self.arg_partner[p, at].astype(np.int64)
            lo, hi = np.minimum(q, w), np.maximum(q, w)
            e = np.lexsort((hi, lo))[0]
            gi[p], gj[p] = lo[e], hi[e]
        return top.astype(np.int64), gi, gj


class TopPairsLoo(NamedTuple):
    """reo_top_pairs_loo: leave-one-out cross-validation of the k-TSP classifier for side A (group a) against side B (group b, or every
    other sample for b None).  Row s = sample s (the caller's column): the kmax picks of the greedy disjoint selection on both sides
    WITHOUT s, in the order of TopPairs with the fold's own counts, sizes and rank shifts; num = N of the fold (signed), rank_num = its
    Gamma, outcome = what sample s itself shows on the pick (+1 gene_i above gene_j, 0 tied, -1 below).  The selection is nested: the
    first k picks are the k-TSP of every k <= kmax.  gene_i = gene_j = -1 (num, rank_num, outcome 0) where a fold has fewer disjoint
    pairs and in the rows of samples on neither side (side 2), which are no folds."""
    gene_i: np.ndarray       # int32, S x kmax
    gene_j: np.ndarray       # int32, S x kmax
    num: np.ndarray          # int64, S x kmax
    rank_num: np.ndarray     # int64, S x kmax
    outcome: np.ndarray      # int8, S x kmax
    side: np.ndarray         # int8, S: 1 = A, 0 = B, 2 = neither
    side_sizes: np.ndarray   # int64, 2: S_A, S_B (of the full data)
    a: int
    b: int | None
    cut: int                 # the cut T on the full-data |N| that defines the candidates
    n_candidates: int

    def votes(self) -> np.ndarray:
        """S x kmax int32: the cumulative sum along k of sign(num) * outcome -- the k-TSP vote of the held-out sample with the first k
        picks of its own fold; positive means A-like."""
        return np.cumsum(np.sign(self.num).astype(np.int32) * self.outcome.astype(np.int32), axis=1, dtype=np.int64).astype(np.int32).reshape(self.num.shape)

    def predictions(self, k: int) -> np.ndarray:
        """int8 per sample with the first k picks: +1 A-like, -1 B-like, 0 undecided; 0 for the samples that are no folds."""
        k = int(k)
        if not 1 <= k <= self.num.shape[1]:
            raise DimensionMismatch(REO_EINVAL, f"predictions: k = {k}, between 1 and kmax = {self.num.shape[1]}")
        return np.where(self.side == 2, 0, np.sign(self.votes()[:, k - 1])).astype(np.int8)

    def errors(self) -> dict:
        """{"n_wrong", "n_undecided", "n_folds"}: per k = 1 .. kmax (int64 arrays of length kmax) the folds whose held-out sample is
        predicted onto the other side, those left undecided (vote 0), and the number of folds."""
        fold = self.side != 2
        truth = np.where(self.side == 1, 1, -1)[fold]
        pred = np.sign(self.votes()[fold, :])
        kmax = self.num.shape[1]
        return {"n_wrong": (pred == -truth[:, None]).sum(axis=0, dtype=np.int64).reshape(kmax),
                "n_undecided": (pred == 0).sum(axis=0, dtype=np.int64).reshape(kmax),
                "n_folds": np.full(kmax, int(fold.sum()), dtype=np.int64)}

    def error_rate(self, k=None):
        """(wrong + undecided) / folds with the first k picks, float64; k None: the array over k = 1 .. kmax."""
        e = self.errors()
        rate = (e["n_wrong"] + e["n_undecided"]).astype(np.float64) / np.maximum(e["n_folds"], 1)
        if k is None:
            return rate
        k = int(k)
        if not 1 <= k <= rate.size:
            raise DimensionMismatch(REO_EINVAL, f"error_rate: k = {k}, between 1 and kmax = {rate.size}")
        return float(rate[k - 1])

    def best_k(self, odd: bool = True) -> int:
        """The smallest k with the lowest error rate; odd=True (the k-TSP convention: no tied votes on tie-free data) looks at odd k only."""
        rate = self.error_rate()
        ks = [k for k in range(1, rate.size + 1) if not odd or k % 2 == 1]
        return min(ks, key=lambda k: (rate[k - 1], k))

    def pair_frequency(self, k: int):
        """(gene_i, gene_j, count): the distinct pairs among the first k picks of all folds and the number of folds that chose each, in the
        order count descending, then (i, j) ascending; int32, int32, int64."""
        k = int(k)
        if not 1 <= k <= self.num.shape[1]:
            raise DimensionMismatch(REO_EINVAL, f"pair_frequency: k = {k}, between 1 and kmax = {self.num.shape[1]}")
        gi, gj = self.gene_i[:, :k].reshape(-1), self.gene_j[:, :k].reshape(-1)
        keep = gi >= 0
        if not keep.any():
            return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int64)
        pairs, count = np.unique(np.stack([gi[keep], gj[keep]], axis=1), axis=0, return_counts=True)
        order = np.lexsort((pairs[:, 1], pairs[:, 0], -count))
        return pairs[order, 0].astype(np.int32), pairs[order, 1].astype(np.int32), count[order].astype(np.int64)


def bh_columns(p: np.ndarray) -> np.ndarray:
    """Benjamini-Hochberg down every column of p (rows x columns, float64): p * n / rank in ascending order (a stable sort), the reverse
    cumulative minimum, clamped to 1 -- the rule of the reference's BenjaminiHochberg call (src/RankCompV3.jl:413), restated in numpy.
    One row: the values as they are."""
    p = np.asarray(p, dtype=np.float64)
    if p.ndim != 2:
        raise DimensionMismatch(REO_EINVAL, "bh_columns takes a rows x columns matrix")
    n = p.shape[0]
    if n <= 1:
        return p.copy()
    order = np.argsort(p, axis=0, kind="stable")
    adj = np.take_along_axis(p, order, axis=0) * (n / np.arange(1, n + 1))[:, None]
    adj = np.minimum.accumulate(adj[::-1], axis=0)[::-1]
    out = np.empty_like(p)
    np.put_along_axis(out, order, np.minimum(adj, 1.0), axis=0)
    return out


class SampleTests(NamedTuple):
    """reo_sample_tests: per query gene (row) and sample (column, the caller's order), Fisher's exact test of the sample's orderings of the
    gene against the pairs that are stable in the control group.  The 2 x 2 table of a cell is [[n_above_ctrl, n_below_ctrl], [u, d]] with
    u = rev_up + (n_above_ctrl - rev_down - the ties of that half) partners below the gene in the sample.  The integer fields are None
    when the call was made with counts=False.  Control samples are tested against a background they helped to define."""
    genes: np.ndarray          # int32, the queries as given
    n_above_ctrl: np.ndarray   # int32, len(genes): background partners the gene is stably above in the control group
    n_below_ctrl: np.ndarray   # int32, len(genes): ... stably below
    rev_up: np.ndarray | None    # int32, len(genes) x S: partners of n_below_ctrl that the gene lies ABOVE in the sample
    rev_down: np.ndarray | None  # int32: partners of n_above_ctrl that the gene lies BELOW in the sample
    tied: np.ndarray | None      # int32: background partners tied with the gene in the sample
    p_up: np.ndarray           # float64, len(genes) x S: P(X >= u)
    p_down: np.ndarray         # float64: P(X <= u)

    @property
    def pval(self) -> np.ndarray:
        """The two-sided value min(1, 2 min(p_up, p_down)): the doubling rule of the reference's own two-sided tests."""
        return np.minimum(1.0, 2.0 * np.minimum(self.p_up, self.p_down))

    def padj(self) -> np.ndarray:
        """Benjamini-Hochberg of pval per sample column, over the queried genes (bh_columns)."""
        return bh_columns(self.pval)

    def calls(self, pval_deg: float, padj_deg: float) -> np.ndarray:
        """int8, len(genes) x S: +1 (up) where pval <= pval_deg, padj <= padj_deg and p_up < p_down; -1 (down) where both thresholds hold
        and p_down < p_up; else 0."""
        sig = (self.pval <= pval_deg) & (self.padj() <= padj_deg)
        out = np.zeros(self.p_up.shape, dtype=np.int8)
        out[sig & (self.p_up < self.p_down)] = 1
        out[sig & (self.p_down < self.p_up)] = -1
        return out


class SampleCalls(NamedTuple):
    """reo_sample_calls: per query gene (row) and sample (column, the caller's order) the call that SampleTests.calls(pval_deg, padj_deg)
    forms on the host, formed on the device -- Benjamini-Hochberg per sample column over the queried genes included.  No p-values and no
    padj values come back (SampleTests keeps those)."""
    genes: np.ndarray    # int32, the queries as given
    calls: np.ndarray    # int8, len(genes) x S: +1 up, -1 down, 0 neither
    cut: np.ndarray      # int32, S: rows of the column with padj <= padj_deg (the step-up rule's k*), whatever pval_deg says
    n_up: np.ndarray     # int32, S: rows of the column called +1
    n_down: np.ndarray   # int32, S: rows of the column called -1


class PermNull(NamedTuple):
    """Context.permutation_null: the label-permutation null of one comparison over B permutations.  delta1_obs[i]: Δ1 of gene i in one pass
    on the observed table with the reference set held fixed; n_ge[i]: permutations whose |Δ1| of gene i reaches the observed one (equality
    counts); n_up[p] / n_down[p]: genes that permutation p calls up / down under the run's pval_deg and padj_deg; se_null[p]: its pass's
    trimmed standard deviation; delta1_null: B x G, every permutation's Δ1 (None unless keep_null=True)."""
    delta1_obs: np.ndarray
    n_ge: np.ndarray
    n_up: np.ndarray
    n_down: np.ndarray
    se_null: np.ndarray
    delta1_null: object = None

    @property
    def n_perm(self) -> int:
        return int(self.n_up.size)

    @property
    def p_perm(self) -> np.ndarray:
        """(1 + n_ge) / (1 + B): the empirical p-value with the observed labelling counted among the permutations."""
        return (1.0 + self.n_ge) / (1.0 + self.n_perm)

    def expected_false_calls(self) -> float:
        """The mean number of genes a permutation calls (n_up + n_down)."""
        return float(np.mean(self.n_up + self.n_down))

    def fdr_hat(self, n_called_obs: int) -> float:
        """expected_false_calls() / max(1, n_called_obs), clipped to 1."""
        return float(min(1.0, self.expected_false_calls() / max(1, int(n_called_obs))))


def side_a_rows(side_a, S: int) -> np.ndarray:
    """Label rows as the B x S uint8 array (1 = side A) that the library reads; a single row becomes 1 x S.  Values other than 0 / 1 (or
    False / True) are kept as they are for the library to refuse."""
    rows = np.asarray(side_a)
    if rows.dtype == bool:
        rows = rows.astype(np.uint8)
    if rows.ndim == 1:
        rows = rows.reshape(1, -1)
    if rows.ndim != 2 or rows.shape[1] != S:
        raise DimensionMismatch(REO_EINVAL, f"side_a has shape {tuple(np.shape(side_a))}, label rows are B x S = B x {S}")
    if rows.size and (rows.min() < 0 or rows.max() > 255):
        raise DimensionMismatch(REO_EINVAL, "side_a: label rows hold 0 (side B) and 1 (side A)")
    return np.ascontiguousarray(rows, dtype=np.uint8)


def permuted_labels(group_ids, k: int, n_perm: int, seed: int = 0, strata=None, include_observed: bool = False) -> np.ndarray:
    """n_perm label rows for Context.permutation_null: uint8 n_perm x S, 1 = side A.  The observed row is group_ids == k; every other row
    shuffles it with numpy's Generator(PCG64(seed)) -- over all samples, or, with `strata` (one label per sample: batch, patient), within
    each stratum, which keeps every stratum's count of ones.  The count of ones is kept in every row, the same seed gives the same rows,
    and a row is never the observed labelling nor a repeat of an earlier row (drawn again; ValueError when the labels do not have that many
    distinct arrangements).  include_observed=True makes row 0 the observed labelling itself (the identity)."""
    gid = np.asarray(group_ids).reshape(-1)
    obs = (gid == k).astype(np.uint8)
    S = obs.size
    if n_perm < 1:
        raise ValueError("n_perm must be at least 1")
    if obs.sum() == 0 or obs.sum() == S:
        raise ValueError(f"group {k!r} holds {int(obs.sum())} of {S} samples: nothing to permute")
    if strata is None:
        blocks = [np.arange(S)]
    else:
        st = np.asarray(strata).reshape(-1)
        if st.size != S:
            raise ValueError(f"strata has {st.size} labels for {S} samples")
        blocks = [np.flatnonzero(st == v) for v in sorted(set(st.tolist()), key=repr)]
    rng = np.random.Generator(np.random.PCG64(int(seed)))
    rows = np.empty((n_perm, S), dtype=np.uint8)
    seen = {obs.tobytes()}
    start = 0
    if include_observed:
        rows[0] = obs
        start = 1
    misses = 0
    p = start
    while p < n_perm:
        row = obs.copy()
        for idx in blocks:
            row[idx] = rng.permutation(obs[idx])
        key = row.tobytes()
        if key in seen:
            misses += 1
            if misses > 1000 + 100 * n_perm:
                raise ValueError(f"the labels have fewer than {n_perm} distinct arrangements besides the observed one")
            continue
        seen.add(key)
        rows[p] = row
        p += 1
    return rows


def permuted_sides(group_ids, a: int, b=None, n_perm: int = 1000, seed: int = 0, strata=None, include_observed: bool = False) -> np.ndarray:
    """n_perm label rows for Context.top_pairs_null: uint8 n_perm x S, 1 = side A (group a), 0 = side B (group b, or every other sample for
    b None), 2 = the samples of groups on neither side, which keep their 2 in every row.  The observed row is shuffled with numpy's
    Generator(PCG64(seed)) among the samples of A and B only -- freely, or, with `strata` (one label per sample: batch, patient), within
    each stratum, which keeps every stratum's count of ones.  The counts of ones and zeros are kept in every row, the same seed gives the
    same rows, and a row is never the observed labelling nor a repeat of an earlier row (drawn again; ValueError when the labels do not
    have that many distinct arrangements).  include_observed=True makes row 0 the observed labelling itself (the identity)."""
    gid = np.asarray(group_ids).reshape(-1)
    if b is not None and b == a:
        raise ValueError(f"b == a == {a!r}: the two sides must differ")
    obs = np.where(gid == a, 1, 0 if b is None else np.where(gid == b, 0, 2)).astype(np.uint8)
    S = obs.size
    if n_perm < 1:
        raise ValueError("n_perm must be at least 1")
    if (obs == 1).sum() == 0 or (obs == 0).sum() == 0:
        raise ValueError(f"side A holds {int((obs == 1).sum())} and side B {int((obs == 0).sum())} of {S} samples: nothing to permute")
    part = obs != 2
    if strata is None:
        blocks = [np.flatnonzero(part)]
    else:
        st = np.asarray(strata).reshape(-1)
        if st.size != S:
            raise ValueError(f"strata has {st.size} labels for {S} samples")
        blocks = [np.flatnonzero((st == v) & part) for v in sorted(set(st.tolist()), key=repr)]
    rng = np.random.Generator(np.random.PCG64(int(seed)))
    rows = np.empty((n_perm, S), dtype=np.uint8)
    seen = {obs.tobytes()}
    start = 0
    if include_observed:
        rows[0] = obs
        start = 1
    misses = 0
    p = start
    while p < n_perm:
        row = obs.copy()
        for idx in blocks:
            row[idx] = rng.permutation(obs[idx])
        key = row.tobytes()
        if key in seen:
            misses += 1
            if misses > 1000 + 100 * n_perm:
                raise ValueError(f"the labels have fewer than {n_perm} distinct arrangements besides the observed one")
            continue
        seen.add(key)
        rows[p] = row
        p += 1
    return rows


class SampleScores(NamedTuple):
    """Per DEG (row) and sample (column): of the gene's n_pairs reversed pairs (n13 and n31 against the partner set), how many show the
    order of the non-control side in that sample (treat_like), how many the control's (ctrl_like), how many are tied."""
    genes: np.ndarray      # int32
    n_pairs: np.ndarray    # int32, len(genes): n13 + n31 partners
    treat_like: np.ndarray  # int32, len(genes) x S: gt(n13) + lt(n31)
    ctrl_like: np.ndarray   # int32: lt(n13) + gt(n31)
    tied: np.ndarray        # int32

    @property
    def net(self) -> np.ndarray:
        return (self.treat_like - self.ctrl_like).astype(np.int32)


def sample_scores_from(c13: SampleCounts, c31: SampleCounts) -> SampleScores:
    """The scores from the counts of the two reversed classes.  Pure: no library, no GPU.  n13 is "control i < j, the rest i > j"
    (src/RankCompV3.jl:369-384), so `gt` is the treatment-like outcome there and `lt` for n31."""
    return SampleScores(c13.genes, (c13.n_sel + c31.n_sel).astype(np.int32), (c13.n_gt + c31.n_lt).astype(np.int32),
                        (c13.n_lt + c31.n_gt).astype(np.int32), (c13.n_eq + c31.n_eq).astype(np.int32))


UNIQUE_ID_BYTES = 128


def comm_unique_id() -> bytes:
    """reo_comm_unique_id: the 128 bytes rank 0 hands to every rank of a one-process-per-GPU run."""
    buf = ctypes.create_string_buffer(UNIQUE_ID_BYTES)
    check(lib().reo_comm_unique_id(buf))
    return buf.raw


def is_device_tensor(data) -> bool:
    """A torch tensor that lives on a GPU (without importing torch for anything that is not one)."""
    return type(data).__module__.split(".")[0] == "torch" and hasattr(data, "data_ptr") and bool(getattr(data, "is_cuda", False))


def device_matrix(t):
    """(device pointer, G, S, ld, dtype name, tensor to keep alive) for a 2-D torch tensor on a ROCm device.  Plumbing only: a tensor
    of float64 / int64 / float32 / int32 whose strides are (1, ld), ld >= G -- column-major -- is used in place; any other layout is
    made column-major ON THE DEVICE (t.t().contiguous().t()), other dtypes are cast on the device first (integers and bool to int64,
    floats to float64).  The stream that produced the tensor is synchronised before the pointer is handed over; the caller keeps the
    returned tensor alive until build_pairs has returned."""
    import torch
    if t.dim() != 2:
        raise DimensionMismatch(REO_EINVAL, "expression matrix must be 2-D (genes x samples)")
    names = {torch.float64: "f64", torch.int64: "i64", torch.float32: "f32", torch.int32: "i32"}
    t = t.detach()
    if t.dtype not in names:
        t = t.to(torch.float64 if t.dtype.is_floating_point else torch.int64)
    G, S = t.shape
    if not (G > 0 and S > 1 and t.stride(0) == 1 and t.stride(1) >= G):
        t = t.t().contiguous().t()   # column-major, ld = G
    torch.cuda.current_stream(t.device).synchronize()
    return int(t.data_ptr()), int(G), int(S), int(t.stride(1)) if S > 1 else int(max(G, 1)), names[t.dtype], t


def is_device_sparse(t) -> bool:
    """A torch tensor on a GPU whose layout is sparse_csc, sparse_csr or sparse_coo (without importing torch for anything that is not a
    tensor).  Such a tensor has no strides and no data_ptr: it never goes to device_matrix."""
    if not (type(t).__module__.split(".")[0] == "torch" and hasattr(t, "layout") and bool(getattr(t, "is_cuda", False))):
        return False
    import torch
    return t.layout in (torch.sparse_csc, torch.sparse_csr, torch.sparse_coo)


def device_csc_entry(t):
    """(type suffix, G, S, nnz, colptr tensor, rowidx tensor, value tensor, index_bits, tensors to keep alive) for a 2-D sparse torch
    tensor (genes x samples, or genes x cells): what reo_set_matrix_csc_dev_<suffix> / reo_set_matrix_pseudobulk_csc_dev_<suffix> take.
    Pure: no library and no GPU (a CPU tensor gets the same answer).  A sparse_csc tensor is used IN PLACE: ccol_indices(), row_indices()
    and values() are the caller's own storage -- and so is the .t() of a cells x genes sparse_csr tensor (AnnData's orientation), which
    torch answers with a sparse_csc view.  Every other layout goes through to_sparse_csc() on the tensor's device.  The index dtype
    (int32 / int64) is kept; value dtypes follow csc_entry's rule: float64 / int64 / float32 / int32 as they are, narrower integers and
    bool to int64, every other float type to float64, cast on the device.
    Nothing is sorted or coalesced here: torch accepts a CSC tensor whose row indices are unsorted or repeated inside a column
    (check_invariants=False), the library refuses it (REO_EINVAL, "not strictly increasing"), and
    t.to_sparse_coo().coalesce().to_sparse_csc() is the canonical form of such a tensor.  The stream that produced the tensor is
    synchronised before the pointers are handed over, as in device_matrix."""
    import torch
    if t.dim() != 2:
        raise DimensionMismatch(REO_EINVAL, "expression matrix must be 2-D (genes x samples): batched sparse tensors are not taken")
    t = t.detach()
    if t.layout != torch.sparse_csc:
        t = t.to_sparse_csc()
    G, S = t.shape
    colptr, rowidx, val = t.ccol_indices(), t.row_indices(), t.values()
    if val.dim() != 1:
        raise DimensionMismatch(REO_EINVAL, "expression matrix must be 2-D (genes x samples): block or hybrid sparse tensors are not taken")
    names = {torch.float64: "f64", torch.int64: "i64", torch.float32: "f32", torch.int32: "i32"}
    if val.dtype not in names:
        val = val.to(torch.float64 if val.dtype.is_floating_point else torch.int64)
    if colptr.dtype != rowidx.dtype or colptr.dtype not in (torch.int32, torch.int64):
        colptr, rowidx = colptr.to(torch.int64), rowidx.to(torch.int64)
    colptr, rowidx, val = colptr.contiguous(), rowidx.contiguous(), val.contiguous()
    if t.is_cuda:
        torch.cuda.current_stream(t.device).synchronize()
    bits = 32 if colptr.dtype == torch.int32 else 64
    return names[val.dtype], int(G), int(S), int(rowidx.numel()), colptr, rowidx, val, bits, [t, colptr, rowidx, val]


def _dptr(t):
    """the device pointer of a tensor, None for an empty one"""
    return ctypes.c_void_p(int(t.data_ptr())) if t.numel() else None


class Context:
    """One reo_ctx: one GPU (or, with n_gpus, all GPUs of this process behind one handle), one expression matrix."""

    def __init__(self, device: int = -1, seed: int = 0, n_gpus: int | None = None):
        self._h = ctypes.c_void_p()
        self._L = lib()
        if n_gpus is None:
            check(self._L.reo_create(ctypes.byref(self._h), int(device), int(seed) & 0xFFFFFFFFFFFFFFFF))
        else:  # reo_create_multi: 0 = all visible devices
            check(self._L.reo_create_multi(ctypes.byref(self._h), int(n_gpus), int(seed) & 0xFFFFFFFFFFFFFFFF))
        self._keep = []  # keeps callbacks / device tensors alive
        self.G = self.S = 0
        self.ngroups = 0
        self._group_id = np.zeros(0, dtype=np.int32)

    def close(self) -> None:
        if self._h:
            self._L.reo_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- problem definition -------------------------------------------------
    def set_matrix(self, X: np.ndarray) -> None:
        """X is genes x samples (host); Float64, Float32, Int64 or Int32 as it is, any other integer dtype -> Int64, any other float
        dtype -> Float64, like Matrix(df_expr).  A column-major array is read in place; a row-major (C-ordered) one is copied
        column-major on the host first, or with REO_ROWMAJOR=1 read in place too (host_matrix_entry).  A scipy.sparse matrix goes up
        as CSC and becomes dense on the device (csc_entry)."""
        if is_sparse(X):   # a scipy.sparse matrix: CSC, densified on the device (csc_entry); there is no other route for one
            name, colptr, rowidx, val, G, S = csc_entry(X)
            check(getattr(self._L, name)(self._h, G, S, _ptr(colptr), _ptr(rowidx) if rowidx.size else None, _ptr(val) if val.size else None))
            self.G, self.S = G, S
            return
        name, Xf, ld = host_matrix_entry(X)
        G, S = Xf.shape
        check(getattr(self._L, name)(self._h, _ptr(Xf), G, S, ld))
        self.G, self.S = G, S

    def set_matrix_device(self, dev_ptr: int, G: int, S: int, ld: int, dtype: str, keepalive=None) -> None:
        """Column-major matrix already resident in HBM (dtype 'f64', 'i64', 'f32' or 'i32')."""
        if dtype not in ("f64", "i64", "f32", "i32"):
            raise DimensionMismatch(REO_EINVAL, f"dtype {dtype!r}: a device matrix is 'f64', 'i64', 'f32' or 'i32'")
        fn = getattr(self._L, "reo_set_matrix_dev_" + dtype)
        check(fn(self._h, ctypes.c_void_p(dev_ptr), G, S, ld))
        self._keep.append(keepalive)
        self.G, self.S = G, S

    def set_matrix_tensor(self, t) -> None:
        """A torch tensor on the context's device (genes x samples) as the expression matrix: a strided one is used where it is
        (device_matrix), a sparse one (sparse_csc / sparse_csr / sparse_coo) is checked and made dense on the device from its CSC arrays
        (device_csc_entry, reo_set_matrix_csc_dev_*; the tensor may go once the call has returned)."""
        if is_device_sparse(t):
            ty, G, S, nnz, colptr, rowidx, val, bits, keep = device_csc_entry(t)
            check(getattr(self._L, "reo_set_matrix_csc_dev_" + ty)(self._h, G, S, nnz, _dptr(colptr), _dptr(rowidx), bits, _dptr(val)))
            self.G, self.S = G, S
            return
        ptr, G, S, ld, dtype, keep = device_matrix(t)
        self.set_matrix_device(ptr, G, S, ld, dtype, keepalive=keep)

    def set_groups(self, group_id, ngroups: int) -> None:
        gid = np.ascontiguousarray(group_id, dtype=np.int32)
        check(self._L.reo_set_groups(self._h, _ptr(gid), gid.size, int(ngroups)))
        self.ngroups = int(ngroups)
        self._group_id = gid.copy()   # (pair_support: the group sizes)

    def compute_thresholds(self, pval_reo: float) -> np.ndarray:
        check(self._L.reo_compute_thresholds(self._h, float(pval_reo)))
        return self.get_thresholds()

    def set_thresholds(self, m) -> None:
        m = np.ascontiguousarray(m, dtype=np.int32)
        if m.size != 2 * self.ngroups:
            raise DimensionMismatch(REO_EINVAL, "thresholds must be 2 x ngroups")
        check(self._L.reo_set_thresholds(self._h, _ptr(m)))

    def get_thresholds(self) -> np.ndarray:
        m = np.zeros(2 * self.ngroups, dtype=np.int32)
        check(self._L.reo_get_thresholds(self._h, _ptr(m)))
        return m.reshape(self.ngroups, 2).T.copy()  # 2 x ngroups like :362

    def set_shard(self, rank: int, world: int) -> None:
        check(self._L.reo_set_shard(self._h, int(rank), int(world)))

    def comm_init_rank(self, unique_id: bytes, rank: int, world: int) -> None:
        """In-library RCCL: join the communicator of `unique_id` as shard `rank` of `world` (sets the shard too)."""
        if len(unique_id) != UNIQUE_ID_BYTES:
            raise DimensionMismatch(REO_EINVAL, "unique id must be 128 bytes")
        check(self._L.reo_comm_init_rank(self._h, ctypes.c_char_p(unique_id), int(rank), int(world)))

    def set_allreduce(self, fn) -> None:
        """fn(dev_ptr: int, count: int, stream: int) -> None: sum int32[count] (the class table) in place across
        shards, ordered on the HIP stream `stream` (see include/reo_hip.h).  None removes the hook."""
        if fn is None:
            check(self._L.reo_set_allreduce(self._h, ALLREDUCE_FN(), None))
            return

        def _cb(ptr, count, stream, _user):
            try:
                fn(int(ptr), int(count), int(stream or 0))
                return 0
            except Exception:  # never let an exception cross the C boundary
                import traceback
                traceback.print_exc()
                return 1
        cb = ALLREDUCE_FN(_cb)
        self._keep.append(cb)
        check(self._L.reo_set_allreduce(self._h, cb, None))

    def set_allgather(self, fn) -> None:
        """fn(send_ptr: int, recv_ptr: int, bytes_per_rank: int, stream: int) -> None: gather `bytes_per_rank` bytes of
        every shard's `send` into `recv + shard * bytes_per_rank` on every shard, ordered on the HIP stream `stream`
        (the cheaper form of the table exchange, see include/reo_hip.h).  None removes the hook."""
        if fn is None:
            check(self._L.reo_set_allgather(self._h, ALLGATHER_FN(), None))
            return

        def _cb(send, recv, nbytes, stream, _user):
            try:
                fn(int(send), int(recv), int(nbytes), int(stream or 0))
                return 0
            except Exception:  # never let an exception cross the C boundary
                import traceback
                traceback.print_exc()
                return 1
        cb = ALLGATHER_FN(_cb)
        self._keep.append(cb)
        check(self._L.reo_set_allgather(self._h, cb, None))

    # -- hot path -------------------------------------------------------------
    def build_pairs(self, k: int = 0) -> None:
        check(self._L.reo_build_pairs(self._h, int(k)))

    def build_contrast(self, ctrl: int, treat: int) -> None:
        """reo_build_pairs_contrast: the class table of group `ctrl` (c-side) against group `treat` (t-side), classified from the per-group
        counts that the one-vs-rest comparisons of more than two groups share; samples of other groups take no part.  Two groups: (0, 1) is
        build_pairs(0), (1, 0) is build_pairs(1).  info()["contrast_treat"] reports `treat` afterwards."""
        check(self._L.reo_build_pairs_contrast(self._h, int(ctrl), int(treat)))

    def pair_counts(self, i0: int, i1: int, j0: int, j1: int):
        shape = (i1 - i0, j1 - j0, self.ngroups)
        gt = np.zeros(shape, dtype=np.uint16)
        eq = np.zeros(shape, dtype=np.uint16)
        check(self._L.reo_pair_counts(self._h, i0, i1, j0, j1, _ptr(gt), _ptr(eq)))
        return gt, eq

    # -- missing values ---------------------------------------------------------
    def set_valid_mask(self, valid) -> None:
        """reo_set_valid_mask: a G x S validity mask (nonzero / True = observed) beside the resident matrix, in the caller's column
        order; None clears it.  The cell under an invalid entry is ignored by build_pairs_masked but must still be a number (NaN stays
        refused).  While a mask is set, sample_counts, sample_tests, sample_calls, pair_support, rank_shift, top_pairs, top_partners and
        build_contrast are refused."""
        if valid is None:
            check(self._L.reo_set_valid_mask(self._h, None, 0, 0, 0))
            return
        v = valid_mask_bytes(valid, (self.G, self.S))
        check(self._L.reo_set_valid_mask(self._h, _ptr(v), v.shape[0], v.shape[1], max(v.shape[0], 1)))

    def side_sizes(self, k: int = 0):
        """(samples of group k, every other sample) under the labels of set_groups."""
        n1 = int(np.count_nonzero(self._group_id == int(k)))
        return n1, int(self._group_id.size) - n1

    def build_pairs_masked(self, k: int = 0, pval_reo: float = 0.01, min_complete=None):
        """reo_build_pairs_masked: the class table of comparison k from the samples where both genes of a pair are valid under the mask
        of set_valid_mask, each side judged against reo_threshold(jointly valid samples of the side, pval_reo); a side with fewer than
        min_complete such samples is unstable.  min_complete: None (per side min(side size, the first n at which the threshold leaves
        its fallback branch: 8 at 0.01)), an int for both sides, or a pair.  Returns the two integers used.  The context's thresholds
        are neither read nor changed."""
        mc = resolve_min_complete(min_complete, self.side_sizes(k), pval_reo)
        arr = np.asarray(mc, dtype=np.int32)
        check(self._L.reo_build_pairs_masked(self._h, int(k), float(pval_reo), _ptr(arr)))
        return mc

    def pair_counts_masked(self, i0: int, i1: int, j0: int, j1: int):
        """reo_pair_counts_masked (parity hook): (n_gt, n_eq, n_avail), int32, each (i1 - i0) x (j1 - j0) x ngroups."""
        shape = (i1 - i0, j1 - j0, max(self.ngroups, 1))
        gt, eq, av = (np.zeros(shape, dtype=np.int32) for _ in range(3))
        check(self._L.reo_pair_counts_masked(self._h, i0, i1, j0, j1, _ptr(gt), _ptr(eq), _ptr(av)))
        return gt, eq, av

    # -- label-permutation null ---------------------------------------------------
    def perm_codes(self, side_a, k: int = 0, i0: int = 0, i1: int | None = None, j0: int = 0, j1: int | None = None) -> np.ndarray:
        """reo_perm_codes (parity hook): the class codes of ONE permutation's table (side_a: S labels, 1 = side A) in the layout of
        get_codes; equals get_codes of a two-group context with the same seed and thresholds and group ids 1 - side_a."""
        i1 = self.G if i1 is None else i1
        j1 = self.G if j1 is None else j1
        row = side_a_rows(side_a, self.S)
        if row.shape[0] != 1:
            raise DimensionMismatch(REO_EINVAL, "perm_codes takes one label row")
        code = np.zeros((max(i1 - i0, 0), max(j1 - j0, 0)), dtype=np.uint8)
        check(self._L.reo_perm_codes(self._h, int(k), _ptr(row), i0, i1, j0, j1, _ptr(code) if code.size else None))
        return code

    def permutation_null(self, side_a, k: int = 0, ref_mask=None, pval_deg: float = 1.0, padj_deg: float = 0.05, keep_null: bool = False) -> PermNull:
        """reo_perm_null: the label-permutation null of comparison k, whose class table must be the resident one (build_pairs(k)).
        side_a: B x S label rows (1 = side A, exactly as many ones per row as group k has samples; permuted_labels makes them).
        ref_mask: the reference set every pass holds fixed; None fetches ref_mask() -- the set of the last identify_degs -- before the
        call.  One pass per permuted table with the run's pval_deg / padj_deg; all B tables of a batch come from one walk over the bit
        planes.  The resident table is intact afterwards; ref_mask() is refused until the next identify_degs."""
        rows = side_a_rows(side_a, self.S)
        B = rows.shape[0]
        ref = self.ref_mask() if ref_mask is None else np.asarray(ref_mask)
        ref = np.ascontiguousarray(ref != 0, dtype=np.uint8)
        if ref.size != self.G:
            raise DimensionMismatch(REO_EINVAL, "reference mask length != number of genes")
        d_obs = np.zeros(self.G, dtype=np.float64)
        n_ge = np.zeros(self.G, dtype=np.int32)
        n_up, n_down = np.zeros(max(B, 1), dtype=np.int32), np.zeros(max(B, 1), dtype=np.int32)
        se = np.zeros(max(B, 1), dtype=np.float64)
        null = np.zeros((B, self.G), dtype=np.float64) if keep_null else None
        check(self._L.reo_perm_null(self._h, int(k), _ptr(rows) if rows.size else None, B, _ptr(ref), float(pval_deg), float(padj_deg), _ptr(d_obs), _ptr(n_ge),
                                    _ptr(n_up), _ptr(n_down), _ptr(se), _opt(null)))
        return PermNull(d_obs, n_ge, n_up[:B], n_down[:B], se[:B], null)

    def get_codes(self, i0: int, i1: int, j0: int, j1: int) -> np.ndarray:
        code = np.zeros((i1 - i0, j1 - j0), dtype=np.uint8)
        check(self._L.reo_get_codes(self._h, i0, i1, j0, j1, _ptr(code)))
        return code

    def tally(self, ref_mask) -> np.ndarray:
        ref = np.ascontiguousarray(np.asarray(ref_mask) != 0, dtype=np.uint8)
        if ref.size != self.G:
            raise DimensionMismatch(REO_EINVAL, "reference mask length != number of genes")
        cont = np.zeros((self.G, 9), dtype=np.int32)
        check(self._L.reo_tally(self._h, _ptr(ref), _ptr(cont)))
        return cont

    def identify_degs(self, ref0, pval_deg: float, padj_deg: float, n_iter: int, n_conv: int):
        ref = np.ascontiguousarray(np.asarray(ref0) != 0, dtype=np.uint8)
        if ref.size != self.G:
            raise DimensionMismatch(REO_EINVAL, "reference mask length != number of genes")
        result = np.zeros((self.G, 15), dtype=np.float64, order="F")
        iters = ctypes.c_int32(0)
        trace = np.zeros((max(int(n_iter), 1), 2), dtype=np.int32)
        check(self._L.reo_identify_degs(self._h, _ptr(ref), float(pval_deg), float(padj_deg), int(n_iter), int(n_conv),
                                        _ptr(result), ctypes.byref(iters), _ptr(trace)))
        return result, iters.value, [tuple(int(v) for v in t) for t in trace[: iters.value]]

    def ref_mask(self) -> np.ndarray:
        """reo_get_ref_mask: the reference set (bool over the genes) that the last identify_degs counted its returned tallies over --
        tally(ref_mask()) equals result[:, 2:11].  Raises DimensionMismatch when there is none or it is out of date."""
        m = np.zeros(max(self.G, 1), dtype=np.uint8)
        check(self._L.reo_get_ref_mask(self._h, _ptr(m), None))
        return m[: self.G].astype(bool)

    def _partner_mask(self, partner_mask):
        """A caller's partner mask as the uint8 array (0 / 1 per gene) that the library reads, or None."""
        if partner_mask is None:
            return None
        pm = np.ascontiguousarray(np.asarray(partner_mask) != 0, dtype=np.uint8)
        if pm.size != self.G:
            raise DimensionMismatch(REO_EINVAL, "partner mask length != number of genes")
        return pm

    def pair_list_raw(self, genes, mask: int, partner_mask, rowptr, partner, code, capacity: int) -> None:
        """reo_pair_list on caller-made arrays (partner and code None: count only); pair_list is the convenient form."""
        check(self._L.reo_pair_list(self._h, *_genes(genes), _opt(partner_mask), ctypes.c_uint32(mask & 0xFFFFFFFF), _opt(rowptr), _opt(partner),
                                    _opt(code), int(capacity)))

    def pair_list(self, genes, classes, partner_mask=None) -> PairList:
        """The partner genes behind the tallies of `genes` (reo_pair_list): for every query gene the partners j, ascending, with
        partner_mask[j] set (None: the reference set of the last identify_degs, ref_mask()) whose pair with it has one of `classes` -- an
        int mask, names "n11" .. "n33", codes 0 .. 8 or "reversed" (class_mask).  Counts first, allocates, then fills."""
        mask = class_mask(classes)
        g = np.ascontiguousarray(genes, dtype=np.int32).reshape(-1)
        pm = self._partner_mask(partner_mask)
        rowptr = np.zeros(g.size + 1, dtype=np.int64)
        self.pair_list_raw(g, mask, pm, rowptr, None, None, 0)
        total = int(rowptr[-1])
        partner = np.zeros(total, dtype=np.int32)
        code = np.zeros(total, dtype=np.uint8)
        if total:
            self.pair_list_raw(g, mask, pm, rowptr, partner, code, total)
        return PairList(g, rowptr, partner, code)

    def sample_counts_raw(self, genes, mask: int, partner_mask, n_sel, n_gt, n_eq) -> None:
        """reo_sample_counts on caller-made arrays (n_sel and n_eq may be None); sample_counts is the convenient form."""
        check(self._L.reo_sample_counts(self._h, *_genes(genes), _opt(partner_mask), ctypes.c_uint32(mask & 0xFFFFFFFF), _opt(n_sel), _opt(n_gt),
                                        _opt(n_eq)))

    def sample_counts(self, genes, classes, partner_mask=None, ties=True) -> SampleCounts:
        """In which samples (reo_sample_counts): for every query gene and every sample, in how many of its selected pairs -- partners j with
        partner_mask[j] set (None: the reference set of the last identify_degs, ref_mask()) whose pair with it has one of `classes`
        (class_mask) -- the gene lies above its partner, and in how many the two are tied.  ties=False: no tied counts (n_eq None)."""
        mask = class_mask(classes)
        g = np.ascontiguousarray(genes, dtype=np.int32).reshape(-1)
        pm = self._partner_mask(partner_mask)
        n_sel = np.zeros(g.size, dtype=np.int32)
        n_gt = np.zeros((g.size, max(self.S, 1)), dtype=np.int32)
        n_eq = np.zeros_like(n_gt) if ties else None
        self.sample_counts_raw(g, mask, pm, n_sel, n_gt, n_eq)
        return SampleCounts(g, n_sel, n_gt[:, : self.S], None if n_eq is None else n_eq[:, : self.S])

    def sample_scores(self, genes, partner_mask=None) -> SampleScores:
        """Per sample, how far every query gene's reversed pairs (n13, n31) show the non-control order: two sample_counts calls."""
        return sample_scores_from(self.sample_counts(genes, "n13", partner_mask), self.sample_counts(genes, "n31", partner_mask))

    def sample_tests_raw(self, genes, partner_mask, n_above_ctrl, n_below_ctrl, rev_up, rev_down, tied, p_up, p_down) -> None:
        """reo_sample_tests on caller-made arrays (the integer arrays may be None); sample_tests is the convenient form."""
        check(self._L.reo_sample_tests(self._h, *_genes(genes), _opt(partner_mask), _opt(n_above_ctrl), _opt(n_below_ctrl), _opt(rev_up),
                                       _opt(rev_down), _opt(tied), _opt(p_up), _opt(p_down)))

    def sample_tests(self, genes=None, partner_mask=None, counts=True) -> SampleTests:
        """Up or down in one sample (reo_sample_tests): for every query gene (None: all genes) and every sample, Fisher's exact test of the
        sample's orderings of the gene against the partners -- partner_mask[j] set (None: the reference set of the last identify_degs,
        ref_mask()) -- that it is stably above or below in the control group of the resident class table.  counts=False: the per-sample
        integer fields are not fetched (None).  Host arrays; not available on a multi-GPU context."""
        g = np.arange(self.G, dtype=np.int32) if genes is None else np.ascontiguousarray(genes, dtype=np.int32).reshape(-1)
        pm = self._partner_mask(partner_mask)
        shape = (g.size, max(self.S, 1))
        n_above, n_below = np.zeros(g.size, dtype=np.int32), np.zeros(g.size, dtype=np.int32)
        ints = [np.zeros(shape, dtype=np.int32) for _ in range(3)] if counts else [None] * 3
        p_up, p_down = np.ones(shape, dtype=np.float64), np.ones(shape, dtype=np.float64)
        self.sample_tests_raw(g, pm, n_above, n_below, ints[0], ints[1], ints[2], p_up, p_down)
        cut = lambda a: None if a is None else a[:, : self.S]   # noqa: E731
        return SampleTests(g, n_above, n_below, cut(ints[0]), cut(ints[1]), cut(ints[2]), cut(p_up), cut(p_down))

    def sample_calls_raw(self, genes, partner_mask, pval_deg: float, padj_deg: float, calls, cut, n_up, n_down) -> None:
        """reo_sample_calls on caller-made arrays (cut, n_up and n_down may be None); sample_calls is the convenient form."""
        check(self._L.reo_sample_calls(self._h, *_genes(genes), _opt(partner_mask), float(pval_deg), float(padj_deg), _opt(calls), _opt(cut),
                                       _opt(n_up), _opt(n_down)))

    def sample_calls(self, pval_deg: float, padj_deg: float, genes=None, partner_mask=None) -> SampleCalls:
        """Up (+1), down (-1) or neither (0) per query gene (None: all genes) and sample (reo_sample_calls): the tails of sample_tests for
        the same genes and partner_mask, the two-sided value, Benjamini-Hochberg down every sample column over the queried genes and the
        two thresholds, all on the device -- byte for byte sample_tests(genes, partner_mask).calls(pval_deg, padj_deg), with one byte per
        cell coming back.  Host arrays; not available on a multi-GPU context."""
        g = np.arange(self.G, dtype=np.int32) if genes is None else np.ascontiguousarray(genes, dtype=np.int32).reshape(-1)
        pm = self._partner_mask(partner_mask)
        S = max(self.S, 1)
        calls = np.zeros((g.size, S), dtype=np.int8)
        cut, n_up, n_down = (np.zeros(S, dtype=np.int32) for _ in range(3))
        self.sample_calls_raw(g, pm, pval_deg, padj_deg, calls, cut, n_up, n_down)
        return SampleCalls(g, calls[:, : self.S], cut[: self.S], n_up[: self.S], n_down[: self.S])

    def pair_support_raw(self, genes, rowptr, partner, n_gt, n_eq, outcome) -> None:
        """reo_pair_support on caller-made arrays (any may be None); pair_support is the convenient form."""
        check(self._L.reo_pair_support(self._h, *_genes(genes), _opt(rowptr), _genes(partner)[0],
                                       _opt(n_gt), _opt(n_eq), _opt(outcome)))

    def pair_support(self, pairs, ties=True, outcomes=False) -> PairSupport:
        """How strongly (reo_pair_support): for every pair of `pairs` -- a PairList, or a (genes, rowptr, partner) triple of the caller's
        own -- and every group, in how many samples the row's gene lies above the partner, and in how many the two are tied.  ties=False:
        no tied counts (n_eq None).  outcomes=True: also the outcome of every sample, entries x S bytes (0 below, 1 tied, 2 above) in the
        caller's column order -- meant for signatures of hundreds of pairs.  Needs the matrix and the groups, no class table."""
        code = None
        if isinstance(pairs, PairList):
            genes, rowptr, partner, code = pairs
        else:
            genes, rowptr, partner = pairs
        g = np.ascontiguousarray(genes, dtype=np.int32).reshape(-1)
        rp = np.ascontiguousarray(rowptr, dtype=np.int64).reshape(-1)
        pa = np.ascontiguousarray(partner, dtype=np.int32).reshape(-1)
        if rp.size != g.size + 1:
            raise DimensionMismatch(REO_EINVAL, f"pair_support: rowptr has {rp.size} entries for {g.size} rows (one more is needed)")
        if rp.size and int(rp[-1]) != pa.size:
            raise DimensionMismatch(REO_EINVAL, f"pair_support: rowptr lists {int(rp[-1])} entries, partner has {pa.size}")
        if code is not None:
            code = np.asarray(code)
            if code.size != pa.size:
                raise DimensionMismatch(REO_EINVAL, f"pair_support: code has {code.size} entries, partner has {pa.size}")
        n, ng, S = pa.size, max(self.ngroups, 1), max(self.S, 1)
        n_gt = np.zeros((n, ng), dtype=np.int32)
        n_eq = np.zeros_like(n_gt) if ties else None
        outcome = np.zeros((n, S), dtype=np.uint8) if outcomes else None
        if g.size:   # (no rows: nothing to ask; the library refuses n_genes < 1)
            self.pair_support_raw(g, rp, pa, n_gt, n_eq, outcome)
        sizes = np.bincount(np.asarray(self._group_id, dtype=np.int64), minlength=ng)[:ng].astype(np.int64)
        return PairSupport(g, rp, pa, code, n_gt, n_eq, None if outcome is None else outcome[:, : self.S], sizes)

    def _sides(self, a, b):
        """(a, b as the library takes it, (S_A, S_B)) of a search: b None = every sample not in group a."""
        a = int(a)
        gid = self._group_id
        s_a = int(np.count_nonzero(gid == a))
        s_b = int(gid.size) - s_a if b is None else int(np.count_nonzero(gid == int(b)))
        return a, (-1 if b is None else int(b)), np.array([s_a, s_b], dtype=np.int64)

    def rank_shift(self, a: int = 0, b=None) -> np.ndarray:
        """reo_rank_shift: D, int64 of length G.  D_i = W_i(A) S_B - W_i(B) S_A with W_i(side) the sum over the side's samples of (genes
        that i lies above) - (genes that i lies below), untied; side A = group a, side B = group b or, for None, every other sample."""
        a, b, _ = self._sides(a, b)
        D = np.zeros(max(self.G, 1), dtype=np.int64)
        check(self._L.reo_rank_shift(self._h, a, b, _ptr(D)))
        return D[: self.G]

    def top_pairs(self, n: int, a: int = 0, b=None, gene_mask=None) -> TopPairs:
        """Which pairs (reo_top_pairs): the n best of all gene pairs i < j -- both genes inside gene_mask (bool over the genes) when one
        is given -- for group a against group b (None: against every other sample), as a TopPairs in its order.  Fewer than n eligible
        pairs: all of them.  Needs the matrix and the groups, no class table; refused under a validity mask, on a sharded context and on
        n_gpus contexts, and above 65 535 genes or samples."""
        n = int(n)
        a, b, sizes = self._sides(a, b)
        gm = None
        if gene_mask is not None:
            gm = np.asarray(gene_mask)
            if gm.shape != (self.G,):
                raise DimensionMismatch(REO_EINVAL, f"top_pairs: gene_mask has shape {tuple(gm.shape)}, the matrix has {self.G} genes")
            gm = np.ascontiguousarray(gm if gm.dtype == np.uint8 else gm != 0, dtype=np.uint8)
        m = min(max(n, 1), 1 << 20)   # (the library refuses n outside [1, 2^20] before it writes)
        gi, gj = np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.int32)
        counts, key = np.zeros((m, 4), dtype=np.int32), np.zeros((m, 2), dtype=np.int64)
        found, passes = ctypes.c_int64(0), ctypes.c_int32(0)
        check(self._L.reo_top_pairs(self._h, a, b, _opt(gm), n, _ptr(gi), _ptr(gj), _ptr(counts), _ptr(key), ctypes.addressof(found),
                                    ctypes.addressof(passes)))
        k = int(found.value)
        return TopPairs(gi[:k].copy(), gj[:k].copy(), counts[:k, 0::2].copy(), counts[:k, 1::2].copy(), key[:k, 0].copy(), key[:k, 1].copy(),
                        sizes, a, None if b < 0 else b, int(passes.value))

    def top_partners(self, genes=None, m: int = 1, a: int = 0, b=None, partner_mask=None) -> TopPartners:
        """Which partners (reo_top_partners): for every gene of `genes` (None: all genes in order; any order, repeats allowed) its m best
        partner genes -- inside partner_mask (bool over the genes) when one is given; the query itself need not be -- for group a against
        group b (None: against every other sample), as a TopPartners.  A row with fewer than m eligible partners is padded.  Exact; sides
        and refusals as in top_pairs; 1 <= m <= 1024, at most 2^20 queries and 2^26 listed partners per call."""
        m = int(m)
        a, b, sizes = self._sides(a, b)
        g = np.arange(self.G, dtype=np.int32) if genes is None else np.ascontiguousarray(np.asarray(genes).reshape(-1), dtype=np.int32)
        pm = None
        if partner_mask is not None:
            pm = np.asarray(partner_mask)
            if pm.shape != (self.G,):
                raise DimensionMismatch(REO_EINVAL, f"top_partners: partner_mask has shape {tuple(pm.shape)}, the matrix has {self.G} genes")
            pm = np.ascontiguousarray(pm if pm.dtype == np.uint8 else pm != 0, dtype=np.uint8)
        Q = int(g.size)
        w = min(max(m, 1), 1024)   # (the library refuses m outside [1, 1024] before it writes)
        rows = Q if 1 <= Q <= 1 << 20 and Q * w <= 1 << 26 else 1   # (and a number of rows it does not take)
        partner = np.full((rows, w), -1, dtype=np.int32)
        counts, key = np.zeros((rows, w, 4), dtype=np.int32), np.zeros((rows, w, 2), dtype=np.int64)
        found = np.zeros(rows, dtype=np.int32)
        check(self._L.reo_top_partners(self._h, a, b, _ptr(g) if Q else None, Q, _opt(pm), m, _ptr(partner), _ptr(counts), _ptr(key), _ptr(found)))
        return TopPartners(g, partner, counts[:, :, 0::2].copy(), counts[:, :, 1::2].copy(), key[:, :, 0].copy(), key[:, :, 1].copy(), found,
                           sizes, a, None if b < 0 else b)

    def top_partners_null(self, sides, genes=None, a: int = 0, b=None, partner_mask=None, cuts=None) -> TopPartnersNull:
        """The null of a gene's best partner (reo_top_partners_null): for every label row of `sides` (B x S, as in top_pairs_null;
        permuted_sides makes them) and every gene of `genes` (None: all genes in order; any order, repeats allowed) the largest |N| over
        the gene's partners -- inside partner_mask when one is given --, the smallest partner that attains it, and with `cuts` (one value
        of |N| per query gene) how many partners reach the gene's cut, as a TopPartnersNull.  Sides and refusals as in top_partners; one
        walk over the bit planes serves 16 rows; at most 2^20 rows, 2^20 queries and 2^26 cells per call."""
        a, b, sizes = self._sides(a, b)
        rows = np.asarray(sides)
        if rows.ndim == 1:
            rows = rows.reshape(1, -1)
        if rows.ndim != 2 or rows.shape[1] != self.S:
            raise DimensionMismatch(REO_EINVAL, f"top_partners_null: sides has shape {tuple(np.shape(sides))}, label rows are B x S = B x {self.S}")
        if rows.size and (rows.min() < 0 or rows.max() > 255):
            raise DimensionMismatch(REO_EINVAL, "top_partners_null: label rows hold 0 (side B), 1 (side A) and 2 (takes no part)")
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        g = np.arange(self.G, dtype=np.int32) if genes is None else np.ascontiguousarray(np.asarray(genes).reshape(-1), dtype=np.int32)
        pm = None
        if partner_mask is not None:
            pm = np.asarray(partner_mask)
            if pm.shape != (self.G,):
                raise DimensionMismatch(REO_EINVAL, f"top_partners_null: partner_mask has shape {tuple(pm.shape)}, the matrix has {self.G} genes")
            pm = np.ascontiguousarray(pm if pm.dtype == np.uint8 else pm != 0, dtype=np.uint8)
        B, Q = rows.shape[0], int(g.size)
        ct = None
        if cuts is not None:
            ct = np.ascontiguousarray(np.asarray(cuts, dtype=np.int64).reshape(-1))
            if ct.size != Q:
                raise DimensionMismatch(REO_EINVAL, f"top_partners_null: cuts has {ct.size} values, one per query gene is {Q}")
        ok = 1 <= B <= 1 << 20 and 1 <= Q <= 1 << 20 and B * Q <= 1 << 26   # (the library refuses anything else before it writes)
        shape = (B, Q) if ok else (1, 1)
        max_n, arg = np.zeros(shape, dtype=np.int64), np.zeros(shape, dtype=np.int32)
        reach = np.zeros(shape, dtype=np.int32) if ct is not None else None
        check(self._L.reo_top_partners_null(self._h, a, b, _ptr(rows) if rows.size else None, B, _ptr(g) if Q else None, Q, _opt(pm),
                                            _ptr(ct) if ct is not None and ct.size else None, _ptr(max_n), _ptr(arg),
                                            _ptr(reach) if reach is not None else None))
        return TopPartnersNull(g, max_n, arg, reach if reach is not None else np.zeros((B, 0), dtype=np.int32),
                               ct if ct is not None else np.zeros(0, dtype=np.int64), sizes, a, None if b < 0 else b)

    def top_pairs_null(self, sides, a: int = 0, b=None, gene_mask=None, cuts=None) -> TopPairsNull:
        """The null of the best score (reo_top_pairs_null): for every label row of `sides` (B x S, 1 = side A, 0 = side B, 2 = the samples of
        groups on neither side; permuted_sides makes them) the largest |N| over all gene pairs i < j -- both genes inside gene_mask when
        one is given --, the pair that attains it, and per value of `cuts` (up to 8 values of |N|) how many pairs reach it, as a
        TopPairsNull.  Sides and refusals as in top_pairs; one walk over the bit planes serves 16 rows."""
        a, b, sizes = self._sides(a, b)
        rows = np.asarray(sides)
        if rows.ndim == 1:
            rows = rows.reshape(1, -1)
        if rows.ndim != 2 or rows.shape[1] != self.S:
            raise DimensionMismatch(REO_EINVAL, f"top_pairs_null: sides has shape {tuple(np.shape(sides))}, label rows are B x S = B x {self.S}")
        if rows.size and (rows.min() < 0 or rows.max() > 255):
            raise DimensionMismatch(REO_EINVAL, "top_pairs_null: label rows hold 0 (side B), 1 (side A) and 2 (takes no part)")
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        gm = None
        if gene_mask is not None:
            gm = np.asarray(gene_mask)
            if gm.shape != (self.G,):
                raise DimensionMismatch(REO_EINVAL, f"top_pairs_null: gene_mask has shape {tuple(gm.shape)}, the matrix has {self.G} genes")
            gm = np.ascontiguousarray(gm if gm.dtype == np.uint8 else gm != 0, dtype=np.uint8)
        ct = np.zeros(0, dtype=np.int64) if cuts is None else np.ascontiguousarray(np.asarray(cuts, dtype=np.int64).reshape(-1))
        B = rows.shape[0]
        m = min(max(B, 1), 1 << 20)   # (the library refuses n_perm outside [1, 2^20] before it writes)
        nc = min(ct.size, 8)
        max_n, gi, gj = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.int32)
        reach = np.zeros((m, nc), dtype=np.int64)
        check(self._L.reo_top_pairs_null(self._h, a, b, _ptr(rows) if rows.size else None, B, _opt(gm), _ptr(ct) if ct.size else None, ct.size,
                                         _ptr(max_n), _ptr(gi), _ptr(gj), _ptr(reach) if reach.size else None))
        return TopPairsNull(max_n[:B], gi[:B], gj[:B], reach[:B], ct, sizes, a, None if b < 0 else b)

    def top_pairs_loo(self, kmax: int, a: int = 0, b=None, gene_mask=None) -> TopPairsLoo:
        """Leave-one-out cross-validation of k-TSP (reo_top_pairs_loo): for every sample of group a or of side B (group b; None: every
        other sample) the kmax greedy disjoint picks of the search on both sides without that sample -- both genes inside gene_mask when
        one is given -- and the sample's own outcome on every pick, as a TopPairsLoo.  Every fold is decided on the device from one set of
        candidate pairs; exact.  Sides and refusals as in top_pairs; each side needs two samples; 1 <= kmax <= 64."""
        kmax = int(kmax)
        a, b, sizes = self._sides(a, b)
        gm = None
        if gene_mask is not None:
            gm = np.asarray(gene_mask)
            if gm.shape != (self.G,):
                raise DimensionMismatch(REO_EINVAL, f"top_pairs_loo: gene_mask has shape {tuple(gm.shape)}, the matrix has {self.G} genes")
            gm = np.ascontiguousarray(gm if gm.dtype == np.uint8 else gm != 0, dtype=np.uint8)
        m, S = min(max(kmax, 1), 64), max(self.S, 1)   # (the library refuses kmax outside [1, 64] before it writes)
        gi, gj = np.full((S, m), -1, dtype=np.int32), np.full((S, m), -1, dtype=np.int32)
        num, gam = np.zeros((S, m), dtype=np.int64), np.zeros((S, m), dtype=np.int64)
        out, side, stats = np.zeros((S, m), dtype=np.int8), np.full(S, 2, dtype=np.int8), np.zeros(4, dtype=np.int64)
        check(self._L.reo_top_pairs_loo(self._h, a, b, _opt(gm), kmax, _ptr(gi), _ptr(gj), _ptr(num), _ptr(gam), _ptr(out), _ptr(side), _ptr(stats)))
        n = self.S
        return TopPairsLoo(gi[:n], gj[:n], num[:n], gam[:n], out[:n], side[:n], sizes, a, None if b < 0 else b, int(stats[0]), int(stats[1]))

    def mccullagh(self, cont) -> np.ndarray:
        cont = np.ascontiguousarray(cont, dtype=np.int32).reshape(-1, 9)
        out = np.zeros((cont.shape[0], 5), dtype=np.float64)
        check(self._L.reo_mccullagh(self._h, _ptr(cont), cont.shape[0], _ptr(out)))
        return out

    # -- pseudo-bulk front end ------------------------------------------------------
    @staticmethod
    def _pseudobulk_args(cells, order, chunk_ptr):
        """The routing of pseudobulk / set_matrix_pseudobulk: ('csc' | 'dense', 'i64' | 'f64', the arguments up to n_out, G, arrays to
        keep alive).  Sparse cells go up as CSC, everything else as a column-major array; integers as Int64, floats as Float64 (Float32
        and Int32 cells are widened here)."""
        order = np.ascontiguousarray(order, dtype=np.int32)
        chunk_ptr = np.ascontiguousarray(chunk_ptr, dtype=np.int32)
        n_out = chunk_ptr.size - 1
        if hasattr(cells, "tocsc"):
            m = cells.tocsc()
            m.sort_indices()
            G, C = m.shape
            isint = np.issubdtype(m.dtype, np.integer)
            val = np.ascontiguousarray(m.data, dtype=np.int64 if isint else np.float64)
            colptr = np.ascontiguousarray(m.indptr, dtype=np.int64)
            rowidx = np.ascontiguousarray(m.indices, dtype=np.int32)
            args = (G, C, _ptr(colptr), _ptr(rowidx), _ptr(val), _ptr(order), order.size, _ptr(chunk_ptr), n_out)
            return "csc", "i64" if isint else "f64", args, G, (m, val, colptr, rowidx, order, chunk_ptr)
        X = np.asarray(cells)
        isint = np.issubdtype(X.dtype, np.integer)
        Xf = np.asfortranarray(X, dtype=np.int64 if isint else np.float64)
        G, C = Xf.shape
        args = (_ptr(Xf), G, C, G, _ptr(order), order.size, _ptr(chunk_ptr), n_out)
        return "dense", "i64" if isint else "f64", args, G, (Xf, order, chunk_ptr)

    def pseudobulk(self, cells, order, chunk_ptr) -> np.ndarray:
        """Row-wise sums of groups of cells (src/RankCompV3.jl:56-67).  `cells` is a genes x cells
        ndarray (Int64 / Float64) or a scipy.sparse matrix (converted to CSC); `order` lists the cells
        of all output profiles back to back and chunk_ptr delimits them.  Returns genes x profiles."""
        form, ty, args, G, keep = self._pseudobulk_args(cells, order, chunk_ptr)
        out = np.zeros((G, args[-1]), dtype=np.int64 if ty == "i64" else np.float64, order="F")
        check(getattr(self._L, f"reo_pseudobulk_{form}_{ty}")(self._h, *args, _ptr(out)))
        return out

    def set_matrix_pseudobulk(self, cells, order, chunk_ptr) -> None:
        """The same sums, left on the device as the context's expression matrix (reo_set_matrix_pseudobulk_*): arguments and routing of
        pseudobulk, nothing comes back to the host.  The profiles are the samples: set_groups wants one label per profile.
        Cells that are a torch tensor on the context's device are read where they are (reo_set_matrix_pseudobulk_*_dev_*): a sparse one
        through device_csc_entry, a strided one column-major as device_matrix makes it; float32 / int32 cells are summed in Float64 /
        Int64, like the host cells that _pseudobulk_args widens."""
        if is_device_sparse(cells) or is_device_tensor(cells):
            order = np.ascontiguousarray(order, dtype=np.int32)
            chunk_ptr = np.ascontiguousarray(chunk_ptr, dtype=np.int32)
            n_out = chunk_ptr.size - 1
            tail = (_ptr(order) if order.size else None, order.size, _ptr(chunk_ptr), n_out)
            if is_device_sparse(cells):
                ty, G, C, nnz, colptr, rowidx, val, bits, keep = device_csc_entry(cells)
                check(getattr(self._L, "reo_set_matrix_pseudobulk_csc_dev_" + ty)(self._h, G, C, nnz, _dptr(colptr), _dptr(rowidx), bits, _dptr(val), *tail))
            else:
                ptr, G, C, ld, ty, keep = device_matrix(cells)
                check(getattr(self._L, "reo_set_matrix_pseudobulk_dense_dev_" + ty)(self._h, ctypes.c_void_p(ptr), G, C, ld, *tail))
            self.G, self.S = G, n_out
            return
        form, ty, args, G, keep = self._pseudobulk_args(cells, order, chunk_ptr)
        check(getattr(self._L, f"reo_set_matrix_pseudobulk_{form}_{ty}")(self._h, *args))
        self.G, self.S = G, args[-1]

    def filter_matrix(self, min_profiles: int = 0, min_features: int = 0):
        """The reference's low-expression filters (src/RankCompV3.jl:618, :626) on the resident matrix, compacted on the device
        (reo_filter_matrix).  Returns (profile_kept, gene_kept), bool masks over the samples and genes the matrix had; the context's G
        and S are those of what is left, and groups have to be set (again) for the kept profiles."""
        info = self.info()
        pk = np.zeros(info["S"], dtype=np.uint8)
        gk = np.zeros(info["G"], dtype=np.uint8)
        sk, gkn = ctypes.c_int64(0), ctypes.c_int64(0)
        check(self._L.reo_filter_matrix(self._h, int(min_profiles), int(min_features), _ptr(pk) if pk.size else None, _ptr(gk) if gk.size else None,
                                        ctypes.byref(sk), ctypes.byref(gkn)))
        self.G, self.S = int(gkn.value), int(sk.value)
        return pk.astype(bool), gk.astype(bool)

    def get_matrix(self) -> np.ndarray:
        """The resident matrix as it stands (parity hook, reo_get_matrix): genes x samples, column-major, float64 / int64 / float32."""
        info = self.info()
        dt = {1: np.float64, 2: np.int64, 3: np.float32}.get(info["resident_dtype"])
        if dt is None:
            raise DimensionMismatch(REO_EINVAL, "no expression matrix set")
        out = np.zeros((info["G"], info["S"]), dtype=dt, order="F")
        check(self._L.reo_get_matrix(self._h, _ptr(out), out.nbytes))
        return out

    # -- instrumentation -------------------------------------------------------
    def set_profiling(self, on: bool) -> None:
        check(self._L.reo_set_profiling(self._h, 1 if on else 0))

    def reset_timings(self) -> None:
        check(self._L.reo_reset_timings(self._h))

    def timings(self) -> dict:
        ms = np.zeros(NTIMINGS, dtype=np.float64)
        check(self._L.reo_get_timings(self._h, _ptr(ms), NTIMINGS))
        return {"transform_ms": ms[0], "k1_ms": ms[1], "k2_ms": ms[2], "iter_ms": ms[3], "k3_ms": max(ms[3] - ms[2], 0.0), "k2_launches": int(ms[4]),
                "k1_launches": int(ms[5]), "exchange_ms": ms[6], "pseudobulk_ms": ms[7], "k2_full_ms": ms[8],
                "k2_full_launches": int(ms[9]), "k2_delta_ms": ms[10], "set_matrix_host_wall_ms": ms[11]}

    def info(self) -> dict:
        w = np.zeros(46, dtype=np.int64)
        check(self._L.reo_get_info(self._h, _ptr(w), 46))
        v = np.zeros(28, dtype=np.int64)   # fields 0-27 keep their places (tests/test_csc_device_cpu.py reads this line); 28 is appended
        v[:] = w[:28]
        return {"G": int(v[0]), "S": int(v[1]), "Gp": int(v[2]), "table_bytes": int(v[3]), "has_ties": int(v[4]),
                "tiles_owned": int(v[5]), "tiles_total": int(v[6]), "tile_i": int(v[7]), "chunk_j": int(v[8]),
                "chunks_per_panel": int(v[9]), "unit_h": int(v[10]), "sample_slots": int(v[11]),
                "shared_group_counts": int(v[12]), "group_count_bytes": int(v[13]), "transform_in_lds": int(v[14]), "xcc_local_histograms": int(v[15]),
                "cycle_period": int(v[16]), "cycle_found_at_pass": int(v[17]), "cycle_passes_skipped": int(v[18]), "upload_link_bytes": int(v[19]),
                "eager_range_launches": int(v[20]), "rowmajor_upload": int(v[21]),
                "csc_upload": int(v[22]), "csc_nnz": int(v[23]), "resident_dtype": int(v[24]),
                "k1_slot_order": int(v[25]), "k1_half_tiles_separated": int(v[26]), "csc_device": int(v[27]),
                "k1_unslot_form": int(w[28]), "contrast_treat": int(w[29]), "k1_slot_sides": int(w[30]),
                "masked_build": int(w[31]), "k1_slot_slice": int(w[32]), "planes_on_demand": int(w[33]),
                "perm_batch": int(w[34]), "perm_kernel_us": int(w[35]),
                "top_pairs_hist_us": int(w[36]), "top_pairs_emit_us": int(w[37]),
                "top_pairs_null_batch": int(w[38]), "top_pairs_null_us": int(w[39]),
                "top_pairs_loo_words_us": int(w[40]), "top_pairs_loo_select_us": int(w[41]),
                "top_partners_count_us": int(w[42]), "top_partners_select_us": int(w[43]),
                "top_partners_null_batch": int(w[44]), "top_partners_null_us": int(w[45])}
