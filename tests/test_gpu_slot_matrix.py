"""The slot order of the pair kernel (kernels.hip: k1_slot_part .. k1_slot_gather, k1w_pairs_slots with emit_constant, k1_unslot_columns)
along the axes that tests/test_gpu_slot_order.py and tests/test_gpu_slot_queue.py hold fixed: sides of different size and block count,
comparison 1 of two groups, shuffled and split labels, every input form, the sizes at which the column un-permute changes its rows per
workgroup, degenerate keys and tiny problems, one context through slot and identity builds, and a differential sweep on levelled data.

The cases and the rule in numpy live in tests/slot_cases.py; tests/test_slot_cases_cpu.py asserts on the CPU that each case separates
what it is there for.  Every case here asserts info()["k1_slot_order"] == 1 and, where the model is affordable, that
info()["k1_half_tiles_separated"] is twice the model's count; the class table is compared with the oracle's (comparison k: group k is the
control side, thresholds thr[:, k]) and / or with that of a context created under REO_K1_SLOTS=0.

emit_constant's `else return` (a constant count that is neither >= hi_thr nor <= n_side - hi_thr) cannot be reached through the API:
reo_compute_thresholds gives n / 2 < thr <= n for every side size and pval_reo (test_slot_cases_cpu.py asserts it), so a count of 0 or
n_side always has a class.  No case here pretends to reach it."""
import numpy as np
import pytest

import sample_counts_cases as scc
import slot_cases as sc
from test_gpu_pair_list import expected as pl_expected, same as pl_same
from test_gpu_parity import _expected_block_codes
from test_gpu_sample_counts import same as sc_same

pytestmark = pytest.mark.gpu

ALL = 0x1FF
ENV = ("REO_K1_SLOTS", "REO_K1_WORKERS", "REO_K1_QUEUE", "REO_ROWMAJOR")


def _env(monkeypatch, **kw):
    """the four variables these tests touch: unset, or as given (slots=0, workers=13, queue=0, rowmajor=1)"""
    for name in ENV:
        v = kw.get(name[4:].lower().replace("k1_", ""))
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


def _host(X):
    return lambda ctx: ctx.set_matrix(np.asfortranarray(X))


def _open(pkg, load, gid, ngroups, pval_reo, seed):
    """a context with the matrix FIRST (groups first would pair the sides as they arrive: the pipelined upload, identity order)"""
    ctx = pkg.Context(device=0, seed=seed)
    try:
        keep = load(ctx)
        ctx.set_groups(gid, ngroups)
        ctx.compute_thresholds(pval_reo)
    except BaseException:
        ctx.close()
        raise
    ctx._slot_test_keep = keep
    return ctx


def _where(got, exp, X, side):
    """where two class tables differ: rows, columns, which side's planes (code = 3 ic + it: ic sits in the control side's two planes, it in
    the other side's), and how many of the differing pairs lie, by the model, in a separated item of either side"""
    i, j = np.nonzero(got != exp)
    if not i.size:
        return "equal"
    G = X.shape[0]
    key, _ = sc.extremes(X, side)
    g2s = np.empty(G, dtype=np.int64)
    g2s[np.lexsort((np.arange(G), key))] = np.arange(G)
    _, sep = sc.masks(X, side)
    t, q = np.minimum(g2s[i], g2s[j]) // sc.TILE, np.maximum(g2s[i], g2s[j]) // sc.CHUNK   # the item that counts the pair: tile of the lower slot, chunk of the higher
    g, e = got[i, j].astype(int), exp[i, j].astype(int)
    inside = {z: int((sep[z][0][t, q] | sep[z][1][t, q]).sum()) for z in (0, 1)}
    return (f"{i.size} codes differ: rows {i.min()}..{i.max()}, columns {j.min()}..{j.max()}, slot tiles {t.min()}..{t.max()}, chunks {q.min()}..{q.max()}; "
            f"side 0 planes differ in {int((g // 3 != e // 3).sum())}, side 1 planes in {int((g % 3 != e % 3).sum())}; in a separated item of side 0: "
            f"{inside[0]}, of side 1: {inside[1]}; first (i, j, got, want): {list(zip(i[:6].tolist(), j[:6].tolist(), g[:6].tolist(), e[:6].tolist()))}")


def _whole_table(pkg, oracle, monkeypatch, X, side, k, pval_reo, seed, load=None, identity=True, flag=None, **env):
    """One case: the slot build of comparison k against the model's count, the oracle's table and tallies and (identity) the table of a
    context created under REO_K1_SLOTS=0.  X: the matrix as integers (the oracle reads it widened); load: how the context gets it."""
    G = X.shape[0]
    gid = sc.gid_of(side, k)
    separated = sc.model_count(X, side)
    load = load or _host(X)
    ref_masks = [np.ones(G, dtype=bool), pkg.synth.ref_mask(G, G // 7, seed)]
    _env(monkeypatch, **env)
    with _open(pkg, load, gid, 2, pval_reo, seed) as ctx:
        if flag:
            assert ctx.info()[flag] == 1, flag
        thr = ctx.get_thresholds()
        ctx.build_pairs(k)
        info = ctx.info()
        print("separated items by the model", separated, "k1_slot_order", info["k1_slot_order"], "k1_half_tiles_separated", info["k1_half_tiles_separated"],
              "thresholds", thr[:, k].tolist())
        assert info["k1_slot_order"] == 1 and info["has_ties"] == 0
        assert info["k1_half_tiles_separated"] == 2 * separated
        got = ctx.get_codes(0, G, 0, G)
        tallies = [ctx.tally(m) for m in ref_masks]
    code = oracle.build_codes(np.asfortranarray(X.astype(np.float64)), gid, 2, k, thr[:, k].tolist(), seed)
    assert np.array_equal(got, code), "class table differs from the oracle's: " + _where(got, code, X, side)
    for m, t in zip(ref_masks, tallies):
        assert np.array_equal(t, oracle.tally(code, m)), "tallies differ from the oracle's"
    if identity:
        _env(monkeypatch, slots=0)
        with _open(pkg, load, gid, 2, pval_reo, seed) as ctx:
            ctx.build_pairs(k)
            assert ctx.info()["k1_slot_order"] == 0 and ctx.info()["k1_half_tiles_separated"] == 0
            ident = ctx.get_codes(0, G, 0, G)
        _env(monkeypatch)
        assert np.array_equal(got, ident), "class table differs from the identity order's: " + _where(got, ident, X, side)
    return got, separated


# ---- a. layouts x comparison

@pytest.mark.parametrize("k", [0, 1])
@pytest.mark.parametrize("lay", sc.LAYOUTS, ids=sc.layout_id)
def test_layouts_and_both_comparisons(pkg, oracle, monkeypatch, lay, k):
    """planted, 1 013 genes, both constants on both sides and a separated item in the last chunk, with side 0 (group k: cb, nc, m1) and side
    1 of different size, block count and padding.  Comparison 1 takes group 1 as the control side: its blocks lie BEHIND group 0's.  A swap
    of nc / nt or m1 / m2 in emit_constant, or of the sides' first slot or size in k1_slot_part, changes the table or the count here."""
    X, side, gid = sc.planted_case(lay, k)
    _, separated = _whole_table(pkg, oracle, monkeypatch, X, side, k, lay[3], seed=3)
    assert separated == 66


def test_group_ids_in_another_order_are_refused(pkg):
    """why no layout has the label of group 0 second in the file: the library numbers groups by first appearance and refuses anything else"""
    with pkg.Context(device=0, seed=1) as ctx:
        with pytest.raises(pkg.DimensionMismatch, match="first appearance"):
            ctx.set_groups(np.array([1] * 24 + [0] * 40, dtype=np.int32), 2)


# ---- b. input forms

@pytest.mark.parametrize("form", sc.FORMS)
def test_every_input_form_takes_the_slot_path(pkg, oracle, monkeypatch, form):
    """planted 1 013 x (20 + 44, shuffled), comparison 0, through every entry point with the matrix first.  Every form ends in the same
    resident matrix and the same transform, which leaves the positions by sample slot (t_pos16) that the slot front reads: slot order 1
    and the oracle's table for each.  (The oracle reads the widened values; they are exact in Float32 and Int32.)"""
    X, side, gid = sc.planted_case(sc.FORM_LAYOUT, 0)
    G, S = X.shape
    env, flag = {}, None
    if form in ("float64", "float32", "int32"):
        load = _host(X.astype(form))
    elif form == "int64_rowmajor":
        Xc = np.ascontiguousarray(X)
        assert Xc.flags.c_contiguous and not Xc.flags.f_contiguous
        load, env, flag = (lambda ctx: ctx.set_matrix(Xc)), dict(rowmajor=1), "rowmajor_upload"
    elif form in ("csc_host", "csc_device"):
        import scipy.sparse as sp
        M = sp.csc_matrix(X)
        assert M.has_canonical_format and X.size - S <= M.nnz == np.count_nonzero(X)   # every entry but the zeros: at most one per column
        if form == "csc_host":
            load, flag = (lambda ctx: ctx.set_matrix(M)), "csc_upload"
        else:
            import torch
            t = torch.sparse_csc_tensor(torch.from_numpy(M.indptr.astype(np.int32)).to("cuda:0"), torch.from_numpy(M.indices.astype(np.int32)).to("cuda:0"),
                                        torch.from_numpy(np.ascontiguousarray(M.data)).to("cuda:0"), size=M.shape)
            load, flag = (lambda ctx: ctx.set_matrix_tensor(t)), "csc_device"
    else:
        assert form == "dense_device_ld"
        from test_gpu_float32 import _device_copy

        def load(ctx):
            keep, ptr, ld = _device_copy(X, pad=8)
            assert ld > G
            ctx.set_matrix_device(ptr, G, S, ld, "i64", keepalive=keep)
            return keep
    _whole_table(pkg, oracle, monkeypatch, X, side, 0, sc.FORM_LAYOUT[3], seed=3, load=load, identity=False, flag=flag, **env)


# ---- c. sizes of the column un-permute

def _rows_per_workgroup(Gp):
    """the rule of k1_slots_back: as many table rows as fit 60 KB of LDS at 16 bytes per 32 columns, out of 6, 4, 2, 1"""
    row_bytes = Gp // 32 * 16
    return next((r for r in (6, 4, 2) if r * row_bytes <= 61440), 1)


@pytest.mark.parametrize("G,Gp,R", [(20480, 20480, 6), (20481, 21504, 4), (30720, 30720, 4), (30721, 31744, 2), (32769, 33792, 2), (61440, 61440, 2),
                                    (61441, 62464, 1), (65535, 65536, 1)])
def test_column_unpermute_at_its_size_limits(pkg, oracle, monkeypatch, G, Gp, R):
    """k1_unslot_columns<R> by the rule in k1_slots_back (no info() field reports R):
      20 480 -> R = 6 with exactly 61 440 bytes of LDS, last workgroup 2 rows;     20 481 (Gp 21 504) -> R = 4, last workgroup 1 row;
      30 720 -> R = 4 with exactly 61 440 bytes, no tail;                          30 721 (Gp 31 744) -> R = 2, last workgroup 1 row;
      32 769 (Gp 33 792; the 16-plane loop) -> R = 2, last workgroup 1 row;        61 440 -> R = 2 with exactly 61 440 bytes, no tail;
      61 441 (Gp 62 464) -> R = 1;                                                 65 535 (Gp 65 536) -> R = 1, positions up to 65 534
      next to the marker 0xFFFF of "no gene" (kSlotNoMin).
    T0 ranks x (4 + 4).  Sampled blocks -- first and last rows and columns, the diagonal, the padded tail, and the last workgroup's rows
    over the first, a middle and the last 256 columns -- and both tallies against the identity order's; the first four blocks against
    the oracle's counts with the thresholds.  Two contexts with tables of up to 2.1 GB, one after the other."""
    S, seed = 8, 13
    assert R == _rows_per_workgroup(Gp) and Gp == (G + 1023) // 1024 * 1024
    X = pkg.synth.t0_ranks(G, S, seed)
    gid, lev = pkg.encode_groups(pkg.synth.groups(S))
    tail = G % R or R
    blocks = [(0, 48, 0, 256), (0, 32, G - 256, G), (G - 40, G, 0, 128), (G - 64, G, G - 64, G), (16000, 16040, 16000, 16200), (20000, 20032, 300, 428),
              (5000, 5032, G - 3000, G - 2872), (G - tail, G, 0, 256), (G - tail, G, G // 2, G // 2 + 256), (G - tail, G, G - 256, G)]
    ref_masks = [np.ones(G, dtype=bool), pkg.synth.ref_mask(G, G // 7, seed)]
    out = {}
    for slots in (1, 0):
        _env(monkeypatch, slots=None if slots else 0)
        with _open(pkg, _host(X), gid, 2, 0.01, seed) as ctx:
            thr = ctx.get_thresholds()
            ctx.build_pairs(0)
            info = ctx.info()
            assert info["Gp"] == Gp and info["k1_slot_order"] == slots and info["has_ties"] == 0
            assert (info["k1_half_tiles_separated"] > 0) == bool(slots)
            out[slots] = ([ctx.get_codes(*b) for b in blocks], [ctx.tally(m) for m in ref_masks])
    _env(monkeypatch)
    Xf = np.asfortranarray(X.astype(np.float64))
    for b, g in zip(blocks[:4], out[1][0][:4]):
        assert np.array_equal(g, _expected_block_codes(oracle, Xf, gid, thr, seed, *b)), b
    for b, g, w in zip(blocks, out[1][0], out[0][0]):
        assert np.array_equal(g, w), b
    for g, w in zip(out[1][1], out[0][1]):
        assert np.array_equal(g, w), "tallies differ from the identity order's"
    assert out[1][1][0].sum() == G * (G - 1)   # (every ordered pair has one class)


# ---- d. degenerate keys and tiny problems

def test_all_keys_different_and_every_range_a_point(pkg, oracle, monkeypatch):
    """same_order 1 000 x (5 + 7): min == max on both sides for every gene; 48 separated items per side, all with count 0"""
    X = sc.same_order(1000, 12, 5)
    _, separated = _whole_table(pkg, oracle, monkeypatch, X, np.array([0] * 5 + [1] * 7), 0, 0.01, seed=5)
    assert separated == 96


def test_all_keys_equal(pkg, oracle, monkeypatch):
    """mirrored 1 000 x (5 + 7): one key for all genes, k1_slot_rank decides everything by the gene index, slots are genes, nothing
    separates: the table is the identity order's (and the oracle's)"""
    X, side = sc.mirrored(1000, 5, 7, 5)
    _, separated = _whole_table(pkg, oracle, monkeypatch, X, side, 0, 0.01, seed=5)
    assert separated == 0


@pytest.mark.parametrize("G", sc.TINY_G)
def test_tiny_gene_counts(pkg, oracle, monkeypatch, G):
    """same_order x (3 + 3) at 2 genes, 31 and 33 (one tile and a one-gene second tile, one chunk), 256 (one full chunk) and 257 (the last
    tile holds one gene and its chunk one slot; 16 separated items)"""
    X = sc.same_order(G, 6, 5)
    _whole_table(pkg, oracle, monkeypatch, X, np.array([0] * 3 + [1] * 3), 0, 0.01, seed=5)


# ---- e. one context, many builds

def test_one_context_through_slot_and_identity_builds(pkg, oracle, monkeypatch):
    """build_pairs(0), build_pairs(1), other group sizes on the same matrix, tie-rich data, the first matrix again, three groups, two
    groups again: slot order comes and goes with what each build is, no map, range or item list of an earlier build leaks into a later
    one, and the last table is the first one.  Then pair_list, ref_mask and sample_counts on the last (slot) build: they read the table
    and the planes in gene order."""
    G, S, seed = 1013, 64, 5
    X, side, gid = sc.planted_case(sc.FORM_LAYOUT, 0)
    Xt = pkg.synth.t1_counts(G, S, seed)
    gid_5_59 = np.array([0] * 5 + [1] * 59, dtype=np.int32)
    gid_3 = np.array([0] * 20 + [1] * 22 + [2] * 22, dtype=np.int32)
    ref_masks = [np.ones(G, dtype=bool), pkg.synth.ref_mask(G, G // 7, seed)]
    _env(monkeypatch)

    def build(ctx, X, gid, ngroups, k, slot_order, has_ties=0):
        thr = ctx.get_thresholds()
        ctx.build_pairs(k)
        info = ctx.info()
        want = 2 * sc.model_count(X, (gid != k).astype(np.int32)) if slot_order else 0
        assert (info["k1_slot_order"], info["k1_half_tiles_separated"], info["has_ties"]) == (slot_order, want, has_ties)
        code = oracle.build_codes(np.asfortranarray(X.astype(np.float64)), gid, ngroups, k, thr[:, k].tolist(), seed)
        got = ctx.get_codes(0, G, 0, G)
        assert np.array_equal(got, code), "class table differs from the oracle's" + (": " + _where(got, code, X, gid != k) if slot_order else "")
        for m in ref_masks:
            assert np.array_equal(ctx.tally(m), oracle.tally(code, m))
        return code

    def regroup(ctx, gid, ngroups):
        ctx.set_groups(gid, ngroups)
        ctx.compute_thresholds(0.01)

    with _open(pkg, _host(X), gid, 2, 0.01, seed) as ctx:
        first = build(ctx, X, gid, 2, 0, 1)                      # 1
        other = build(ctx, X, gid, 2, 1, 1)                      # 2: the sides exchanged
        assert not np.array_equal(first, other)
        regroup(ctx, gid_5_59, 2)                                # 3: another split of the same samples, no set_matrix
        build(ctx, X, gid_5_59, 2, 0, 1)
        ctx.set_matrix(np.asfortranarray(Xt)); regroup(ctx, gid, 2)
        build(ctx, Xt, gid, 2, 0, 0, has_ties=1)                 # 4: tie-rich
        ctx.set_matrix(np.asfortranarray(X)); regroup(ctx, gid, 2)
        assert np.array_equal(build(ctx, X, gid, 2, 0, 1), first)   # 5
        regroup(ctx, gid_3, 3)
        build(ctx, X, gid_3, 3, 2, 0)                            # 6: three groups, one against the rest
        regroup(ctx, gid, 2)
        assert np.array_equal(build(ctx, X, gid, 2, 0, 1), first)   # 7
        # the readers of the table and of the planes, on the slot build that has just run
        q = np.array([0, G // 2, G - 1], dtype=np.int32)
        pm = ref_masks[1]
        st = scc.states(X, q)
        for mask in (ALL, 0x44):
            pl_same(ctx.pair_list(q, mask, pm), pl_expected(lambda i: first[i], q, mask, pm), mask)
            sc_same(ctx.sample_counts(q, mask, pm), scc.expected_counts(X, lambda i: first[i], q, mask, pm, st), mask)
        result, iters, _ = ctx.identify_degs(pm, 1.0, 0.05, 4, 1)
        ref = ctx.ref_mask()
        assert iters >= 1 and np.array_equal(oracle.tally(first, ref), result[:, 2:11].astype(np.int32))
        pl_same(ctx.pair_list(q, "reversed"), pl_expected(lambda i: first[i], q, 0x44, ref))
        sc_same(ctx.sample_counts(q, "reversed"), scc.expected_counts(X, lambda i: first[i], q, 0x44, ref, st))
        assert ctx.info()["k1_slot_order"] == 1


# ---- f. differential sweep

@pytest.mark.parametrize("no", range(sc.SWEEP_CASES))
def test_sweep_on_levelled_data(pkg, oracle, monkeypatch, no):
    """24 cases from one seed (slot_cases.sweep; at least 16 of them separate something, asserted on the CPU): 257 to 1 499 genes, sides of
    2 to 69 samples, contiguous or shuffled labels, comparison 0 or 1, three values of pval_reo, four element types, worker counts 1 / 13
    / 40 / the default and both launch forms: whole table against the oracle, separated half tiles against the model."""
    cs = sc.sweep()[no]
    print({n: cs[n] for n in ("G", "n0", "n1", "k", "pval_reo", "dtype", "workers", "queue", "levels", "separated")})
    _whole_table(pkg, oracle, monkeypatch, cs["X"], cs["side"], cs["k"], cs["pval_reo"], seed=no, load=_host(cs["X"].astype(cs["dtype"])),
                 identity=False, workers=cs["workers"], queue=cs["queue"])
