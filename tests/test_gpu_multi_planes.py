"""The forms of the pair kernel that a run with more than two groups takes, and the workgroup form of two groups, at 15 and 16 position
planes -- the instantiations that launch_pairs<15> and launch_pairs<16> (csrc/kernels.hip) select:

  (a) k1w_group_counts<NB, TIES> + k1_classify<kRJ>     more than two groups, shared count planes (the default)
  (b) k1_classify_contrast<kRJ>                         reo_build_pairs_contrast on those planes
  (c) k1_pairs<NB, TIES, true>                          REO_SHARE_GROUP_COUNTS=0, or planes that do not fit: every comparison recounted
  (d) k1_group_counts<NB, TIES> + k1_classify<kRJTies>  more than two groups with REO_K1_WAVE=0
      k1_pairs<NB, TIES, false>                         two groups with REO_K1_WAVE=0
  (e) the passes on a table of (a) and of (b); (f) two shards of (a)
  (g) k1w_pairs_wide<15, TIES>                          two groups, more than 65 535 samples
      k1_pairs_wide<15, TIES, false>                    ... with REO_K1_WAVE=0
      k1_pairs_wide<15, true, true>                     three groups, more than 65 535 samples (REO_K1_WAVE=0 selects the same instantiation)

at the gene counts, layouts and matrices of tests/multi_plane_cases.py: 4 096, 4 097, 9 000 and 32 767 genes run NB = 15, 32 768 and 65 535
run NB = 16, `free` runs TIES = false and `counts` TIES = true.  In count_pass the number of pos-plane quarters is (NB + 3) / 4: 4 here,
3 at the 12 planes of every earlier run of (c) and (d).  Every comparison of codes and tallies is an equality, on the rectangles, the
four column strips and the three row strips of multi_plane_cases.blocks against the thin references of that file;
tests/test_multi_plane_cases_cpu.py holds the references to the whole-table oracle on small cases and shows that no chain that ignored
planes 12 and up (15, at 65 535 genes) could match a rectangle.  Which form ran is read from info() as far as info() tells:
shared_group_counts, group_count_bytes, has_ties, Gp, and chunk_j = 256 x the genes per lane of the form
(tests/sharding_mirror.genes_per_lane).  That separates every form from the default but one: tie-free, the workgroup forms take four genes
per lane as the wave forms do, so for k1_group_counts<15, false> in (d) and for k1_pairs<NB, false, false> nothing but REO_K1_WAVE=0, which
the context reads when it is created, says that the workgroup kernel ran (info() has no field for the switch or for the item count).

At 65 535 genes with three groups the count planes are 34 GB and the class table 2.1 GB: one context at a time (Shared.close), and
trim_memory after each.

(g) runs 4 200 genes on 65 536 Int32 samples, a side of 2 048 sample blocks: count_pass_wide with four pos-plane quarters, the wave form's
count loop in two runs of blocks; the cells are the rectangles and two strips of 8 columns, the reference counts every sample of them.
Not run: 16 planes with more than 65 535 samples, which would take a host matrix of at least 8.6 GB and is out of scope (DESIGN.md,
section 7)."""
import numpy as np
import pytest

import big_plane_cases as bp
import multi_plane_cases as mc
import sharding_mirror
from test_gpu_big_planes import P_ATOL, STAT_RTOL, _check_result, _p_error, _stat_error   # the tolerances of the passes: those of that file

pytestmark = pytest.mark.gpu

class Shared:
    """Owner of the one long-lived context of the module, and of what the default form built on it.  context(ref): the context of a
    three-group case in the default form with every comparison built once, in the order K_ORDER -- the first build counts the planes
    (k1w_group_counts), each one classifies from them; the checks (a), (b), (e) of a case follow each other and find it open.  It keeps
    what the tables held on the blocks, and their tallies over ref_set(G), since later checks build other tables on the context.
    default_tables(ref): those readings, for (d) as well; a run that selects a test of (d) alone pays the default build of its case here
    (34 GB of planes at 65 535 genes), and the context is closed before (d) opens its own.  close(): before any other context is opened --
    at 65 535 genes with three groups never two at once"""

    def __init__(self, pkg):
        self.pkg, self.key, self.ctx, self.default = pkg, None, None, {}

    def close(self):
        if self.ctx is not None:
            self.ctx.close()
            self.key, self.ctx = None, None
            self.pkg._ffi.trim_memory()     # (up to 36 GB went back to the block cache: return it to the driver)

    def context(self, ref):
        key = (ref.G, ref.kind, ref.layout)
        if self.key != key:
            self.close()
            self.ctx = _open(self.pkg, ref)
            self.key = key
            tables, tallies = {}, {}
            for k in ref.ks:
                self.ctx.build_pairs(k)
                info = _form(self.ctx, ref, "wave", shared=True)
                assert info["contrast_treat"] == -1
                tables[k] = _read_blocks(self.ctx, ref)
                tallies[k] = self.ctx.tally(bp.ref_set(ref.G))
            self.default[key] = (tables, tallies)
        return self.ctx

    def default_tables(self, ref):
        """({k: {block: codes}}, {k: tally over ref_set}) as the default form built them"""
        key = (ref.G, ref.kind, ref.layout)
        if key not in self.default:
            self.context(ref)
        return self.default[key]


@pytest.fixture(scope="module")
def shared(pkg):
    owner = Shared(pkg)
    yield owner
    owner.close()


def _open(pkg, ref):
    ctx = pkg.Context(device=0, seed=ref.seed)
    ctx.set_matrix(ref.X)
    ctx.set_groups(ref.gid, ref.ngroups)
    thr = ctx.compute_thresholds(mc.PVAL_REO)
    assert np.array_equal(thr, ref.thr), (thr, ref.thr)
    return ctx


def _form(ctx, ref, form, shared):
    """which kernels ran, as far as info() tells: the tie form, the pad, the genes per lane of the form, shared planes or none"""
    info = ctx.info()
    want_bytes = (ref.ngroups + 1) * ref.Gp * ref.Gp * 2 if shared else 0
    got = (info["has_ties"], info["Gp"], info["chunk_j"], info["shared_group_counts"], info["group_count_bytes"])
    assert got == (ref.has_ties, ref.Gp, 256 * sharding_mirror.genes_per_lane(bool(ref.has_ties), form), int(shared), want_bytes), (form, info)
    return info


def _read_blocks(ctx, ref):
    return {name: ctx.get_codes(*block) for name, block in ref.blocks.items()}


# ---- (a), (b), (e): the shared count planes, one context per case

def _tables(shared, ref):
    """(a) every comparison on every block against the reference, and tally(ref_set) against the tallies of the reference's column strips"""
    tables, tallies = shared.default_tables(ref)
    assert list(tables) == list(mc.K_ORDER) != [0, 1, 2]
    for k in ref.ks:
        mc.check_same_tables(tables[k], ref.codes[k], ref.blocks, f"{ref.G} {ref.kind} {ref.layout} k {k}")
        bp.check_tally(tallies[k], bp.ref_set_tally(mc.column_strips(ref, k)), what=f"{ref.G} {ref.kind} {ref.layout} k {k} tally(ref_set)")


def _contrasts(shared, ref):
    """(b) four ordered contrasts from the planes of (a): codes, contrast_treat, the tally; then comparison 1 again, which must be the
    table of (a) -- and the planes are those of (a), not recounted: group_count_bytes stays"""
    ctx = shared.context(ref)
    tables, _ = shared.default_tables(ref)
    for c, t in ref.contrasts:
        ctx.build_contrast(c, t)
        info = _form(ctx, ref, "wave", shared=True)
        assert info["contrast_treat"] == t
        mc.check_table(ctx.get_codes, ref, (c, t), f"{ref.G} {ref.kind} {ref.layout}")
        bp.check_tally(ctx.tally(bp.ref_set(ref.G)), bp.ref_set_tally(mc.column_strips(ref, (c, t))), what=f"contrast {(c, t)} tally(ref_set)")
    ctx.build_pairs(1)
    assert _form(ctx, ref, "wave", shared=True)["contrast_treat"] == -1
    mc.check_same_tables(_read_blocks(ctx, ref), tables[1], ref.blocks, "comparison 1 after the contrasts")


def _passes(shared, ref):
    """(e) identify_degs on the table of comparison 1 and on the contrast (2, 1), as test_passes_at_18_planes: three passes against the
    oracle's iteration over the device's own tally (which (a) and (b) hold to the reference), and one pass against the oracle's pass over
    the tallies of the reference's strips, with nothing of the device's in it"""
    ctx, G = shared.context(ref), ref.G
    ref0 = bp.ref_set(G)
    for table in (1, (2, 1)):
        if table == 1:
            ctx.build_pairs(1)
        else:
            ctx.build_contrast(*table)
        got = ctx.identify_degs(ref0, 1.0, 0.05, 3, 0)
        mask = ctx.ref_mask()                                          # (reo_tally drops the run's mask: first)
        exp = bp.reference_run(ctx.tally, G, ref0, 1.0, 0.05, 3, 0)
        print(G, ref.kind, table, "passes", got[1], "trace", got[2], "reference", exp[1], exp[2])
        print("largest error of p / padj", _p_error(got[0], exp[0]), "of", P_ATOL, "; of the statistics, relative", _stat_error(got[0], exp[0]), "of", STAT_RTOL)
        bp.check_run(got, exp, _check_result, f"{G} {ref.kind} {table}")
        assert _p_error(got[0], exp[0]) <= P_ATOL
        bp.check_tally(ctx.tally(mask), got[0][:, 2:11].astype(np.int32), what=f"{table} tally(ref_mask)")
        one = ctx.identify_degs(ref0, 1.0, 0.05, 1, 0)
        cont = bp.ref_set_tally(mc.column_strips(ref, table))
        bp.check_run(one, bp.reference_run(lambda m: cont, G, ref0, 1.0, 0.05, 1, 0), _check_result, f"{G} {ref.kind} {table}, one pass")


SHARED_RUN = [(what, case) for case in mc.SHARED_CASES for what in ("tables", "contrasts", "passes")
              if what == "tables" or (what == "contrasts" and case[0] in mc.CONTRAST_G) or (what == "passes" and case in mc.PASS_CASES)]


def _id(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("what,case", SHARED_RUN, ids=_id)
def test_shared_group_counts(shared, oracle, what, case):
    """(a) tables, (b) contrasts, (e) passes: the checks of one case follow each other and run on one context"""
    ref = mc.reference(oracle, *case)
    if what == "tables":
        _tables(shared, ref)
    elif what == "contrasts":
        _contrasts(shared, ref)
    else:
        _passes(shared, ref)


# ---- (c): every comparison recounted

@pytest.mark.parametrize("case", mc.RECOUNT_CASES, ids=_id)
def test_comparisons_recounted_by_the_workgroup_form(pkg, shared, oracle, monkeypatch, case):
    """(c) REO_SHARE_GROUP_COUNTS=0: k1_pairs<NB, TIES, true>, count_pass with four pos-plane quarters; what a run takes whose planes do
    not fit the device (30 groups at 60 000 genes)"""
    monkeypatch.setenv("REO_SHARE_GROUP_COUNTS", "0")
    ref = mc.reference(oracle, *case)
    shared.close()
    with _open(pkg, ref) as ctx:
        for k in ref.ks:
            ctx.build_pairs(k)
            _form(ctx, ref, "wg", shared=False)
            mc.check_table(ctx.get_codes, ref, k, f"recount {case}")
    pkg._ffi.trim_memory()


# ---- (d): the workgroup forms behind REO_K1_WAVE=0

@pytest.mark.parametrize("case", mc.WG_COUNT_CASES, ids=_id)
def test_workgroup_group_counts(pkg, shared, oracle, monkeypatch, case):
    """(d) REO_K1_WAVE=0 with three groups: k1_group_counts<NB, TIES> makes the planes, k1_classify<kRJTies> (tie-free: <kRJ>) reads them.
    The tables of (a) cell for cell on every block, and the reference"""
    ref = mc.reference(oracle, *case)
    tables, tallies = shared.default_tables(ref)
    shared.close()
    monkeypatch.setenv("REO_K1_WAVE", "0")
    with _open(pkg, ref) as ctx:
        for k in ref.ks:
            ctx.build_pairs(k)
            _form(ctx, ref, "wg", shared=True)
            got = mc.check_table(ctx.get_codes, ref, k, f"REO_K1_WAVE=0 {case}")
            mc.check_same_tables(got, tables[k], ref.blocks, f"REO_K1_WAVE=0 against the default form, {case} k {k}")
            bp.check_tally(ctx.tally(bp.ref_set(ref.G)), tallies[k], what=f"REO_K1_WAVE=0 {case} k {k} tally(ref_set)")
    pkg._ffi.trim_memory()


@pytest.mark.parametrize("case", mc.WG_TWO_CASES, ids=_id)
def test_workgroup_form_of_two_groups(pkg, shared, oracle, monkeypatch, case):
    """(d) REO_K1_WAVE=0 with two groups: k1_pairs<NB, TIES, false>, the cross-check of the wave form, against expected_codes(..., 2, 0)"""
    monkeypatch.setenv("REO_K1_WAVE", "0")
    ref = mc.reference(oracle, *case)
    assert ref.ngroups == 2 and ref.thr.tolist() == [[7, 7], [7, 7]]
    shared.close()
    with _open(pkg, ref) as ctx:
        ctx.build_pairs(0)
        info = _form(ctx, ref, "wg", shared=False)
        assert info["k1_slot_order"] == 0, info
        mc.check_table(ctx.get_codes, ref, 0, f"REO_K1_WAVE=0 {case}")
        bp.check_tally(ctx.tally(bp.ref_set(ref.G)), bp.ref_set_tally(mc.column_strips(ref, 0)), what=f"REO_K1_WAVE=0 {case} tally(ref_set)")
    pkg._ffi.trim_memory()


# ---- (f): two shards

@pytest.mark.parametrize("case", mc.SHARD_CASES, ids=_id)
def test_two_shards_add_up_at_15_planes(pkg, shared, oracle, case):
    """(f) the last part of test_shared_group_counts_equal_recounting at 9 000 genes: each shard counts the planes of its own work units
    and classifies comparison 1, then comparison k; the shards' raw counters over the column strips -- no whole table is read back -- add
    up to the tallies of the unsharded table.  A cell belongs to one shard only: in the other's table it is class 4"""
    ref = mc.reference(oracle, *case)
    shared.close()
    ref0 = bp.ref_set(ref.G)
    for k in (2, 0):
        tot, owned, cells = 0, [], [0] * 4
        for rank in range(2):
            with _open(pkg, ref) as ctx:
                ctx.set_shard(rank, 2)
                ctx.build_pairs(1)
                ctx.build_pairs(k)
                info = _form(ctx, ref, "wave", shared=True)
                owned.append(info["tiles_owned"])
                with pytest.raises(pkg.ReoError):
                    ctx.tally(ref0)                  # REO_ECOMM: nothing has exchanged the table
                strips = {j0: ctx.get_codes(0, ref.G, j0, j0 + bp.STRIP) for j0 in bp.ref_runs(ref.G)}
            tot = tot + mc.strips_raw_counters(strips, sharding_mirror)
            cells = [n + ((c != 4) & (c != 255)) for n, c in zip(cells, strips.values())]
        assert min(owned) > 0 and sum(owned) == info["tiles_total"], (owned, info)
        exp = mc.column_strips(ref, k)
        assert all(np.array_equal(cells[j] > 0, (exp[j0] != 4) & (exp[j0] != 255)) and cells[j].max() == 1 for j, j0 in enumerate(exp)), k
        bp.check_tally(sharding_mirror.derive_tallies(tot, ref0), bp.ref_set_tally(exp), what=f"two shards, {case} k {k}")
    pkg._ffi.trim_memory()



# ---- (g): more than 65 535 samples at 15 planes

@pytest.mark.parametrize("case", mc.WIDE_CASES, ids=_id)
def test_wide_samples_at_15_planes(pkg, shared, oracle, monkeypatch, case):
    """(g) 4 200 genes x 65 536 samples, Int32.  Two groups, tie-rich and tie-free: k1w_pairs_wide<15, TIES>, then k1_pairs_wide<15, TIES,
    false> behind REO_K1_WAVE=0 -- each against the reference, and the tables of one matrix cell for cell against each other.  Three
    groups, tie-rich: k1_pairs_wide<15, true, true>, every comparison.  chunk_j tells the wide workgroup form (one gene per lane with ties,
    two without) from the wave form (four)"""
    ref = mc.reference(oracle, *case)
    assert ref.X.dtype == np.int32 and ref.X.flags.f_contiguous and ref.X.shape == (mc.WIDE_G, 65536) and ref.Gp == 5120
    shared.close()
    tables = {}
    for form in ("wave", "wide") if ref.ngroups == 2 else ("wide",):
        if form == "wide" and ref.ngroups == 2:
            monkeypatch.setenv("REO_K1_WAVE", "0")
        with _open(pkg, ref) as ctx:
            for k in ref.ks:
                ctx.build_pairs(k)
                info = _form(ctx, ref, form, shared=False)
                assert info["S"] == 65536 and info["sample_slots"] == 65536 + 32 * (ref.ngroups - 1), info
                tables[form, k] = mc.check_table(ctx.get_codes, ref, k, f"{case} {form}")
        pkg._ffi.trim_memory()
    if ref.ngroups == 2:
        mc.check_same_tables(tables["wide", 0], tables["wave", 0], ref.blocks, "REO_K1_WAVE=0 against the wave form")
