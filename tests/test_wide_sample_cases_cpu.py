"""The wide sample layouts (tests/wide_sample_cases.py), the parts that need no GPU: the conditions under which tests/test_gpu_wide_samples.py
means something, asserted from the numpy oracle -- block and chunk counts, all nine classes, pairs tied in more than 64 samples of a group,
counts above 255, columns that differ -- and two cross-checks of the references themselves: the per-sample restatement against the oracle's
pair counts, and the numpy slot map against sc_slot_map of csrc/sample_counts.h (the stand-alone driver, under the sanitizers)."""
import os
import subprocess

import numpy as np
import pytest

import masked_pairs_cases as mpc
import perm_null_cases as pnc
import sample_counts_cases as scc
import wide_sample_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = 0x1FF
SEED = 11   # the context seed of the query tests (tests/test_gpu_sample_counts.py, open_ctx)


def oracle_codes(rn, name, k, G=wc.G_QUERY):
    gid = wc.gid_of(name)
    sizes = wc.sizes_of(name)
    thr = (rn.threshold(int(sizes[k]), wc.QUERY_PVAL_REO), rn.threshold(int(sizes.sum() - sizes[k]), wc.QUERY_PVAL_REO))
    return rn.build_codes(wc.int_ties(name, G, wc.QUERY_SEED, k), gid, sizes.size, k, thr, SEED)


@pytest.mark.parametrize("name", list(wc.LAYOUTS))
def test_blocks_and_chunks_are_those_of_the_table(name):
    sizes, shuffled, _, nblk, chunks = wc.LAYOUTS[name]
    gid = wc.gid_of(name)
    assert sorted(wc.sizes_of(name).tolist()) == sorted(sizes) and gid.size == sum(sizes)
    first = [int(np.flatnonzero(gid == g)[0]) for g in range(len(sizes))]
    assert first == sorted(first) and gid[0] == 0                                # ids in order of first appearance
    per_group, total, per_chunk = wc.blocks_of(name)
    m = wc.slot_map(name)
    assert total == nblk == m.size // 32 == sum((n + 31) // 32 for n in sizes) and m.size % 32 == 0 and per_chunk == chunks
    assert nblk >= 10 and len(chunks) in (2, 3)
    assert sorted(m[m >= 0].tolist()) == list(range(gid.size)) and int((m < 0).sum()) == 32 * nblk - gid.size
    if shuffled:
        assert (np.diff(gid) != 0).sum() > len(sizes)                            # the slot map is not the identity
    if name == "seam_in_group":                                                  # block 8, where the second chunk starts, lies inside group 1
        assert per_group == [5, 5] and (m < 0).sum() > 0 and chunks[-1] < wc.CHUNK_BLOCKS
    if name == "full_blocks":
        assert (m >= 0).all() and per_group == [8, 8]                            # no padding slot; the chunk seam is the group seam
    if name == "three_groups":
        assert max(per_group) > wc.CHUNK_BLOCKS
    if name == "mostly_padding":
        assert chunks[-1] == 1 and (m < 0).mean() > 0.8 and per_group == [1] * 17


@pytest.mark.parametrize("name,k", wc.query_cases())
def test_every_class_occurs_and_the_sample_columns_differ(rn, name, k):
    G = wc.G_QUERY
    code = oracle_codes(rn, name, k)
    off = ~np.eye(G, dtype=bool)
    seen = np.bincount(code[off], minlength=9)
    assert seen.size == 9 and seen.min() >= 100, seen.tolist()                   # all nine classes, none of them rare
    X = wc.int_ties(name, G, wc.QUERY_SEED, k)
    q = np.arange(0, G, 13)
    n_sel, n_gt, n_eq = scc.expected_counts(X, lambda i: code[i], q, ALL, np.ones(G, dtype=bool))
    S = X.shape[1]
    assert len({tuple(c) for c in n_gt.T.tolist()}) > S // 2                    # a swapped or shifted column shows
    assert n_eq.sum() > 0 and (n_sel == G - 1).all()


@pytest.mark.parametrize("name,k", [("seam_in_group", 0), ("mostly_padding", None)])
def test_sample_counts_restatement_sums_to_the_oracles_pair_counts(rn, name, k):
    """sample_counts_cases.expected_counts, summed over the samples of a group, is oracle.reo_numpy.pair_counts summed over the selected
    partners: two restatements that share no code, at the wide layouts"""
    G = wc.G_QUERY
    k = wc.group_of_size(name, 30) if k is None else k
    gid = wc.gid_of(name)
    ng = int(gid.max()) + 1
    X = wc.int_ties(name, G, wc.QUERY_SEED, k)
    code = oracle_codes(rn, name, k)
    pm = np.random.default_rng(5).random(G) < 0.7
    q = np.arange(G)
    gt, eq = rn.pair_counts(X, gid, ng)
    for mask in (ALL, 0x44):
        n_sel, n_gt, n_eq = scc.expected_counts(X, lambda i: code[i], q, mask, pm)
        sel = np.stack([scc.selection(code[i], mask, pm) for i in q])
        assert np.array_equal(n_sel, sel.sum(axis=1)) and n_sel.sum() > 0
        for g in range(ng):
            assert np.array_equal(n_gt[:, gid == g].sum(axis=1), (gt[:, :, g] * sel).sum(axis=1)), (mask, g)
            assert np.array_equal(n_eq[:, gid == g].sum(axis=1), (eq[:, :, g] * sel).sum(axis=1)), (mask, g)


def test_pairs_tied_in_more_than_64_samples_of_a_group(rn):
    """the tie-rich tables of G_TABLE genes: tie_wins (csrc/tie_coin.h) takes the second 64-bit word of its stream"""
    G = wc.G_TABLE
    upper = np.triu(np.ones((G, G), dtype=bool), 1)
    for name in ("seam_in_group", "full_blocks"):
        gid = wc.gid_of(name)
        _, eq = rn.pair_counts(wc.int_ties(name, G, wc.TABLE_SEED[name], 0, pattern=False), gid, 2)
        n = int(((eq.max(axis=2) > 64) & upper).sum())
        assert n >= (100 if name == "full_blocks" else 1), (name, n)
    # under the 30 % mask of the masked build's test the complete gene 1 still has such pairs on full_blocks
    name = "full_blocks"
    V = wc.random_valid(name, G, 7)
    n_gt, n_eq, n_av = mpc.masked_counts(wc.int_ties(name, G, wc.TABLE_SEED[name], 0, pattern=False), V, wc.gid_of(name), 2)
    assert ((n_eq.max(axis=2) > 64) & upper).any() and n_av.max() == 256 and n_av[upper].min() == 0


def test_contrast_counts_above_255_in_two_planes(rn):
    name, G = "contrast_groups", wc.G_CONTRAST
    gid = wc.gid_of(name)
    a, b = wc.group_of_size(name, 300), wc.group_of_size(name, 260)
    gt, eq = rn.pair_counts(wc.planted_ties(name, G, wc.QUERY_SEED), gid, 3)
    upper = np.triu(np.ones((G, G), dtype=bool), 1)
    assert ((gt[:, :, a] > 255) & (gt[:, :, b] > 255) & upper).sum() > 100        # the high byte of both counts of one pair
    assert (eq[:, :, a][upper] > 64).any()
    X = wc.ranks(name, G, wc.QUERY_SEED, effect_group=a)
    assert (np.sort(X, axis=0) == np.arange(G)[:, None]).all()                    # still a permutation per sample
    gt, eq = rn.pair_counts(X, gid, 3)
    assert ((gt[:, :, a] > 255) & (gt[:, :, b] > 255) & upper).sum() > 100 and not eq[upper].any()
    assert gt[:30, 60:, a].mean() / 300 > gt[:30, 60:, b].mean() / 260 + 0.3      # the planted genes are up in group a alone


def test_pair_support_counts_above_255(rn):
    gid = wc.gid_of("three_groups")
    gt, _ = rn.pair_counts(wc.int_ties("three_groups", wc.G_QUERY, wc.QUERY_SEED, 0), gid, 3)
    assert gt[:, :, wc.group_of_size("three_groups", 300)].max() > 255


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("wide_samples") / "sample_counts_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "rankcompv3.jl_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "sample_counts_driver.cpp")])
    return exe


@pytest.mark.parametrize("name", ["mostly_padding", "three_groups"])
def test_numpy_slot_map_is_sc_slot_map(driver, name):
    """perm_null_cases.slot_map (and with it pack_words) against csrc/sample_counts.h on 17 groups of one block and on a group of ten"""
    gid = wc.gid_of(name)
    ng = int(gid.max()) + 1
    run = subprocess.run([driver, "map", str(ng), str(gid.size)], input=" ".join(map(str, gid.tolist())) + "\n", capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert len(lines) == 2 and lines[1].startswith("ok ")
    got = np.array(lines[0].split(), dtype=np.int32)
    assert np.array_equal(got, pnc.slot_map(gid, ng)) and got.size == 32 * wc.LAYOUTS[name][3]
    rows = pnc.shuffled_rows(gid, 0, 3, 1)
    aw, live = pnc.pack_words(rows, gid, ng)
    assert np.array_equal(live, np.array([sum(1 << s for s in range(32) if got[32 * b + s] >= 0) for b in range(got.size // 32)], dtype=np.uint32))
    assert [sum(bin(int(w)).count("1") for w in r) for r in aw] == rows.sum(axis=1).tolist()
