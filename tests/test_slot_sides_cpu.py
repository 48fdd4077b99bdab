"""The per-side slot order of the pair kernel without a GPU (csrc/k1_slots.h; the rule in numpy: tests/slot_sides_cases.py).

a. What every case of tests/test_gpu_slot_sides.py is there for: the per-side rule separates STRICTLY more items than the common rule
   (slot_cases.model_count) -- a GPU test that asserts the per-side count can then not pass by running the common order -- and the
   common build of the same matrix, which the GPU tests run as the A/B partner, emits both constants (count 0 and count n_side).
   Three things the data cannot give, reasoned in slot_sides_cases' docstrings and asserted here as what they are:
   - a per-side build never separates an item with the count n_side (a later slot of a side's own order has no smaller key), so "both
     constants" is asserted for the common order of the case, and the per-side model's n_side counts are asserted to be 0;
   - where every key of one side is equal, the common key is the other side's key plus a constant: both rules give the same order on
     the levelled side and gene order on the flat one, so that case has EQUAL counts (its GPU test rests on k1_slot_sides == 2);
   - 257 genes: the second chunk holds one gene, the last of the common order, which is the highest class of side 1: only side 0 can
     have the count n_side there.
b. tests/k1_slot_sides_driver.cpp, a stand-alone program built with AddressSanitizer and UBSan: the per-side host rank (32-bit keys),
   invert and ranges against brute force, and the pair form of the word un-permute against slot_unpermute_row with two different maps,
   at 2, 33, 257, 1 000, 2 049 and 65 535 genes, R = 4 and 8, tail groups included."""
import os
import subprocess

import numpy as np
import pytest

import slot_cases as sc
import slot_sides_cases as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(ss.CASES))
def test_cases_are_what_they_are_for(name):
    X, side, gid, k = ss.case(name)
    G = X.shape[0]
    assert X.min() >= 0 and X.max() < 2 ** 24
    assert all(np.unique(X[:, s]).size == G for s in range(0, X.shape[1], max(1, X.shape[1] // 4))), "tie-free inside a sample"
    assert gid[0] == 0 and np.array_equal(gid != k, side != 0)
    live, per_side = ss.model(X, side)
    live_c, common = sc.model(X, side)
    n_sides, n_common = ss.model_count(X, side), sc.model_count(X, side)
    print(name, "live", live, "per-side", per_side, "=", n_sides, "common", common, "=", n_common)
    assert live == live_c
    assert per_side[0][0] == 0 and per_side[1][0] == 0, "a side in its own order has no item with the count n_side"
    if name == "flat_side0":
        assert n_sides == n_common > 0 and per_side[0] == [0, 0] and per_side[1][1] > 0
        s2g, _ = ss.orders(X, side)
        assert np.array_equal(s2g[0], np.arange(G)), "equal keys: the gene index decides"
        assert not np.array_equal(s2g[1], np.arange(G))
        return
    assert n_sides > n_common > 0, "the per-side rule separates strictly more"
    assert per_side[0][1] > 0 and per_side[1][1] > 0, "count 0 on both sides"
    if name == "257":
        assert all(v > 0 for v in common[0]) and common[1][1] > 0, "both constants on side 0, count 0 on side 1 (common order)"
    else:
        assert all(v > 0 for z in (0, 1) for v in common[z]), "both constants on both sides (common order)"
    s2g, _ = ss.orders(X, side)
    assert not np.array_equal(s2g[0], s2g[1]), "two different orders"


def test_rule_by_blocks():
    assert [ss.sides_by_rule(*n) for n in ((7 * 32, 8 * 32), (8 * 32, 8 * 32), (15 * 32, 32), (7 * 32 + 1, 8 * 32), (2, 2))] == [1, 2, 2, 2, 1]


def test_slot_sides_driver_under_sanitizers(tmp_path):
    exe = str(tmp_path / "k1_slot_sides_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "rankcompv3.jl_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "k1_slot_sides_driver.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.splitlines()
    assert [l.split()[:2] for l in lines] == [["ok", n] for n in ("bits", "rule", "maps", "pair_form")], run.stdout
    assert int(lines[2].split()[3]) > 0, run.stdout
