"""The index rules of the pair kernel's slot order (csrc/k1_slots.h) without a GPU: tests/k1_slots_driver.cpp, a stand-alone program
built with AddressSanitizer and UBSan, checks on random levelled data that the order is a permutation sorted by (key, gene), that
g2s o s2g is the identity, that the separation predicate agrees with the genes' own ranges and never fires for a tile inside its chunk,
and that un-permuting a table row and permuting it again is the identity (G not a multiple of 32 included)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_slot_rules_driver_under_sanitizers(tmp_path):
    exe = str(tmp_path / "k1_slots_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "rankcompv3.jl_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "k1_slots_driver.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.splitlines()
    assert [l.split()[:2] for l in lines] == [["ok", n] for n in ("levels64", "odd_G", "tiny", "one_level", "equal_keys")], run.stdout
    by = {l.split()[1]: (int(l.split()[5]), int(l.split()[7])) for l in lines}   # name -> (live, separated)
    assert by["levels64"][1] > by["levels64"][0] // 2 and by["tiny"][1] == 0, run.stdout
