"""The slot form's operands sliced straight from the 16-bit position rows, without a GPU (csrc/k1_slots.h: slot_slice_*).

tests/k1_slot_slice_driver.cpp, a stand-alone program built with AddressSanitizer and UBSan: the host model of k1_slot_slice against the
composed host models of what it replaces -- t_slice's two plane layouts written one bit at a time, then k1_slot_gather's copy by the
launch's block ranges -- at 2, 33, 257, 1 000 (padded to 1 024), 2 049 and 65 535 genes, two different maps, side 0 first and side 1
first (and in the middle), padding sample slots and padded genes zero, all 16 plane words with the record layout's skew; and the form
the kernel runs, by genes through g2s, against the rule by slots."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_slot_slice_driver_under_sanitizers(tmp_path):
    exe = str(tmp_path / "k1_slot_slice_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "rankcompv3.jl_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "k1_slot_slice_driver.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    words = run.stdout.split()
    assert words[:4] == ["ok", "slice", "cases", "13"], run.stdout
    assert int(words[5]) > 0, run.stdout
