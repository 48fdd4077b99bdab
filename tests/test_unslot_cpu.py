"""The word forms of the column un-permute (csrc/k1_slots.h: unslot_*; kernels.hip, k1_unslot_words) without a GPU:
tests/k1_unslot_driver.cpp, a stand-alone program built with AddressSanitizer and UBSan, runs the serial host model of the kernel -- its
own steps through the functions the kernel uses -- against slot_unpermute_row: random, identity and reversed orders, both forms, 2 to
9 000 genes, last groups of 1, R - 1 and R rows, padding slots and zeroed columns; the LDS index (one entry per slot, inside the bytes the
rule reports, neighbouring words on different banks); the form chosen at 25 600, 26 624, 38 912, 39 936 and 65 536 slots; the workgroup size."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_unslot_rules_driver_under_sanitizers(tmp_path):
    exe = str(tmp_path / "k1_unslot_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "rankcompv3.jl_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "k1_unslot_driver.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.splitlines()
    assert [l.split()[:2] for l in lines] == [["ok", n] for n in ("transposes", "random", "identity", "reversal", "lds_index", "form")], run.stdout
    form = lines[-1].split()
    by = dict(zip(form[2::2], (int(v) for v in form[3::2])))
    # 33 words per 32 slots (wide), 17 per 32 (narrow); 640 words (20 480 slots) in one trip of 640 threads, 1 056 in two of 576 with a partial second
    assert by == {"wide_bytes_38912": 38912 // 32 * 132, "narrow_bytes_65536": 65536 // 32 * 68, "threads_640": 640, "threads_1056": 576}, run.stdout
    assert by["wide_bytes_38912"] <= 160 * 1024 and by["narrow_bytes_65536"] <= 160 * 1024
