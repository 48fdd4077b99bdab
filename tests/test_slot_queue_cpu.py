"""The index rules of the pair kernel's item queues (csrc/k1_queue.h) without a GPU: tests/k1_queue_driver.cpp, a stand-alone program
built with AddressSanitizer and UBSan, lets W simulated workers draw from the eight counters in a randomly interleaved order, with
stealing, and checks that every list index 0 .. n-1 is taken exactly once and none beyond, for n in {0, 1, 7, 8, 9, 1 000, 51 946} and
W in {1, 8, 13, 3 072}, and that the queue lengths sum to n."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_queue_rules_driver_under_sanitizers(tmp_path):
    exe = str(tmp_path / "k1_queue_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "rankcompv3.jl_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "k1_queue_driver.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    cases = [l.split()[:3] for l in run.stdout.splitlines()]
    assert cases == [["ok", str(n), str(w)] for n in (0, 1, 7, 8, 9, 1000, 51946) for w in (1, 8, 13, 3072)], run.stdout
