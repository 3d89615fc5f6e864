"""The windows of a list of loop candidates and a round's slice of them (scl_slam_amd/csrc/candidate_windows.hpp: the offsets of a
round, rebased, with and without the loop forms' leading window) without a GPU: tests/cpp/candidate_windows_check.cpp, built by `make`
under ASan + UBSan as a program of its own."""
import os
import subprocess

ROOT = os.path.dirname(os.path.abspath(__file__))


def test_a_rounds_slice_of_the_candidates_windows():
    exe = os.path.join(ROOT, "cpp", "candidate_windows_check")
    assert os.path.exists(exe), "build it with `make`"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "candidate_windows_check: ok" in r.stdout, r.stdout + r.stderr
