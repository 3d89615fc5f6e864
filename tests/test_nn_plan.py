"""The plan of the vector plugins' batched search (scl_slam_amd/csrc/nn_plan.hpp: the grouping by list, the list offsets, the launch
groups, the partial lists' rows and the 2^31 guard) without a GPU: tests/cpp/nn_plan_check.cpp, built by `make` under ASan + UBSan
as a program of its own."""
import os
import subprocess

ROOT = os.path.dirname(os.path.abspath(__file__))


def test_the_plan_of_a_batched_search():
    exe = os.path.join(ROOT, "cpp", "nn_plan_check")
    assert os.path.exists(exe), "build it with `make`"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "nn_plan_check: ok" in r.stdout, r.stdout + r.stderr
