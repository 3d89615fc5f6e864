"""The exhaustive ranked search of the LiDAR-Iris C++ adapter (searchIntraLoopClosureIDs, searchInterLoopClosureIDs) against the C
calls: tests/cpp/iris_search_check.cpp, built by `make`."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.gpu
def test_ranked_lists_of_the_adapter_agree_with_the_c_calls():
    exe = os.path.join(ROOT, "cpp", "iris_search_check")
    assert os.path.exists(exe), "build it with `make`"
    r = subprocess.run([exe, "44"], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout + r.stderr
    assert any(line.startswith("ok iris:") for line in r.stdout.splitlines()), r.stdout
