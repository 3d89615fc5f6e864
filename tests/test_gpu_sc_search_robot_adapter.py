"""The per-robot ranked searches of the Scan Context C++ adapter (searchIntraLoopClosureIDs, searchInterLoopClosureIDs) against the C
calls: tests/cpp/sc_search_robot_check.cpp, built by `make`."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.gpu
@pytest.mark.parametrize("shards", [0, 2])
def test_per_robot_lists_of_the_adapter_agree_with_the_c_calls(shards):
    exe = os.path.join(ROOT, "cpp", "sc_search_robot_check")
    assert os.path.exists(exe), "build it with `make`"
    r = subprocess.run([exe, "90", str(shards)], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout + r.stderr
    assert any(line.startswith("ok sc:") for line in r.stdout.splitlines()), r.stdout
