"""The candidate lists of the three C++ adapters (detectIntraLoopCandidates, detectInterLoopCandidates) against the C calls:
tests/cpp/plugin_topk_check.cpp, built by `make`."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.gpu
def test_candidate_lists_of_the_adapters_agree_with_the_c_calls():
    exe = os.path.join(ROOT, "cpp", "plugin_topk_check")
    assert os.path.exists(exe), "build it with `make`"
    r = subprocess.run([exe, "44"], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout + r.stderr
    for name in ("m2dp", "fpfh", "grsd"):
        assert any(line.startswith(f"ok {name}:") for line in r.stdout.splitlines()), r.stdout
