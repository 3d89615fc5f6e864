"""The batch forms of the three C++ adapters (detectIntraLoopClosureIDs, detectInterLoopClosureIDs, makeSaveAndDetect) against
loops over the virtuals: tests/cpp/plugin_batch_check.cpp, built by `make`."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.gpu
def test_batch_forms_of_the_adapters_agree_with_the_virtuals():
    exe = os.path.join(ROOT, "cpp", "plugin_batch_check")
    assert os.path.exists(exe), "build it with `make`"
    r = subprocess.run([exe, "44"], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout + r.stderr
    for name in ("m2dp", "fpfh", "grsd"):
        assert any(line.startswith(f"ok {name}:") for line in r.stdout.splitlines()), r.stdout
