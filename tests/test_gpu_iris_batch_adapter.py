"""The batch forms of the LiDAR-Iris C++ adapter (makeAndSaveDescriptorsAndKeys, saveDescriptorsAndKeys, detectIntraLoopClosureIDs,
detectInterLoopClosureIDs, makeSaveAndDetect) against loops over its six virtuals on a second object:
tests/cpp/iris_batch_check.cpp, built by `make`."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.gpu
def test_batch_forms_of_the_iris_adapter_agree_with_the_virtuals():
    exe = os.path.join(ROOT, "cpp", "iris_batch_check")
    assert os.path.exists(exe), "build it with `make`"
    r = subprocess.run([exe, "44"], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout + r.stderr
    assert sum(line.startswith("ok iris:") for line in r.stdout.splitlines()) == 2, r.stdout
