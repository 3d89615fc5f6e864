"""The launch schedule of a chunk of the screened stream form (scl_slam_amd/csrc/screen_plan.hpp: which groups go as pairs, who aligns
whom, when a tail reaches into the next chunk) without a GPU: tests/cpp/screen_plan_check.cpp, built by `make` under ASan + UBSan as a
program of its own.  It compares the plan with a restatement of the loop it was taken out of and with invariants that do not mention
that loop."""
import os
import subprocess

ROOT = os.path.dirname(os.path.abspath(__file__))


def test_the_schedule_of_a_chunk_of_the_screened_stream():
    exe = os.path.join(ROOT, "cpp", "screen_plan_check")
    assert os.path.exists(exe), "build it with `make`"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "screen_plan_check: ok" in r.stdout, r.stdout + r.stderr
