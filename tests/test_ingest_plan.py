"""The copy plan of a group of clouds of the points pipeline (scl_slam_amd/csrc/ingest_plan.hpp: one merged copy or one copy per cloud,
and where each cloud lies in the device buffer) and the table of the database's arrays (scl_slam_amd/csrc/db_arrays.hpp) without a GPU:
tests/cpp/ingest_plan_check.cpp, built by `make` under ASan + UBSan as a program of its own.  It compares the plan with a restatement
of the lambda it was taken out of and with invariants that do not mention that lambda, and the table with the sizes and offsets the
database's growth was written with before."""
import os
import subprocess

ROOT = os.path.dirname(os.path.abspath(__file__))


def test_the_copy_plan_of_a_group_and_the_table_of_the_database_arrays():
    exe = os.path.join(ROOT, "cpp", "ingest_plan_check")
    assert os.path.exists(exe), "build it with `make`"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ingest_plan_check: ok" in r.stdout, r.stdout + r.stderr
