"""The FPFH CPU restatement (tests/fpfh_checker.py, tests/cpp/fpfh_checker.c) and the exported ABI, without a GPU: the restated
acosf against libm on every float, the closed-form histogram values against the plain loop, hand-worked pair features, the
33-D 1-NN against the reference's nanoflann golden, the C99 header, the exported symbols and the defaults."""
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

import fpfh_checker as fc
from golden.gen_fpfh_nn_golden import golden_keys, golden_queries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scl_fpfh.h")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_acosf_equals_libm_on_every_float():
    """all 2^32 inputs against this platform's libm acosf, and the block checksums the GPU test uses"""
    diffs, blocks = fc.acosf_exhaustive()
    assert diffs == 0
    gold = json.load(open(os.path.join(GOLDEN, "acosf_blocks.json")))
    assert gold["differences_vs_libm"] == 0 and blocks == gold["blocks"]


def test_acosf_special_values():
    for x, want in [(1.0, 0.0), (-1.0, np.float32(math.pi)), (0.0, np.float32(math.pi / 2)), (-0.0, np.float32(math.pi / 2))]:
        assert fc.acosf(x) == np.float32(want)
    for x in (1.0000001, -1.5, 2.0, np.inf, -np.inf, np.nan):
        assert np.isnan(fc.acosf(x))


@pytest.mark.parametrize("n", [3, 4, 1000, 96000, 240000])
def test_closed_form_values_equal_the_loop(n):
    from scl_slam_amd.fpfh import hist_values
    inc = fc.hist_incr(n)
    want = fc.values_prefix(n, inc)
    got = hist_values(np.arange(n + 1, dtype=np.uint32), inc)
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    assert bad.size == 0, f"counts {bad[:5].tolist()} differ"
    assert fc.value_loop(n - 1, inc) == want[n - 1]


def test_pair_features_hand_worked():
    z = np.array([0.0, 0.0, 1.0], np.float32)
    t = np.array([0.6, 0.0, 0.8], np.float32)
    # no swap: a1 = n1 . dp / |dp| = 0.6, a2 = 0, acos(0.6) < acos(0): f3 = a1; v = dp x n1 = (0, -0.8, 0) / 0.8, w = n1 x v
    ok, f = fc.pair_features([0, 0, 0], t, [1, 0, 0], z)
    assert ok and f[2] == np.float32(0.6) and f[3] == 1.0
    assert f[1] == 0.0 and np.isclose(f[0], math.atan2(-0.6, 0.8), atol=1e-6)
    # the swap branch: the same pair with the normals exchanged: n2 takes n1's role, dp is negated, f3 = -a2
    ok, f = fc.pair_features([0, 0, 0], z, [1, 0, 0], t)
    assert ok and f[2] == np.float32(-0.6) and f[3] == 1.0
    assert f[1] == 0.0 and np.isclose(f[0], math.atan2(0.6, 0.8), atol=1e-6)
    # swapped onto a normal parallel to dp: |dp x n2| = 0, skipped
    ok, f = fc.pair_features([0, 0, 0], np.array([0.0, 0.6, 0.8], np.float32), [2, 0, 0], np.array([1, 0, 0], np.float32))
    assert not ok and f[3] == 0.0
    # skipped: the same point, and dp parallel to the (swapped) first normal
    ok, f = fc.pair_features([1, 2, 3], z, [1, 2, 3], z)
    assert not ok and f[3] == 0.0
    ok, _ = fc.pair_features([0, 0, 0], z, [0, 0, 5], z)
    assert not ok
    # |a| > 1 (a normal longer than 1): acosf gives NaN, the swap test is false, f3 = a1 > 1 lands in the last bin
    big = np.array([0.0, 0.0, 2.0], np.float32)
    ok, f = fc.pair_features([0, 0, 0], big, [0, 0.1, 1], z)
    assert ok and f[2] > 1.0 and np.isnan(fc.acosf(abs(f[2])))
    assert fc.pair_bins(f)[2] == 10


def test_knn_and_normals_small():
    pts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 2]], np.float32)
    idx, d2 = fc.knn(pts)
    assert idx.shape == (4, 4) and idx[0].tolist() == [0, 1, 2, 3] and d2[0].tolist() == [0, 1, 1, 4]
    assert idx[1].tolist() == [1, 0, 2, 3]                  # d2 2 to point 2 (index 2) before 5 to point 3
    nrm = fc.normals(np.array([[0, 0, 5], [1, 0, 5], [0, 1, 5], [1, 1, 5]], np.float32))
    assert np.array_equal(nrm, np.tile(np.array([[0, 0, -1]], np.float32), (4, 1)))   # flipped towards the origin


def test_nearest_equals_nanoflann_golden():
    gold = json.load(open(os.path.join(GOLDEN, "fpfh_nn_golden.json")))
    n = 0
    for name, case in gold["cases"].items():
        keys = golden_keys(case["N"], case["seed"], case["kind"])
        queries = golden_queries(keys, case["seed"], case["nq"], case["kind"])
        for q, want in zip(queries, case["results"]):
            pos, d2 = fc.nearest(q, keys)
            assert pos == want["idx"] and int(np.float32(d2).view(np.uint32)) == want["d2_bits"], (name, pos, want)
            n += 1
    assert n >= 40


def test_checker_inter_counter_and_snapshot():
    c = fc.FpfhChecker(num_exclude_recent=3, tree_making_period=2)
    keys = golden_keys(12, 5, "hist")
    for k in keys[:3]:
        c.save(k)
    assert c.detect_inter(0) == (-1, np.float32(0.0)) and c.counter == 0
    c.save(keys[3])
    c.detect_inter(3)
    assert c.counter == 1 and c.snap_n == 1
    c.save(keys[4]); c.detect_inter(4)
    assert c.snap_n == 1                                    # stale between rebuilds
    c.save(keys[5]); c.detect_inter(5)
    assert c.snap_n == 3


def test_header_compiles_as_c99():
    out = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                          "-x", "c", HEADER], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_library_exports_every_fpfh_symbol_and_defaults():
    from scl_slam_amd import load_library
    from scl_slam_amd.fpfh import default_config
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(scl_fpfh_[a-z0-9_]+)\s*\(", text)))
    assert len(names) == 21 and "scl_fpfh_make_and_save_many" in names and "scl_fpfh_values" in names
    lib = load_library()
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    c = default_config()
    assert (c.dist_thres, c.num_exclude_recent, c.tree_making_period, c.report_dims, c.inter_mode) == (100.0, 30, 10, 21, 0)
    assert (c.robot_num, c.this_id, c.device) == (1, 0, 0)
