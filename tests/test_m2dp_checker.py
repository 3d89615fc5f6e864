"""The M2DP checker's known answers, its rotation invariance, and the C ABI's surface (no GPU needed)."""
import math
import os
import re
import subprocess

import numpy as np

import m2dp_checker as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scl_m2dp.h")


def _frame_identity():
    return np.zeros(3, np.float32), np.eye(3, dtype=np.float32)


def _counts_of_pca_rows(rows_xyz, max_rho):
    """counts of points given directly as cloudPca rows (x, y, -z) under the identity frame (cloud z = -row z)"""
    cloud = np.array([[x, y, -z] for x, y, z in rows_xyz], np.float32)
    return mc.signature_matrix(cloud, _frame_identity())


def test_plane_vectors_equal_the_formulas():
    px, py = mc.planes()
    for i in range(4):
        for j in range(16):
            azm = -math.pi / 2 + i * math.pi / 3
            elv = j * (math.pi / 2) / 15
            n = np.array([math.cos(elv) * math.cos(azm), math.cos(elv) * math.sin(azm), math.sin(elv)])
            p = np.array([1.0, 0.0, 0.0]) - n[0] * n
            r = i * 16 + j
            assert np.allclose(px[r], p, atol=1e-15) and np.allclose(py[r], np.cross(n, p), atol=1e-15)
            assert abs(px[r] @ n) < 1e-15 and abs(py[r] @ n) < 1e-15 and abs(px[r] @ py[r]) < 1e-15


def test_bin_edges_follow_the_reference_expressions():
    tl = mc.theta_list()
    assert tl[0] == -math.pi and tl[8] == 0.0 and tl[16] == math.pi and len(tl) == 17
    rl = mc.rho_list(4.0)
    assert rl[0] == 0.0 and rl[4] == 1.0 and rl[8] == 4.0 + 0.001 and len(rl) == 9


def test_column_order_is_rho_bin_times_16_plus_theta_bin():
    """one point per (theta, rho) bin in plane 0: the column is rho_bin * 16 + theta_bin (hist's column-major index)"""
    px, py = mc.planes()
    R = 64.0
    rows, want = [], []
    for rb in range(6):                                         # rho <= 0.47 R: sqrt(x*x + x*x + z*z) stays below maxRho = R
        for tb in range(16):
            rho = R * ((rb + 0.5) / 8) ** 2                     # rhoList[j] = R * (j / 8)^2
            th = -math.pi + (tb + 0.5) * 2 * math.pi / 16
            v = rho * math.cos(th) * px[0] + rho * math.sin(th) * py[0]
            rows.append(tuple(v)); want.append(rb * 16 + tb)
    rows.append((0.0, 0.0, -R))                                 # the point that sets maxRho = 64 (cloud z = 64, x = 0)
    counts, max_rho = _counts_of_pca_rows(rows, None)
    assert max_rho == R
    expected = np.zeros(128, np.int64)
    np.add.at(expected, want, 1)
    extra = counts[0].astype(np.int64) - expected
    assert extra.min() == 0 and extra.sum() == 1               # every bin point where it belongs; the maxRho point in one bin


def test_theta_plus_pi_and_beyond_last_rho_edge_are_dropped():
    px, py = mc.planes()
    pcx = np.array([-1.0, 1.0, -1.0]); pcy = np.array([0.0, 0.0, -0.0])
    tb, _ = mc.theta_bins(pcx, pcy)
    assert tb[0] == 16 and tb[1] == 8 and tb[2] == 0            # atan2(+0, -1) = +pi -> dropped; (-0, -1) = -pi -> bin 0
    rl = mc.rho_list(9.0)
    rb = np.searchsorted(np.asarray(rl), np.array([rl[8], 8.99, 0.0]), side="right") - 1
    assert rb[0] == 8 and rb[1] == 7 and rb[2] == 0             # rho >= rhoList[8] -> bin 8 -> dropped


def test_max_rho_quirk_uses_x_twice_and_no_y():
    cloud = np.array([[1.0, 5.0, 0.0], [0.0, 0.0, 1.0], [-1.0, -5.0, -1.0]], np.float32)
    _, max_rho = mc.cloud_pca(cloud, _frame_identity())
    assert max_rho == np.float32(math.sqrt(1 + 1 + 1))          # point 2: x twice + z, not sqrt(1 + 25 + 1)
    assert max_rho != np.float32(math.sqrt(1 + 25 + 1))


def test_rotation_and_translation_invariance():
    from scl_slam_amd.synth import synth_scan
    cloud = synth_scan(6000, seed=3)[:, :3].astype(np.float64)
    rs = np.random.RandomState(5)
    q = rs.standard_normal(4); q /= np.linalg.norm(q)
    w, x, y, z = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    moved = (cloud @ R.T + np.array([12.5, -3.0, 7.25])).astype(np.float32)
    m0, a0 = mc.frame(cloud.astype(np.float32)); m1, a1 = mc.frame(moved)
    back = (a1.astype(np.float64) @ R)                          # axes of the moved cloud, rotated back
    assert np.max(np.abs(back - a0.astype(np.float64))) < 1e-6
    c0, _ = mc.signature_matrix(cloud.astype(np.float32)); c1, _ = mc.signature_matrix(moved)
    flips = int(np.abs(c0.astype(np.int64) - c1.astype(np.int64)).sum())
    # the float frame and projection can move a few (point, plane) votes across bin edges; measured on this cloud: 0 of 384 000
    assert flips < 0.002 * 64 * cloud.shape[0], flips
    s0 = mc.signature_from_counts(c0, cloud.shape[0]); s1 = mc.signature_from_counts(c1, cloud.shape[0])
    assert np.max(np.abs(s0 - s1)) < 1e-3


def test_signature_is_the_non_negative_perron_pair():
    from scl_slam_amd.synth import synth_scan
    s = mc.signature(synth_scan(3000, seed=9))
    assert s.shape == (192,) and s.dtype == np.float32
    assert np.all(s >= -1e-7) and abs(np.linalg.norm(s[:64]) - 1) < 1e-6 and abs(np.linalg.norm(s[64:]) - 1) < 1e-6


def test_nanoflann_distance_order():
    rs = np.random.RandomState(1)
    a = rs.standard_normal(192).astype(np.float32); b = rs.standard_normal(192).astype(np.float32)
    d = mc.sqdist_nanoflann(a, b)
    assert d.dtype == np.float32 and abs(float(d) - float(np.sum((a.astype(np.float64) - b) ** 2))) < 1e-3


def test_edge_constants_in_the_kernel_equal_the_checker():
    """the double-double (cos, sin) of every theta edge's midpoint, embedded in m2dp.hip, recomputed at 70 digits"""
    src = open(os.path.join(ROOT, "scl_slam_amd", "csrc", "m2dp.hip")).read()
    block = src.split("c_edge_cs[17][4] = {")[1].split("};")[0]
    rows = re.findall(r"\{([^{}]+)\}", block)
    assert len(rows) == 17
    got = [tuple(float.fromhex(x.strip()) for x in r.split(",")) for r in rows]
    assert got == mc.theta_edge_constants()


def test_header_compiles_as_c99():
    out = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                          "-x", "c", HEADER], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def _declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(scl_m2dp_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_m2dp_symbol():
    from scl_slam_amd import load_library
    names = _declared()
    assert len(names) == 17 and "scl_m2dp_make_and_save_many" in names and "scl_m2dp_signature_matrix" in names
    lib = load_library()
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing

