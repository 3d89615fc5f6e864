"""The inputs of tests/icp_guess_cases.py, pinned with the CPU checker alone (no GPU): icpo_transform, then icpo_icp_align, and
T = T_icp * G restated in float64 -- so that tests/test_gpu_icp_guess.py may rest on them.

For the yawed cases (icp_guess_cases.YAWED):
  (a) without the guess the alignment fails: icpo_icp_align(src, tgt) ends with a fitness above 0.3 (historyKeyframeFitnessScore,
      DM.h:192) or with |T - T_true|max >= 5e-3;
  (b) with the guess it succeeds: converged, fitness below 0.3, |T_icp * G - T_true|max < 5e-3 (the bound of
      tests/test_gpu_icp.py's test_icp_align_matches_oracle);
  (c) it is off every knife edge: three copies of the source with half of the coordinates moved by one ulp (before the guess
      moves them) give the same (converged, iterations) and T_icp within 5e-6.
(c) holds for every pair of icp_guess_cases.CHECKED, the ones the GPU test compares with the checker.

Measured (x86-64): without the guess, fitness 2.8 to 116 and |T - T_true| 3.0 to 31; with it, fitness 3.0e-4 and |T - T_true| 6.6e-5
(point to point) to 3.1e-4 (point to plane) in 3 to 7 iterations; jittered copies move T_icp by at most 6.0e-7 and the fitness by
at most 4.6e-6 relative.  The 20 x 60 chain on the checker: 19 974 pairs, all inliers, then one ICP iteration to fitness 3.0e-4 and
|T - T_true| 1.8e-4; from identity guesses 457 inliers, fitness 4.5, |T - T_true| 53."""
import numpy as np
import pytest

import icp_guess_cases as gc
import oracle_icp_binding as oi
from scl_slam_amd import ScanContextEngine

JITTERS = (0, 1, 2)


@pytest.fixture(scope="module")
def results():
    """every checker run this file needs, side by side, once"""
    reqs = []
    for n, p in gc.CHECKED:
        reqs += [(n, p, True, None)] + [(n, p, True, j) for j in JITTERS]
    reqs += [(n, p, False, None) for n, p in gc.YAWED]
    gc.oracle_many(reqs)
    return gc.oracle


def _whole(T_icp, name):
    return gc.compose(T_icp, gc.guesses()[gc.NAMES.index(name)])


def test_the_list_is_what_the_docstring_says():
    G, tg = gc.guesses(), gc.targets()
    assert G.shape == (len(gc.NAMES), 4, 4) and G.dtype == np.float32 and len(tg) == len(gc.NAMES)
    assert np.array_equal(G[0], np.eye(4, dtype=np.float32)) and len({g.tobytes() for g in G}) == len(gc.NAMES)
    assert gc.source().shape == (3000, 8) and all(t.shape == (6000, 8) for t in tg)
    yaws = [np.degrees(np.arctan2(g[1, 0], g[0, 0])) for g in G]
    assert abs(yaws[0]) < 1e-6 and 85 < yaws[1] < 95 and 175 < abs(yaws[2]) <= 180
    assert all(np.linalg.norm(G[k][:3, 3]) > 30 for k in (1, 2, 3, 4))          # tens of metres
    moved = [oi.transform(gc.source(), g) for g in G]
    boxes = {(tuple(m[:, :3].min(0)), tuple(m[:, :3].max(0))) for m in moved}
    assert len(boxes) == len(gc.NAMES)                                          # every candidate's source has a box of its own
    assert set(gc.YAWED) <= set(gc.CHECKED) and all(n in gc.NAMES and p in gc.PARAMS for n, p in gc.CHECKED)


@pytest.mark.parametrize("name,pname", gc.YAWED, ids=lambda v: str(v))
def test_without_the_guess_the_case_fails(results, name, pname):
    T, f, cv, it = results(name, pname, False)
    print(name, pname, "unguessed", cv, it, "fitness", f, "|T - T_true|", np.abs(T - gc.TRUE[name]).max())
    assert f > gc.FITNESS_MAX or np.abs(T - gc.TRUE[name]).max() >= gc.T_TRUE_TOL


@pytest.mark.parametrize("name,pname", gc.YAWED, ids=lambda v: str(v))
def test_with_the_guess_it_succeeds(results, name, pname):
    T, f, cv, it = results(name, pname)
    err = np.abs(_whole(T, name).astype(np.float64) - gc.TRUE[name]).max()
    print(name, pname, "guessed", cv, it, "fitness", f, "|T_icp G - T_true|", err)
    assert cv and f < gc.FITNESS_MAX and err < gc.T_TRUE_TOL
    assert np.abs(T - np.eye(4)).max() > 100 * gc.TOL                          # the guess leaves the alignment something to do


@pytest.mark.parametrize("name,pname", gc.CHECKED, ids=lambda v: str(v))
def test_case_is_not_on_a_knife_edge(results, name, pname):
    T, f, cv, it = results(name, pname)
    for j in JITTERS:
        Tj, fj, cvj, itj = results(name, pname, True, j)
        print(name, pname, j, (cvj, itj), "|dT_icp|", np.abs(Tj - T).max(), "fitness", abs(fj - f) / max(1e-6, abs(f)))
        assert (cvj, itj) == (cv, it)
        assert np.abs(Tj - T).max() <= gc.JITTER_TOL


def test_the_far_guess_finds_no_pair(results):
    """fewer than three pairs at the first search: not converged, no iteration, T_icp = identity, so T = G with the last row 0 0 0 1"""
    T, f, cv, it = results("far", "mcd0.5")
    assert (cv, it) == (False, 0) and np.array_equal(T, np.eye(4, dtype=np.float32))
    k = gc.NAMES.index("far")
    _, d2 = oi.nn(oi.transform(gc.source(), gc.guesses()[k]), gc.targets()[k], use_grid=False)
    assert d2.min() > 25.0                                            # no source within 5 m, against a threshold of 0.5
    want = gc.guesses()[k].copy(); want[3] = (0, 0, 0, 1)
    assert np.array_equal(_whole(T, "far").view(np.uint32), want.view(np.uint32))


def test_the_restated_product_is_the_double_product():
    rs = np.random.RandomState(3)
    A, G = rs.standard_normal((4, 4)).astype(np.float32), (30 * rs.standard_normal((4, 4))).astype(np.float32)
    A[3] = (0, 0, 0, 1)
    G4 = G.copy(); G4[3] = (0, 0, 0, 1)
    want = A.astype(np.float64) @ G4.astype(np.float64)
    assert np.abs(gc.compose(A, G).astype(np.float64) - want).max() <= 2.0 ** -23 * np.abs(want).max()
    assert np.array_equal(gc.compose(A, G), gc.compose(A, G4))                 # G's last row is not read


def test_the_chain_on_the_checker_meets_both_bounds():
    """the 20 x 60 chain's input: voxel filter, guessed verification, its T as the ICP's guess -- fitness < 0.3 and |T - T_true|max <
    5e-3 on the checker alone; the same chain from identity guesses meets neither"""
    cloud, other, turned, received, T_true = gc.end_to_end()
    filt = oi.voxel_grid(received, gc.E2E_LEAF)
    sub = oi.voxel_grid(gc.moved(cloud, gc.pose_matrix(gc.POSE_PRE)), gc.E2E_LEAF)
    assert filt is not None and sub is not None and len(filt) >= 300 and len(sub) >= 1000
    G = ScanContextEngine.loop_guess_from_shift(gc.SECTORS_TURNED, 60, gc.POSE_CUR, gc.POSE_PRE)
    out = {}
    for name, g in (("guess", G), ("identity", np.eye(4, dtype=np.float32))):
        Tf, ok, nc, ni = oi.geometric_verification(oi.transform(filt, g), sub, 300, 0.25, 0.45, 1)
        Tv = gc.compose(Tf, g)
        Ti, f, cv, it = oi.icp_align(oi.transform(filt, Tv), sub)
        err = np.abs(gc.compose(Ti, Tv).astype(np.float64) - T_true).max()
        print(name, "verification", ok, nc, ni, "icp", cv, it, "fitness", f, "|T - T_true|", err)
        out[name] = (ok, cv, f, err)
    ok, cv, f, err = out["guess"]
    assert ok and cv and f < gc.FITNESS_MAX and err < gc.T_TRUE_TOL
    ok, cv, f, err = out["identity"]
    assert not (f < gc.FITNESS_MAX and err < gc.T_TRUE_TOL)
