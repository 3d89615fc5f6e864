"""The inputs of tests/offset_cases.py held to what tests/test_gpu_registration_offsets.py relies on, with the CPU checker alone (no GPU):
the checker's grid walk equals its brute force on every family at every offset, the border lattice has exact ties at every offset, a
checker with a wrong pruning margin is caught by these inputs, the exact lattice's answers are the unshifted lattice's, and the
measured bars of the toleranced quantities are the recorded ones."""
import ctypes
import os
import shutil
import subprocess
from ctypes import POINTER, c_float, c_int, c_void_p

import numpy as np
import pytest

import icp_param_cases as pc
import offset_cases as oc
import oracle_binding as ob
import oracle_icp_binding as oi
import registration_plane_cases as rp
import verification_cases as vc
from test_registration_plane_cases import eigen_residuals

CASES = [(f, off) for f in oc.FAMILIES for off in oc.OFFSETS]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name,off", CASES, ids=lambda v: str(v))
def test_checker_grid_equals_brute_force(name, off):
    src, tgt = oc.family(name, off)
    gi, gd = oi.nn(src, tgt, use_grid=True)
    bi, bd = oi.nn(src, tgt, use_grid=False)
    ties = oc.tie_count(src, tgt)
    print(f"{name} at {off:g} m: {len(src)} queries against {len(tgt)} points, {ties} queries with an exact tie for the minimum, "
          f"{int((gi != bi).sum())} mismatches")
    assert np.array_equal(gi, bi) and np.array_equal(_bits(gd), _bits(bd))
    assert (bi >= 0).all()
    if name == "border_lattice":
        assert ties > 0


def test_the_families_are_what_they_are_named_for():
    for off in oc.OFFSETS:
        c = off * oc.OFFSET_DIR
        for name in oc.FAMILIES:
            src, tgt = oc.family(name, off)
            assert src.shape == (oc.N_SRC, 8) and src.dtype == tgt.dtype == np.float32 and np.isfinite(src).all() and np.isfinite(tgt).all()
            assert np.abs(tgt[:, :3].astype(np.float64).min(0) - c).max() < 100.0
        src, tgt = oc.family("scene", off)
        lo, hi = tgt[:, :3].min(0), tgt[:, :3].max(0)
        assert len(tgt) == 6000 and int(((src[:, :3] > hi + 100).all(1)).sum()) == oc.N_SRC // 50
        src, tgt = oc.family("border_lattice", off)
        assert len(tgt) == 97 * 40 * 3
        ext = np.float32((tgt[:, :3].max(0) - tgt[:, :3].min(0)).max())
        assert abs(float(ext / np.float32(96.0)) - oc.PITCH) < 1e-4           # the cell size is the pitch
        lo, hi = tgt[:, :3].min(0), tgt[:, :3].max(0)
        assert ((src[:, :3] < lo - 0.5).any(1) | (src[:, :3] > hi + 0.5).any(1)).any()
        src, tgt = oc.family("dense", off)
        ext = float((tgt[:, :3].max(0) - tgt[:, :3].min(0)).max())
        quanta = ext / 96.0 / float(np.spacing(np.float32(np.abs(tgt[:, :3]).max())))
        print(f"dense at {off:g} m: a cell is {quanta:.1f} quanta of the largest coordinate")
        assert len(tgt) == 5000 and 0.9 < ext < 1.0 and (off < 8000 or quanta < 25)
        src, tgt = oc.family("clusters", off)
        assert len(np.unique(tgt[:, 2])) == 1
        near = np.abs(tgt[:, :2].astype(np.float64) - tgt[0, :2]).max(1) < 0.02
        assert near.sum() == 2500 and len(tgt) == 5000
    assert np.array_equal(oc.family("scene", 0.0)[1], oc._base("scene")[1])


def test_a_checker_with_a_wrong_margin_is_caught(tmp_path):
    """the mutation proof: oracle/icp_oracle.c copied, its `bound *= 0.9999f` turned into `1.02f` (a walk that ends too early), built
    apart -- at least one family x offset must then disagree with brute force, or these inputs would not tell a wrong search from a
    right one"""
    for f in ("icp_oracle.c", "icp_oracle.h"):
        shutil.copy(os.path.join(ob.ORACLE_DIR, f), tmp_path / f)
    text = (tmp_path / "icp_oracle.c").read_text()
    assert text.count("bound *= 0.9999f") == 1
    (tmp_path / "icp_oracle.c").write_text(text.replace("bound *= 0.9999f", "bound *= 1.02f"))
    lib = tmp_path / "libmutant.so"
    subprocess.check_call([os.environ.get("CC", "gcc"), "-O3", "-DNDEBUG", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-std=gnu11",
                           "-shared", "-o", str(lib), str(tmp_path / "icp_oracle.c"), "-lm"])
    L = ctypes.CDLL(str(lib))
    L.icpo_nn.argtypes = [c_void_p, c_int, c_void_p, c_int, c_int, c_int, POINTER(c_int), POINTER(c_float)]
    caught = {}
    for name, off in CASES:
        src, tgt = oc.family(name, off)
        idx = np.empty(len(src), np.int32); d2 = np.empty(len(src), np.float32)
        L.icpo_nn(src.ctypes.data_as(c_void_p), len(src), tgt.ctypes.data_as(c_void_p), len(tgt), 32, 1,
                  idx.ctypes.data_as(POINTER(c_int)), d2.ctypes.data_as(POINTER(c_float)))
        bi, bd = oi.nn(src, tgt, use_grid=False)
        caught[(name, off)] = int(((idx != bi) | (_bits(d2) != _bits(bd))).sum())
    print("queries the mutated checker gets wrong:", {f"{k[0]}@{k[1]:g}": v for k, v in caught.items()})
    assert any(caught.values())


@pytest.mark.parametrize("name", oc.EXACT_EDGE + oc.EXACT_TILE)
def test_the_exact_lattice_carries_over(name):
    """moved by the integer vector, the lattice's every distance is the unshifted lattice's, and the checker's answer too, bit for
    bit (its covariance is formed about the centroids, in double: nothing of the shift is left in it)"""
    c, s = pc.case(name), oc.exact_lattice(name)
    for a, b in ((c.src, s.src), (c.tgts[0], s.tgts[0])):
        assert np.array_equal(b[:, :3].astype(np.float64) - np.asarray(oc.EXACT_SHIFT), a[:, :3].astype(np.float64))
    o, os_ = pc.oracle(c), pc.oracle(s)
    print(name, "unshifted", o[1:], "shifted", os_[1:], "T", os_[0][:3, 3].tolist())
    assert np.array_equal(_bits(o[0]), _bits(os_[0])) and o[1:] == os_[1:]
    if name.endswith("0.4999999"):
        assert (o[2], o[3]) == (False, 0)
    else:
        assert (o[2], o[3]) == (True, 1) and np.array_equal(o[0][:3, :3], np.eye(3, dtype=np.float32))


def test_icp_bars_are_the_recorded_ones():
    """spread, bound and fitness bar of ICP on icp_small per offset and estimator, printed; the spread pinned within a factor 2 of
    offset_cases.RECORDED_SPREAD; the iteration count is the cap on every run"""
    for est in (0, 1):
        for off in oc.OFFSETS:
            T, f, conv, it = oc.icp_checker(off, est)
            spread, bound, fbar = oc.icp_spread(off, est), oc.icp_offset_bound(off, est), oc.fitness_bar(off, est)
            print(f"estimator {est} at {off:g} m: spread {spread:.3e} m, bound {bound:.3e} m, fitness {f:.6e}, fitness bar {fbar:.3e}, "
                  f"converged {conv}, iterations {it}")
            assert (conv, it) == (True, 10)
            rec = oc.RECORDED_SPREAD[(off, est)]
            assert rec / 2 <= spread <= rec * 2
            src, tgt = oc.icp_small(off)
            assert bound >= 2.0 * float(np.spacing(np.float32(max(off * 0.48, 1.0)))) and fbar >= pc.FIT_REL[est]
            # the checker's float T, a rotation rounded to 2^-24 per iteration and carried over the offset's lever, ten times over
            assert spread <= 10 * 8 * 2.0 ** -24 * max(off, 50.0) + 1e-3


def test_verification_and_scoring_inputs():
    """`matching`: every pair an inlier (the test is about the search and the fit).  `ratio_exact`: 100 of 200 pairs are inliers, the
    others 100 m and more off, so the set is a strict subset that only a clean hypothesis finds, and the gate sits on its boundary.  No
    pair is within 1e-6 m of the threshold under the best hypothesis, so the counts cannot sit on a knife edge"""
    for off in oc.OFFSETS:
        for name in oc.VERIFICATIONS:
            o, p, spread, bound, (si, ti, mask, n_inl, best, Tb) = oc.verification_checked(name, off)
            src, tgt, iters, thr, ratio, seed = oc.verification(name, off)
            gap = float(np.abs(oc.ransac_residuals(src, tgt, si, ti, Tb) - thr).min())
            print(f"verification of {name} at {off:g} m: {o[1:]}, best hypothesis {best}, nearest residual to the threshold {gap:.3e} m, "
                  f"spread {spread:.3e} m, bound {bound:.3e} m")
            assert gap > 1e-6
            assert spread < 1e-6 + 4 * 2.0 ** -24 * max(off, 50.0)
            if name == "matching":
                assert o[1:] == (True, 2000, 2000)
            else:
                assert o[1:] == (True, 200, 100) and mask.sum() == 100 and np.array_equal(mask[::2], np.ones(100, np.int32))
        chk = oc.eval_checked(off)
        print(f"scoring at {off:g} m: valid {[c[0] for c in chk]}, inliers {[c[1] for c in chk]}")
        assert [c[0] for c in chk] == [1500, 1500, 1500, 0, 1500] and chk[0][1] > 100


@pytest.mark.parametrize("name", oc.RANSACS)
def test_ransac_inputs_far_out(name):
    """shifted, the RANSAC inputs keep what they promise: the mask is the good pairs, a strict subset; the tie is won by the lower of
    two clean hypotheses, which is not the first, and the `last` case by the last hypothesis; every residual is a factor 10 off the
    threshold"""
    row = next(r for r in vc.RANSAC_TABLE if r[0] == name)
    for off in oc.OFFSETS:
        src, tgt, si, ti, iters, thr, seed, good = oc.ransac_input(name, off)
        mask, n_inl, best, T = oc.ransac_checked(name, off)
        res = oc.ransac_residuals(src, tgt, si, ti, T)
        print(f"{name} at {off:g} m: {n_inl} of {len(si)} inliers, best hypothesis {best} of {iters}, largest inlier residual {res[good].max():.3e} m, "
              f"smallest outlier residual {res[~good].min():.3e} m (threshold {thr})")
        assert np.array_equal(mask.astype(bool), good) and 3 <= n_inl == good.sum() < len(si)
        assert res[good].max() < thr / 10 and res[~good].min() > 10 * thr
        if name.startswith("tie"):
            assert 0 < best <= row[7][0] < row[7][1]
        if name.startswith("last"):
            assert best == iters - 1


def test_clusters_hold_a_cell_heavier_than_a_tile():
    """in the grid both sides build (cells of extent / 96) the knot lies in one or two cells with more points than a tile holds
    (kTilePts = 1 536 in csrc/icp.hip), and the grid has one layer in z"""
    for off in oc.OFFSETS:
        tgt = oc.family("clusters", off)[1][:, :3]
        mn = tgt.min(0)
        h = np.float32((tgt.max(0) - mn).max()) / np.float32(96.0)
        dims = np.floor((tgt.max(0) - mn) / h).astype(int) + 1
        cells = np.floor((tgt - mn) / h).astype(int)
        _, counts = np.unique(cells, axis=0, return_counts=True)
        print(f"clusters at {off:g} m: grid {dims.tolist()}, cell size {float(h):.4f}, heaviest cell {counts.max()} points")
        assert dims[2] == 1 and counts.max() > 1536


def test_normal_residuals_is_eigen_residuals():
    """the neighbour-list form of the normals' bar against the full-matrix one of tests/test_registration_plane_cases.py"""
    tgt = rp.place()
    nrm = rp.cpu_normals_once(tgt, 1.0)
    few, unit, res = eigen_residuals(tgt, 1.0, nrm)
    few2, unit2, res2 = oc.normal_residuals(tgt, 1.0, nrm)
    assert np.array_equal(few, few2) and np.array_equal(unit, unit2)
    assert np.abs(res - res2)[~few].max() < 2.0 ** -30
    lat = oc.family("border_lattice", 0.0)[1]
    d2 = ((lat[:, :3].astype(np.float64) - lat[5 * 40 * 3 + 60, :3]) ** 2).sum(1)
    r2 = (2 * oc.PITCH) ** 2
    assert (np.abs(d2 - r2) < 1e-6).sum() >= 4                       # points at the radius, up to rounding
