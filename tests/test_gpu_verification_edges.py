"""The one-shot kernels of geometric verification (csrc/icp.hip: rigid fit over explicit pairs, RANSAC over explicit pairs, the whole
verification, the cloud transform) against the CPU checker at the edges of their dispatch rules and buffer arithmetic: the inputs of
tests/verification_cases.py, which tests/test_verification_cases.py pins on the CPU.  Bars: transforms within TOL = 1e-5 (the offset
cases: test_verification_cases.offset_bound, on moved points), RANSAC and the transform bit for bit."""
import functools

import numpy as np
import pytest

import oracle_icp_binding as oi
import verification_cases as vc
from scl_slam_amd import ScanContextEngine
from scl_slam_amd.engine import SclError
from test_verification_cases import offset_bound
from voxel_cases import same_bits

pytestmark = pytest.mark.gpu
TOL = 1e-5
INVALID_ARG, OUT_OF_RANGE = -1, -4                                   # include/scl_engine.h


@pytest.fixture(scope="module")
def eng():
    e = ScanContextEngine()
    yield e
    e.close()


def _moved(T, p):
    return p @ np.asarray(T, np.float64)[:3, :3].T + np.asarray(T, np.float64)[:3, 3]


@functools.lru_cache(maxsize=None)
def _checker_fit(name):
    src, tgt, si, ti, _ = vc.rigid_cases()[name]
    return oi.rigid_svd(src, tgt, si, ti)


# ---- rigid fit ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in vc.rigid_names() if not n.startswith(("offset", "collinear"))])
def test_rigid_svd_matches_checker(eng, name):
    """every pair count around the reduction's lane blocks, wave passes and grid-stride loops; slabs on both sides of the switch
    between the polar factor and Horn's quaternion (the checker always takes Horn's), a planar cloud, a mirrored target"""
    src, tgt, si, ti, _ = vc.rigid_cases()[name]
    Tg, To = eng.rigid_svd(src, tgt, si, ti), _checker_fit(name)
    print(name, float(np.abs(Tg - To).max()))
    assert np.abs(Tg - To).max() < TOL
    assert np.array_equal(Tg[3], [0, 0, 0, 1])
    if name == "identical":                                          # S is exactly zero: R = I, t = q - p
        assert np.array_equal(Tg[:3, :3], np.eye(3, dtype=np.float32)) and np.array_equal(Tg[:3, 3], tgt[5, :3] - src[2, :3])


@pytest.mark.parametrize("name", vc.rigid_names("offset"))
def test_rigid_svd_far_from_the_origin(eng, name):
    """the covariance formed in one pass (device) against the checker's two passes, the cloud 0 .. 8 km from the origin"""
    src, tgt, si, ti, _ = vc.rigid_cases()[name]
    Tg, To = eng.rigid_svd(src, tgt, si, ti), _checker_fit(name)
    p = src[si, :3].astype(np.float64)
    err, bound = float(np.abs(_moved(Tg, p) - _moved(To, p)).max()), offset_bound(name)
    print(name, err, bound)
    assert err <= bound
    assert np.abs(Tg[:3, :3] - To[:3, :3]).max() < TOL


@pytest.mark.parametrize("name", vc.rigid_names("collinear"))
def test_rigid_svd_collinear_invariants(eng, name):
    """the rotation about the line is free on both sides: a finite proper rotation whose fit is no worse than the checker's"""
    src, tgt, si, ti, _ = vc.rigid_cases()[name]
    Tg, To = eng.rigid_svd(src, tgt, si, ti), _checker_fit(name)
    R = Tg[:3, :3].astype(np.float64)
    assert np.isfinite(Tg).all() and np.array_equal(Tg[3], [0, 0, 0, 1])
    assert np.abs(R.T @ R - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(R) - 1) < 1e-6
    p, q = src[si, :3].astype(np.float64), tgt[ti, :3].astype(np.float64)
    rms = lambda T: float(np.sqrt(((_moved(T, p) - q) ** 2).sum(1).mean()))
    print(name, rms(Tg), rms(To))
    assert rms(Tg) <= rms(To) + TOL


# ---- RANSAC ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _checker_ransac(name):
    case, iters, thr, seed = vc.ransac_get(name)
    return oi.ransac(case["src"], case["tgt"], case["si"], case["ti"], iters, thr, seed)


def _assert_ransac(got, want):
    gm, gn, gb, gT = got
    om, on, ob_, oT = want
    assert (gn, gb) == (on, ob_)
    assert np.array_equal(gm, om)
    assert np.abs(gT[:3] - oT).max() < 1e-6


@pytest.mark.parametrize("name", vc.ransac_names())
def test_ransac_matches_checker_bit_for_bit(eng, name):
    case, iters, thr, seed = vc.ransac_get(name)
    got = eng.ransac_correspondences(case["src"], case["tgt"], case["si"], case["ti"], iters, thr, seed)
    _assert_ransac(got, _checker_ransac(name))
    n = len(case["si"])
    if thr == 0.0:
        assert (got[1], got[2]) == (0, 0) and not got[0].any()
    elif thr == 1e3:
        assert (got[1], got[2]) == (n, 0) and got[0].all()
    else:
        assert got[1] == case["n_good"] and np.array_equal(got[0].astype(bool), case["good"])
    if n == 3:
        assert got[2] == 0                                           # every hypothesis is the same triple


def test_ransac_fewer_iterations_after_more_on_one_engine(eng):
    """counts, best and the model share one buffer laid out by the iteration count: 4 096 iterations, then 9, 1 and 257 on inputs of
    other sizes, each equal to a fresh engine's (and to the checker's)"""
    names = ("n5000_i4096", "n1025_i9", "n257_i1", "n255_i257")
    fresh = []
    for name in names:
        case, iters, thr, seed = vc.ransac_get(name)
        e = ScanContextEngine()
        fresh.append(e.ransac_correspondences(case["src"], case["tgt"], case["si"], case["ti"], iters, thr, seed))
        e.close()
    e = ScanContextEngine()
    for name, want in zip(names, fresh):
        case, iters, thr, seed = vc.ransac_get(name)
        got = e.ransac_correspondences(case["src"], case["tgt"], case["si"], case["ti"], iters, thr, seed)
        assert (got[1], got[2]) == (want[1], want[2]) and np.array_equal(got[0], want[0])
        assert np.array_equal(got[3].view(np.uint32), want[3].view(np.uint32))
        _assert_ransac(got, _checker_ransac(name))
    e.close()


def test_status_codes_and_the_engine_afterwards(eng):
    case, iters, thr, seed = vc.ransac_get("n257_i9")
    src, tgt, si, ti = case["src"], case["tgt"], case["si"], case["ti"]

    def status(call):
        with pytest.raises(SclError) as ei:
            call()
        return ei.value.status

    assert status(lambda: eng.ransac_correspondences(src, tgt, si[:0], ti[:0], 9, thr, seed)) == INVALID_ARG
    assert status(lambda: eng.ransac_correspondences(src, tgt, si[:2], ti[:2], 9, thr, seed)) == INVALID_ARG
    assert status(lambda: eng.ransac_correspondences(src, tgt, si, ti, 0, thr, seed)) == INVALID_ARG
    assert status(lambda: eng.ransac_correspondences(src, tgt, si, ti, 2 ** 20 + 1, thr, seed)) == INVALID_ARG
    assert status(lambda: eng.rigid_svd(src, tgt, si[:0], ti[:0])) == INVALID_ARG
    assert status(lambda: eng.rigid_svd(src, tgt, si[:2], ti[:2])) == INVALID_ARG
    for bad_s, bad_t in ((-1, None), (len(src), None), (None, -1), (None, len(tgt))):
        s2, t2 = si.copy(), ti.copy()
        if bad_s is not None:
            s2[100] = bad_s
        if bad_t is not None:
            t2[256] = bad_t
        assert status(lambda: eng.ransac_correspondences(src, tgt, s2, t2, 9, thr, seed)) == OUT_OF_RANGE
        assert status(lambda: eng.rigid_svd(src, tgt, s2, t2)) == OUT_OF_RANGE
    _assert_ransac(eng.ransac_correspondences(src, tgt, si, ti, iters, thr, seed), _checker_ransac("n257_i9"))
    rsrc, rtgt, rsi, rti, _ = vc.rigid_cases()["pairs_257"]
    assert np.abs(eng.rigid_svd(rsrc, rtgt, rsi, rti) - _checker_fit("pairs_257")).max() < TOL


# ---- geometric verification -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", vc.verification_names())
def test_geometric_verification_matches_checker(eng, name):
    """success, the pair count, the inlier count and T; a source with a non-finite coordinate has no nearest neighbour and is no
    pair -- n_corr = n_src - k, hypotheses draw from the pairs that are left"""
    src, tgt, iters, thr, ratio, seed = vc.verification_cases()[name]
    g = eng.geometric_verification(src, tgt, iters, thr, ratio, seed)
    o = oi.geometric_verification(vc.checker_source(name), tgt, iters, thr, ratio, seed)   # (see vc.CHECKER_ON_FINITE_ROWS)
    print(name, g[1:], o[1:])
    assert g[1:] == o[1:]
    assert np.abs(g[0] - o[0]).max() < TOL
    if name in vc.NONFINITE_COUNTS:
        assert g[2] == len(src) - vc.NONFINITE_COUNTS[name]
    if g[3] < 3:
        assert np.array_equal(g[0], np.eye(4, dtype=np.float32))


# ---- transform ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", vc.WIDTHS)
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 5000])
def test_transform_cloud_bit_exact(eng, n, width):
    """x, y, z moved in fp32 without FMA, every other float of a record unchanged; the last row of T is not read; non-finite
    coordinates go through the same arithmetic"""
    rs = np.random.RandomState(5000 + n + width)
    c = rs.uniform(-50, 50, (n, width)).astype(np.float32)
    T = vc.rigid_transform(0.3, 0.2, -1.0, 4, 5, 6).astype(np.float32)
    T[3] = [7.0, -3.0, 0.5, 2.0]
    for k, v in enumerate((np.nan, np.inf, -np.inf)):
        if n > 8:
            c[2 * k + 1, k] = v; c[n - 1 - k, (k + 1) % 3] = v
    g, o = eng.transform_cloud(c, T), oi.transform(c, T)
    assert same_bits(g, o)                                           # (a NaN is a NaN: its sign and payload are the hardware's)
    assert np.array_equal(g[:, 3:].view(np.uint32), c[:, 3:].view(np.uint32))
    T2 = T.copy(); T2[3] = [0, 0, 0, 1]
    assert same_bits(eng.transform_cloud(c, T2), o)
