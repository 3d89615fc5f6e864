"""Geometric verification where its host layer can go wrong (csrc/icp.hip: the single call's chain, a round of candidates and the
workspaces they share): the pair count across the trips of the pair scan, one engine through growing and shared buffers, and a
refused call.  Inputs from the helpers of tests/verification_cases.py; bars as in tests/test_gpu_verification_edges.py: counts
and success exactly, transforms within TOL = 1e-5 of the CPU checker's, one engine against another bit for bit."""
import functools

import numpy as np
import pytest

import oracle_icp_binding as oi
import verification_cases as vc
from scl_slam_amd import ScanContextEngine
from scl_slam_amd.engine import SclError
from scl_slam_amd.synth import rigid_transform, synth_structured_cloud

pytestmark = pytest.mark.gpu
TOL = 1e-5
INVALID_ARG = -1                                                     # include/scl_engine.h
TRIP_SIZES = (4095, 4096, 4097, 8193)
T_SMALL = rigid_transform(0.0, 0.0, 0.002, 0.02, -0.01, 0.0)


@pytest.fixture(scope="module")
def eng():
    e = ScanContextEngine()
    yield e
    e.close()


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _trip_case(n_src):
    """n_src noisy, slightly moved copies of the points of a 3 000-point target (every target point several times over), three of
    them non-finite as vc.with_nonfinite writes them (NaN in x, +inf in y, -inf in z): one in the pair scan's first trip of 4 096
    sources, one at the trip boundary, the last -> (src, tgt, checker)"""
    tgt = synth_structured_cloud(3000, seed=37)
    src = vc._moved_copy(tgt[np.arange(n_src) % len(tgt)], T_SMALL, 1, 0.003, n_src)
    for m, r in enumerate((7, min(4096, n_src - 2), n_src - 1)):
        src[r, m % 3] = vc.NONFINITE[m]
    return src, tgt, oi.geometric_verification(src, tgt, 9, 0.25, 0.45, 3)


@pytest.mark.parametrize("n_src", TRIP_SIZES)
def test_verification_across_the_pair_scan_trips(eng, n_src):
    """The pairs of a candidate: the single call's device-wide prefix sum and, in a round of one candidate, the 4 096 sources per
    trip of verify_pairs_batch_kernel with the count carried along.  9 hypotheses, threshold 0.25, ratio 0.45, seed 3.  The
    checker's (success, n_corr, n_inliers): 4095 -> (True, 4092, 4092), 4096 -> (True, 4093, 4093), 4097 -> (True, 4094, 4094),
    8193 -> (True, 8190, 8190): every pair an inlier, far above 0.45 * n_corr."""
    src, tgt, o = _trip_case(n_src)
    g = eng.geometric_verification(src, tgt, 9, 0.25, 0.45, 3)
    b = eng.geometric_verification_batch(src, [tgt], 9, 0.25, 0.45, 3)
    print(n_src, g[1:], o[1:], float(np.abs(g[0] - o[0]).max()), float(np.abs(b[0][0] - o[0]).max()))
    assert o[1:] == (True, n_src - 3, n_src - 3)
    assert g[1:] == o[1:] and (bool(b[1][0]), int(b[2][0]), int(b[3][0])) == o[1:]
    assert np.abs(g[0] - o[0]).max() < TOL and np.abs(b[0][0] - o[0]).max() < TOL
    assert np.array_equal(_bits(b[0][0]), _bits(g[0]))


def _same_answer(got, want):
    """two answers of one call, floats as uint32"""
    assert len(got) == len(want)
    for a, b in zip(got, want):
        if isinstance(a, np.ndarray) and a.dtype == np.float32 or isinstance(a, float):
            assert np.array_equal(_bits(a), _bits(b))
        else:
            assert np.array_equal(a, b)


@functools.lru_cache(maxsize=None)
def _small_case():
    """300 sources on 500 targets -> (src, tgt, checker)"""
    tgt = synth_structured_cloud(500, seed=41)
    src = vc._moved_copy(tgt, T_SMALL, 1, 0.003, 5)[:300]
    return src, tgt, oi.geometric_verification(src, tgt, 300, 0.25, 0.45, 3)


def _small_verification(e):
    src, tgt, o = _small_case()
    g = e.geometric_verification(src, tgt, 300, 0.25, 0.45, 3)
    assert g[1:] == o[1:] and g[3] >= 3 and np.abs(g[0] - o[0]).max() < TOL
    return g


def _growth_calls():
    """the calls of test_one_engine_through_growing_and_shared_buffers, each a function of an engine"""
    big = synth_structured_cloud(5000, seed=43)
    big_src = vc._moved_copy(big, T_SMALL, 1, 0.003, 6)
    far = big.copy(); far[:, :3] += np.float32(40.0)
    big_tgts = [big, synth_structured_cloud(5000, seed=44), far]
    trip_src, trip_tgt, _ = _trip_case(4097)
    m_src, m_tgt = vc.verification_cases()["matching"][:2]           # 2 000 sources; every other target point: 2 000
    case, iters, thr, seed = vc.ransac_get("n5000_i4096")

    def plane(e):
        p = e.icp_default_params(); p.max_iterations = 8; p.estimator = 1; p.normal_radius = 1.5
        return e.icp_align(m_src, m_tgt[::2], p)

    return [_small_verification,
            lambda e: e.geometric_verification_batch(big_src, big_tgts, 300, 0.25, 0.45, 3),
            lambda e: e.geometric_verification(trip_src, trip_tgt, 9, 0.25, 0.45, 3),
            plane,
            lambda e: e.ransac_correspondences(case["src"], case["tgt"], case["si"], case["ti"], iters, thr, seed),
            _small_verification]


def test_one_engine_through_growing_and_shared_buffers():
    """The single calls share one workspace whose slots only grow, an alignment's workspace is its batch's ctl as well, and the
    rounds keep their tables in slots of their own: a small verification, a batch of 3 x 5 000 points, a verification of 4 097
    sources (every buffer grows), a point-to-plane alignment (normals in B_OUT's slot), RANSAC with 4 096 hypotheses (B_HYP,
    B_MASK), the first verification again -- every answer equal, floats as uint32, to a fresh engine's answer to that call alone"""
    calls = _growth_calls()
    want = []
    for call in calls[:-1]:
        e = ScanContextEngine()
        want.append(call(e))
        e.close()
    want.append(want[0])
    e = ScanContextEngine()
    for k, (call, w) in enumerate(zip(calls, want)):
        print(k, [x if not isinstance(x, np.ndarray) else x.shape for x in w])
        _same_answer(call(e), w)
    e.close()


def test_verification_refused_and_the_engine_afterwards():
    """no hypotheses for three sources: INVALID_ARG and its message, nothing launched; the engine then answers as a fresh one"""
    e = ScanContextEngine()
    want = _small_verification(e)
    e.close()
    e = ScanContextEngine()
    src, tgt = vc.verification_cases()["sizes_3_4000"][:2]
    for iters in (0, 2 ** 20 + 1):
        with pytest.raises(SclError) as ei:
            e.geometric_verification(src, tgt, iters, 0.25, 0.45, 3)
        assert ei.value.status == INVALID_ARG and "ransac iterations out of range" in str(ei.value)
    _same_answer(_small_verification(e), want)
    e.close()
