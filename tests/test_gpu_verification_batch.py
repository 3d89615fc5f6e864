"""scl_geometric_verification_batch and scl_geometric_verification_batch_from_store (csrc/icp.hip, the batched verification tail)
against the single calls, bit for bit, and against the CPU checker on the list of tests/verification_batch_cases.py, which
tests/test_verification_batch_cases.py pins on the CPU.  Bars: entry c of a batch is the single call's answer for candidate c (T
compared as uint32, success, pair count, inlier count); counts and success equal the checker's, T within TOL = 1e-5 of it (the
project's bar, tests/test_gpu_verification_edges.py)."""
import functools
from ctypes import POINTER, byref, c_float, c_int, c_void_p

import numpy as np
import pytest

import verification_batch_cases as bc
import verification_cases as vc
from scl_slam_amd import ScanContextEngine
from scl_slam_amd.engine import SclError
from scl_slam_amd.synth import rigid_transform, synth_structured_cloud
from test_verification_batch_cases import checker

pytestmark = pytest.mark.gpu
TOL = 1e-5
INVALID_ARG = -1                                                      # include/scl_engine.h
IDENT = np.eye(4, dtype=np.float32)
THR, RATIO, SEED = bc.THRESHOLD, bc.RATIO, bc.SEED


@pytest.fixture(scope="module")
def eng():
    e = ScanContextEngine()
    yield e
    e.close()


def _singles(e, src, tgts, *args):
    return [e.geometric_verification(src, t, *args) for t in tgts]


def _assert_entries(batch, singles):
    T, ok, nc, ni = batch
    assert T.shape == (len(singles), 4, 4) and len(ok) == len(nc) == len(ni) == len(singles)
    for c, (T1, ok1, nc1, ni1) in enumerate(singles):
        assert (bool(ok[c]), int(nc[c]), int(ni[c])) == (ok1, nc1, ni1), (c, ok[c], nc[c], ni[c], ok1, nc1, ni1)
        assert np.array_equal(T[c].view(np.uint32), T1.view(np.uint32)), c


@functools.lru_cache(maxsize=None)
def _list_singles(iterations, thr=THR, ratio=RATIO):
    """the single call per candidate of the list on an engine of its own (shared by the tests that batch the same list)"""
    e = ScanContextEngine()
    try:
        return _singles(e, bc.source()[0], bc.clouds(), iterations, thr, ratio, SEED)
    finally:
        e.close()


# ---- the whole list in one call ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iterations", bc.ITERATIONS)
def test_whole_list_in_one_call(eng, iterations):
    """hypothesis counts on the edges of kHypPerBlock = 8 and of the pick kernel's 256-thread trip"""
    got = eng.geometric_verification_batch(bc.source()[0], bc.clouds(), iterations, THR, RATIO, SEED)
    _assert_entries(got, _list_singles(iterations))
    for c, (To, oko, nco, nio) in enumerate(checker(iterations)):
        print(iterations, bc.names()[c], bool(got[1][c]), int(got[2][c]), int(got[3][c]), float(np.abs(got[0][c] - To).max()))
        assert (bool(got[1][c]), int(got[2][c]), int(got[3][c])) == (oko, nco, nio)
        assert np.abs(got[0][c] - To).max() < TOL


@pytest.mark.parametrize("ratio", [0.0, 0.45, 1.0])
def test_ratios(eng, ratio):
    got = eng.geometric_verification_batch(bc.source()[0], bc.clouds(), 300, THR, ratio, SEED)
    _assert_entries(got, _list_singles(300, THR, ratio))
    want = [r[1] for r in checker(300, THR, ratio)]
    assert [bool(x) for x in got[1]] == want
    if ratio == 0.0:
        assert all(want[c] for c, n in enumerate(bc.names()) if n != "empty")      # 0 inliers of n pairs: not (0 < 0)


@pytest.mark.parametrize("thr", [0.0, 1e3])
def test_thresholds(eng, thr):
    got = eng.geometric_verification_batch(bc.source()[0], bc.clouds(), 9, thr, RATIO, SEED)
    _assert_entries(got, _list_singles(9, thr))
    for c, n in enumerate(bc.names()):
        if thr == 0.0:
            assert got[3][c] == 0 and np.array_equal(got[0][c], IDENT)
        else:
            assert got[3][c] == got[2][c] == (0 if n == "empty" else 2000 - bc.N_NONFINITE)


# ---- few pairs, few sources ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1997, 1998])
def test_few_pairs(eng, k):
    """all but 3 (2) sources non-finite: n_corr = 3 (2) on the device for every non-empty candidate"""
    src = vc.with_nonfinite(vc.verification_cases()["matching"][0], k)[0]
    got = eng.geometric_verification_batch(src, bc.clouds(), 300, THR, RATIO, SEED)
    _assert_entries(got, _singles(eng, src, bc.clouds(), 300, THR, RATIO, SEED))
    for c, n in enumerate(bc.names()):
        assert got[2][c] == (0 if n == "empty" else 2000 - k)
        if k == 1998:
            assert not got[1][c] and got[3][c] == 0 and np.array_equal(got[0][c], IDENT)


@pytest.mark.parametrize("n_src", [0, 1, 2, 3])
def test_tiny_sources(eng, n_src):
    src = bc.finite_source()[:n_src]
    got = eng.geometric_verification_batch(src, bc.clouds(), 300, THR, RATIO, SEED)
    _assert_entries(got, _singles(eng, src, bc.clouds(), 300, THR, RATIO, SEED))
    assert all(got[2][c] == (0 if n == "empty" else n_src) for c, n in enumerate(bc.names()))
    if n_src < 3:                                                     # nothing is sampled: the iteration count is not looked at
        assert not got[1].any() and np.array_equal(got[0], np.broadcast_to(IDENT, got[0].shape))
        _assert_entries(eng.geometric_verification_batch(src, bc.clouds(), 0, THR, RATIO, SEED), _singles(eng, src, bc.clouds(), 0, THR, RATIO, SEED))


# ---- the reduction's partition ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pairs", [255, 256, 257])
def test_pair_counts_around_one_workgroup(eng, pairs):
    """rb = ceil(n_corr / 256) workgroups share a candidate's pairs: 1, 1 and 2, while the launch is sized for the sources"""
    src = bc.finite_source()[:pairs + 3].copy()
    src[5, 0], src[100, 1], src[pairs + 2, 2] = np.nan, np.inf, -np.inf   # n_src = pairs + 3 > n_corr = pairs
    got = eng.geometric_verification_batch(src, bc.clouds(), 9, THR, RATIO, SEED)
    _assert_entries(got, _singles(eng, src, bc.clouds(), 9, THR, RATIO, SEED))
    assert got[2][0] == pairs and got[3][0] >= 3


def test_more_pairs_than_the_reduction_has_workgroups(eng):
    """70 000 pairs > kRedBlocks x 256 = 65 536 (every workgroup strides) beside a candidate with the same pairs and few inliers"""
    tgt = synth_structured_cloud(70000, seed=41)
    src = vc._moved_copy(tgt, rigid_transform(0.0, 0.0, 0.002, 0.02, -0.01, 0.0), 1, 0.003, 2)
    tgts = [tgt, np.ascontiguousarray(bc._yawed(tgt, 3.0)[:30000])]
    got = eng.geometric_verification_batch(src, tgts, 16, THR, RATIO, SEED)
    _assert_entries(got, _singles(eng, src, tgts, 16, THR, RATIO, SEED))
    print(got[1], got[2], got[3])
    assert got[2][0] == got[2][1] == 70000 and got[3][0] >= 3 and got[3][1] < got[3][0]


# ---- candidate counts ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 32, 33])
def test_candidate_counts(eng, n):
    """rounds of 32: 33 candidates are two rounds, the 33rd another cloud than the 1st"""
    order = [c % len(bc.names()) for c in range(n)]
    assert n < 33 or order[32] != order[0]
    got = eng.geometric_verification_batch(bc.source()[0], [bc.clouds()[c] for c in order], 9, THR, RATIO, SEED)
    _assert_entries(got, [_list_singles(9)[c] for c in order])
    assert got[0].shape == (n, 4, 4)


@pytest.mark.parametrize("width", [3, 4, 8])
def test_record_strides(eng, width):
    src = np.ascontiguousarray(bc.source()[0][:, :width])
    tgts = [np.ascontiguousarray(c[:, :width]) for c in bc.clouds()]
    got = eng.geometric_verification_batch(src, tgts, 9, THR, RATIO, SEED)
    _assert_entries(got, _singles(eng, src, tgts, 9, THR, RATIO, SEED))
    _assert_entries(got, _list_singles(9))                            # the fields behind z are not read


# ---- from the keyframe store --------------------------------------------------------------------------------------------------------
N_KF, SN, LEAF, SRC_LEAF = 12, 2, 0.3, 0.2


def _fill_store(e):
    base = synth_structured_cloud(36000, seed=13)
    perm = np.random.RandomState(6).permutation(12000)               # keyframes 0 .. 7 see the received scan's place, 8 .. 11 another
    for k in range(N_KF):
        e.keyframe_put(0, k, (base if k < 8 else synth_structured_cloud(36000, seed=50 + k))[k % 3::3][perm][:12000 - 2500 * (k % 4)].copy())
    e.keyframe_put(1, 0, base[:500].copy())
    e.keyframe_put(1, 2, base[500:1000].copy())                       # keyframe 1 of robot 1 is never stored
    received = vc._moved_copy(base, rigid_transform(0.0, 0.0, 0.002, 0.02, -0.01, 0.0), 3, 0.01, 4)
    received[::9, :3] += 2.5                                          # outliers for the RANSAC stage
    return received


@pytest.fixture(scope="module")
def store():
    e = ScanContextEngine()
    received = _fill_store(e)
    yield e, received
    e.close()


def _windows(keys, sn=SN):
    return np.broadcast_to(IDENT, (len(keys), 2 * sn + 1, 4, 4)).copy()


def _store_singles(e, received, keys, iters, sn=SN, **gate):
    return [e.geometric_verification_from_store(received, SRC_LEAF, 0, int(k), sn, _windows([k], sn)[0], LEAF, iters, THR, RATIO, SEED, **gate)
            for k in keys]


def _assert_store_entries(got, singles):
    T, ok, ns, nt, nc, ni = got
    for c, (T1, ok1, ns1, nt1, nc1, ni1) in enumerate(singles):
        assert (bool(ok[c]), ns, int(nt[c]), int(nc[c]), int(ni[c])) == (ok1, ns1, nt1, nc1, ni1), c
        assert np.array_equal(T[c].view(np.uint32), T1.view(np.uint32)), c


KEYS40 = [0, N_KF - 1, 3, 5, 9, 1, 10, 6, -1, N_KF, 2, 7, 4, 8, N_KF + 1, -2, 11, 0, 3, 10] * 2


def test_from_store_forty_candidates(store):
    """two rounds; keys at both ends of the trajectory and beyond them (shorter windows, smaller submaps), a min_tgt_points between
    the submaps' sizes, a min_src_points that gates all"""
    e, received = store
    assert len(KEYS40) == 40
    got = e.geometric_verification_batch_from_store(received, SRC_LEAF, 0, KEYS40, SN, _windows(KEYS40), LEAF, 64, THR, RATIO, SEED,
                                                    min_src_points=300, min_tgt_points=1000)
    singles = _store_singles(e, received, KEYS40[:20], 64, min_src_points=300, min_tgt_points=1000) * 2
    _assert_store_entries(got, singles)
    assert got[1].any() and not got[1].all() and len(set(got[3].tolist())) >= 5 and got[2] >= 300
    sizes = sorted(set(int(x) for x in got[3]))
    cut = sizes[len(sizes) // 2]                                      # gates the candidates with the smaller submaps only
    gated = e.geometric_verification_batch_from_store(received, SRC_LEAF, 0, KEYS40, SN, _windows(KEYS40), LEAF, 64, THR, RATIO, SEED,
                                                      min_src_points=300, min_tgt_points=cut)
    _assert_store_entries(gated, _store_singles(e, received, KEYS40[:20], 64, min_src_points=300, min_tgt_points=cut) * 2)
    small = gated[3] < cut
    assert small.any() and not small.all() and np.array_equal(gated[3], got[3])
    assert not gated[1][small].any() and not gated[4][small].any() and not gated[5][small].any()
    assert np.array_equal(gated[0][small], np.broadcast_to(IDENT, gated[0][small].shape))
    assert np.array_equal(gated[0][~small].view(np.uint32), got[0][~small].view(np.uint32))
    none = e.geometric_verification_batch_from_store(received, SRC_LEAF, 0, KEYS40, SN, _windows(KEYS40), LEAF, 64, THR, RATIO, SEED,
                                                     min_src_points=10 ** 7, min_tgt_points=1000)
    assert not none[1].any() and not none[4].any() and none[2] == got[2] and np.array_equal(none[3], got[3])
    assert np.array_equal(none[0], np.broadcast_to(IDENT, none[0].shape))
    empty = e.geometric_verification_batch_from_store(received, SRC_LEAF, 0, [], SN, _windows([]), LEAF, 64, THR, RATIO, SEED)
    assert empty[0].shape == (0, 4, 4) and empty[2] == got[2]         # no candidate: the received cloud's filtered size is still reported


# ---- errors: nothing is written -------------------------------------------------------------------------------------------------------
def _raw_batch(e, src, tgts, iters, stride=None, n=None, null_T=False, null_target=None, n_src=None):
    lib = e._lib
    s = np.ascontiguousarray(src, np.float32)
    arrs = [np.ascontiguousarray(t, np.float32) for t in tgts]
    ptrs = (c_void_p * max(1, len(arrs)))(*[a.ctypes.data for a in arrs])
    if null_target is not None:
        ptrs[null_target] = None
    counts = np.asarray([len(a) for a in arrs], np.int32)
    m = len(arrs) if n is None else n
    out = [np.full((max(len(arrs), 1), 16), 7.0, np.float32)] + [np.full(max(len(arrs), 1), 7, np.int32) for _ in range(3)]
    rc = lib.scl_geometric_verification_batch(e._h, s.ctypes.data_as(c_void_p), len(s) if n_src is None else n_src, ptrs,
                                              counts.ctypes.data_as(POINTER(c_int)), m, s.shape[1] * 4 if stride is None else stride, iters, THR, RATIO, SEED,
                                              None if null_T else out[0].ctypes.data_as(POINTER(c_float)), *[o.ctypes.data_as(POINTER(c_int)) for o in out[1:]])
    return rc, all((o == 7).all() for o in out)


def _raw_store(e, received, robot, keys, sn, iters, stride=None, n=None, null_T=False):
    lib = e._lib
    s = np.ascontiguousarray(received, np.float32)
    k = np.asarray(keys, np.int32)
    poses = _windows(keys, sn).astype(np.float32).reshape(-1)
    m = len(k) if n is None else n
    out = [np.full((max(len(k), 1), 16), 7.0, np.float32)] + [np.full(max(len(k), 1), 7, np.int32) for _ in range(4)]
    ns = c_int(7)
    ip = lambda a: a.ctypes.data_as(POINTER(c_int))
    rc = lib.scl_geometric_verification_batch_from_store(e._h, s.ctypes.data_as(c_void_p), len(s), s.shape[1] * 4 if stride is None else stride, SRC_LEAF,
                                                         robot, m, ip(k), sn, poses.ctypes.data_as(POINTER(c_float)), LEAF, 300, 1000,
                                                         iters, THR, RATIO, SEED, None if null_T else out[0].ctypes.data_as(POINTER(c_float)),
                                                         ip(out[1]), byref(ns), ip(out[2]), ip(out[3]), ip(out[4]))
    return rc, all((o == 7).all() for o in out) and ns.value == 7


def test_errors_write_nothing(store):
    e, received = store
    src, tgts = bc.source()[0], bc.clouds()[:3]
    for kw in (dict(null_T=True), dict(n=-1), dict(stride=10), dict(stride=14), dict(stride=8), dict(null_target=1), dict(n_src=-1)):
        assert _raw_batch(e, src, tgts, 9, **kw) == (INVALID_ARG, True), kw
    for iters in (0, -5, 2 ** 20 + 1):
        assert _raw_batch(e, src, tgts, iters) == (INVALID_ARG, True), iters
        assert _raw_store(e, received, 0, [3, 5], SN, iters) == (INVALID_ARG, True), iters
    for kw in (dict(null_T=True), dict(n=-1), dict(stride=16), dict(stride=12)):         # (the store's records are 32 bytes)
        assert _raw_store(e, received, 0, [3, 5], SN, 9, **kw) == (INVALID_ARG, True), kw
    assert _raw_store(e, received, 1, [0, 1, 0], 0, 9) == (INVALID_ARG, True)           # keyframe 1 of robot 1 was never stored
    assert _raw_store(e, received, 1, [0, 2, 2], 1, 9) == (INVALID_ARG, True)           # ... and lies inside these windows
    with pytest.raises(SclError) as ei:
        e.geometric_verification_batch_from_store(received, SRC_LEAF, 1, [0, 1], 0, _windows([0, 1], 0), LEAF, 9)
    assert ei.value.status == INVALID_ARG
    rc, untouched = _raw_store(e, received, 1, [0, 2], 0, 9)                             # the same robot, stored keyframes only
    assert rc == 0 and not untouched
    rc, untouched = _raw_batch(e, src, tgts, 9)
    assert rc == 0 and not untouched
    got = e.geometric_verification_batch(src, tgts, 9, THR, RATIO, SEED)                 # and the engine afterwards
    _assert_entries(got, _list_singles(9)[:3])


# ---- state ----------------------------------------------------------------------------------------------------------------------------
def test_engine_state_across_calls():
    """buffers reused and regrown: a smaller batch after a larger one and a larger after a smaller, each equal to the singles of an
    engine that never batched; a single call after a batch equals a fresh engine's"""
    src, all_tgts = bc.source()[0], bc.clouds()
    big_src = np.concatenate([src, src[::-1]])
    fresh = ScanContextEngine()
    want_small = _singles(fresh, src[:700], all_tgts[2:5], 9, THR, RATIO, SEED)
    want_big = _singles(fresh, big_src, all_tgts, 257, THR, RATIO, SEED)
    fresh.close()
    e = ScanContextEngine()
    try:
        _assert_entries(e.geometric_verification_batch(src[:700], all_tgts[2:5], 9, THR, RATIO, SEED), want_small)
        _assert_entries(e.geometric_verification_batch(big_src, all_tgts, 257, THR, RATIO, SEED), want_big)
        _assert_entries(e.geometric_verification_batch(src[:700], all_tgts[2:5], 9, THR, RATIO, SEED), want_small)
        one = e.geometric_verification(src, all_tgts[2], 300, THR, RATIO, SEED)
        ref = _list_singles(300)[2]
        assert one[1:] == ref[1:] and np.array_equal(one[0].view(np.uint32), ref[0].view(np.uint32))
    finally:
        e.close()


def test_icp_batch_after_a_verification_batch():
    """scl_loop_icp_batch_from_store shares the candidates' workspaces with the verification batch: after one it answers what a twin
    engine that never verified answers"""
    keys = [3, 6, 10, 1]
    out = []
    for verify_first in (False, True):
        e = ScanContextEngine()
        try:
            received = _fill_store(e)
            if verify_first:
                e.geometric_verification_batch_from_store(received, SRC_LEAF, 0, KEYS40[:9], SN, _windows(KEYS40[:9]), LEAF, 64, THR, RATIO, SEED)
                e.geometric_verification_batch(bc.source()[0], bc.clouds(), 9, THR, RATIO, SEED)
            pp = e.icp_default_params(); pp.max_iterations = 20
            out.append(e.loop_icp_batch_from_store(0, 4, IDENT, keys, 1, _windows(keys, 1), LEAF, pp))
        finally:
            e.close()
    a, b = out
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and a[4] == b[4] and np.array_equal(a[5], b[5])
    assert a[2].any()


def test_sharded_engine_equals_plain(store):
    """a 2-shard engine on one device: the calls run on the shard that owns the keyframe store"""
    e, received = store
    sh = ScanContextEngine(devices=[0, 0], exchange=1)
    try:
        _fill_store(sh)
        keys = KEYS40[:7]
        a = sh.geometric_verification_batch_from_store(received, SRC_LEAF, 0, keys, SN, _windows(keys), LEAF, 64, THR, RATIO, SEED)
        b = e.geometric_verification_batch_from_store(received, SRC_LEAF, 0, keys, SN, _windows(keys), LEAF, 64, THR, RATIO, SEED)
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and a[2] == b[2]
        assert all(np.array_equal(a[i], b[i]) for i in (1, 3, 4, 5))
        _assert_entries(sh.geometric_verification_batch(bc.source()[0], bc.clouds(), 9, THR, RATIO, SEED), _list_singles(9))
    finally:
        sh.close()
