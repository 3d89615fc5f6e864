"""scl_geometric_verification_batch_guess and scl_geometric_verification_batch_from_store_guess (csrc/icp.hip, the batched verification
with a per-candidate source; include/scl_engine.h "THE BATCHED VERIFICATION WITH INITIAL GUESSES") on the list of
tests/verification_guess_cases.py, which tests/test_verification_guess_cases.py pins on the CPU checker.

Bars.  T_fit, success, pair count and inlier count of entry c are the single call's for (transform_cloud(src, G_c), tgt_c) on the same
engine, T_fit compared as uint32; counts and success equal the checker's on the finite rows, T_fit within TOL = 1e-5 of it (the
project's bar, tests/test_gpu_verification_batch.py).  T is the double product T_fit * G_c restated with Python scalars in the
header's order, bit for bit."""
import functools
from ctypes import POINTER, byref, c_float, c_int, c_void_p

import numpy as np
import pytest

import oracle_binding as ob
import verification_batch_cases as bc
import verification_guess_cases as gc
from scl_slam_amd import ScanContextEngine
from scl_slam_amd.synth import rigid_transform, synth_scan
from test_gpu_verification_batch import KEYS40, LEAF, N_KF, SN, SRC_LEAF, _fill_store, _windows
from test_loop_guess_from_shift import SECTORS_TURNED, sign_case
from test_verification_guess_cases import checker

pytestmark = pytest.mark.gpu
TOL = 1e-5
INVALID_ARG = -1                                                      # include/scl_engine.h
IDENT = np.eye(4, dtype=np.float32)
THR, RATIO, SEED = gc.THRESHOLD, gc.RATIO, gc.SEED


@pytest.fixture(scope="module")
def eng():
    e = ScanContextEngine()
    yield e
    e.close()


def compose(T_fit, G):
    """T_fit * G with G's last row taken as (0, 0, 0, 1): ((a0 b0 + a1 b1) + a2 b2) + a3 b3 in double (Python floats), rounded once"""
    out = np.empty((4, 4), np.float32)
    for r in range(4):
        a0, a1, a2, a3 = (float(v) for v in T_fit[r])
        for c in range(4):
            b0, b1, b2, b3 = float(G[0, c]), float(G[1, c]), float(G[2, c]), (1.0 if c == 3 else 0.0)
            out[r, c] = np.float32(((a0 * b0 + a1 * b1) + a2 * b2) + a3 * b3)
    return out


def _singles(e, src, tgts, guesses, *args):
    """the definition: the single call on the source moved by the candidate's guess"""
    return [e.geometric_verification(e.transform_cloud(src, g) if len(src) else src, t, *args) for t, g in zip(tgts, guesses)]


def _assert_entries(got, singles, guesses, bits=True):
    T, ok, nc, ni, Tf = got
    assert T.shape == Tf.shape == (len(singles), 4, 4) and len(ok) == len(nc) == len(ni) == len(singles)
    for c, (T1, ok1, nc1, ni1) in enumerate(singles):
        assert (bool(ok[c]), int(nc[c]), int(ni[c])) == (ok1, nc1, ni1), (c, ok[c], nc[c], ni[c], ok1, nc1, ni1)
        assert np.array_equal(Tf[c].view(np.uint32), T1.view(np.uint32)), c
        want = compose(Tf[c], guesses[c])
        assert np.array_equal(T[c].view(np.uint32), want.view(np.uint32)) if bits else np.array_equal(T[c], want, equal_nan=True), c


@functools.lru_cache(maxsize=None)
def _list_singles(iterations):
    """per candidate of the list on an engine of its own (shared by the tests that batch the same list)"""
    e = ScanContextEngine()
    try:
        return _singles(e, gc.source()[0], gc.clouds(), gc.guesses(), iterations, THR, RATIO, SEED)
    finally:
        e.close()


# ---- 5. the whole list in one call --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iterations", gc.ITERATIONS)
def test_whole_list_in_one_call(eng, iterations):
    G = gc.guesses()
    got = eng.geometric_verification_batch_guess(gc.source()[0], gc.clouds(), G, iterations, THR, RATIO, SEED)
    _assert_entries(got, _list_singles(iterations), G)
    for c, (To, oko, nco, nio) in enumerate(checker(iterations)):
        print(iterations, gc.names()[c], bool(got[1][c]), int(got[2][c]), int(got[3][c]), float(np.abs(got[4][c] - To).max()))
        assert (bool(got[1][c]), int(got[2][c]), int(got[3][c])) == (oko, nco, nio)
        assert np.abs(got[4][c] - To).max() < TOL
    res = dict(zip(gc.names(), zip(*got[1:4])))
    if iterations >= 9:                                               # what the guess is for, on the device
        assert all(res[n] == (True, 1995, 1995) for n in ("yaw_3", "yaw_20", "yaw_90", "moved_6dof"))
        assert res["matching"][0] and not res["matching_again"][0]


# ---- 6. identity guesses: the unguessed batch -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("iterations", [9, 300])
def test_identity_guesses_equal_the_unguessed_batch(eng, iterations):
    src, tgts = gc.source()[0], gc.clouds()
    plain = eng.geometric_verification_batch(src, tgts, iterations, THR, RATIO, SEED)
    got = eng.geometric_verification_batch_guess(src, tgts, np.broadcast_to(IDENT, (len(tgts), 4, 4)), iterations, THR, RATIO, SEED)
    assert np.array_equal(got[4].view(np.uint32), plain[0].view(np.uint32))
    assert all(np.array_equal(got[i], plain[i]) for i in (1, 2, 3))
    assert np.array_equal(got[0], got[4])                             # T == T_fit


# ---- 7. edges of the move kernel and of the rounds -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 32, 33])
def test_candidate_counts_with_distinct_guesses(eng, n):
    """rounds of 32: the 33rd candidate gets its own guess, not the 1st's"""
    m = len(gc.names())
    order = [c % m for c in range(n)]
    G = np.stack([(rigid_transform(0, 0, np.radians(0.3 * c), 0.01 * c, 0, 0) @ gc.guesses()[order[c]].astype(np.float64)).astype(np.float32)
                  for c in range(n)]) if n else np.zeros((0, 4, 4), np.float32)
    assert len({g.tobytes() for g in G}) == n
    tgts = [gc.clouds()[c] for c in order]
    got = eng.geometric_verification_batch_guess(gc.source()[0], tgts, G, 9, THR, RATIO, SEED)
    assert got[0].shape == got[4].shape == (n, 4, 4)
    _assert_entries(got, _singles(eng, gc.source()[0], tgts, G, 9, THR, RATIO, SEED), G)
    if n == 33:
        assert (int(got[2][32]), int(got[3][32])) != (int(got[2][0]), int(got[3][0])) or not np.array_equal(got[4][32], got[4][0])


EDGE = ("matching", "yaw_20", "first_3", "empty", "moved_6dof", "matching_again")


def _edge_list():
    idx = [gc.names().index(n) for n in EDGE]
    return [gc.clouds()[i] for i in idx], gc.guesses()[idx]


def _long_source(n):
    s = gc.source()[0]
    parts = [s.copy() for _ in range((n + len(s) - 1) // len(s))]
    for k, p in enumerate(parts):
        p[:, 0] += np.float32(0.013 * k)
    return np.ascontiguousarray(np.concatenate(parts)[:n])


@pytest.mark.parametrize("n_src", [0, 1, 2, 3, 255, 256, 257, 4097])
def test_source_sizes(eng, n_src):
    """around the early exits, one workgroup of the move kernel (256) and one trip of the pairs kernel (4 096)"""
    tgts, G = _edge_list()
    src = _long_source(n_src) if n_src else gc.source()[0][:0]
    got = eng.geometric_verification_batch_guess(src, tgts, G, 9, THR, RATIO, SEED)
    _assert_entries(got, _singles(eng, src, tgts, G, 9, THR, RATIO, SEED), G)
    finite = int(np.isfinite(src[:, :3]).all(1).sum())
    assert [int(x) for x in got[2]] == [0 if n == "empty" else finite for n in EDGE]
    if n_src < 3:                                                     # nothing is sampled: T_fit = identity, T = G with the last row 0 0 0 1
        assert not got[1].any() and np.array_equal(got[4], np.broadcast_to(IDENT, got[4].shape))
        assert np.array_equal(got[0][:, :3], G[:, :3]) and np.array_equal(got[0][:, 3], IDENT[[3] * len(G)])
    if n_src == 4097:
        assert got[1][EDGE.index("moved_6dof")] and not got[1][EDGE.index("matching_again")]


@pytest.mark.parametrize("width", [3, 4, 8])
def test_record_strides(eng, width):
    tgts, G = _edge_list()
    src = np.ascontiguousarray(gc.source()[0][:, :width])
    tgts = [np.ascontiguousarray(c[:, :width]) for c in tgts]
    got = eng.geometric_verification_batch_guess(src, tgts, G, 9, THR, RATIO, SEED)
    _assert_entries(got, _singles(eng, src, tgts, G, 9, THR, RATIO, SEED), G)
    want = [_list_singles(9)[gc.names().index(n)] for n in EDGE]      # the fields behind z play no part
    _assert_entries(got, want, G)


def test_points_that_overflow_only_after_the_move(eng):
    """a finite point times 1e38 is infinite: such a row finds no neighbour and is no pair, as in the single call.  (The rows that stay
    finite lie 1e37 m out: their squared distances overflow, so they find no neighbour either -- what counts is the single call's answer.)"""
    tgts, G = _edge_list()
    G = G.copy()
    G[1] = np.diag([1e38, 1.0, 1.0, 1.0]).astype(np.float32)          # |x| > 3.4 overflows
    G[2, 0, 3] = 3e38; G[2, 0, 0] = 1e30                              # the translation added to a large product
    src = gc.finite_source()
    got = eng.geometric_verification_batch_guess(src, tgts, G, 9, THR, RATIO, SEED)
    singles = _singles(eng, src, tgts, G, 9, THR, RATIO, SEED)
    _assert_entries(got, singles, G, bits=False)
    moved = eng.transform_cloud(src, G[1])
    still = int(np.isfinite(moved[:, :3]).all(1).sum())
    print("rows finite after the move", still, "of", len(src), "pairs", got[2])
    assert 0 < still < len(src) and int(got[2][1]) == singles[1][2] <= still and int(got[2][0]) == len(src)
    assert not got[1][1] and np.array_equal(got[4][1], IDENT)


# ---- 8. from the keyframe store --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def store():
    e = ScanContextEngine()
    received = _fill_store(e)
    yield e, received
    e.close()


def _store_guesses(n):
    """small motions (most candidates of the scan's place still verify), every eighth a wrong 30 degrees; all distinct"""
    return np.stack([rigid_transform(0, 0, np.radians(30.0 if c % 8 == 5 else 0.02 * c), 0.002 * c, -0.001 * c, 0).astype(np.float32)
                     for c in range(n)]) if n else np.zeros((0, 4, 4), np.float32)


def _store_singles(e, received, keys, G, iters, min_src_points, min_tgt_points):
    """scl_geometric_verification(scl_transform_cloud(scl_voxel_grid(src, src_leaf), G_c), scl_submap_from_store(key_c, ...)) behind
    the size gate -> [(T_fit, ok, n_src_filtered, n_tgt, n_corr, n_inl, gated)]"""
    filt = e.voxel_grid(received, SRC_LEAF)
    subs, out = {}, []
    for k, g in zip(keys, G):
        if k not in subs:
            subs[k] = e.submap_from_store(0, int(k), SN, _windows([k])[0], LEAF, N_KF * 12000)
        sub = subs[k]
        if len(filt) < min_src_points or len(sub) < min_tgt_points:
            out.append((IDENT, False, len(filt), len(sub), 0, 0, True))
        else:
            T1, ok1, nc1, ni1 = e.geometric_verification(e.transform_cloud(filt, g), sub, iters, THR, RATIO, SEED)
            out.append((T1, ok1, len(filt), len(sub), nc1, ni1, False))
    return out


def _assert_store_entries(got, singles, G):
    T, ok, ns, nt, nc, ni, Tf = got
    for c, (T1, ok1, ns1, nt1, nc1, ni1, gated) in enumerate(singles):
        assert (bool(ok[c]), ns, int(nt[c]), int(nc[c]), int(ni[c])) == (ok1, ns1, nt1, nc1, ni1), c
        assert np.array_equal(Tf[c].view(np.uint32), T1.view(np.uint32)), c
        want = IDENT if gated else compose(Tf[c], G[c])
        assert np.array_equal(T[c].view(np.uint32), want.view(np.uint32)), c


def test_from_store_forty_candidates(store):
    """two rounds, keys at both ends of the trajectory and beyond, a min_tgt_points between the submaps' sizes and a min_src_points
    that gates all: against the composition of single calls"""
    e, received = store
    G = _store_guesses(40)
    args = (received, SRC_LEAF, 0, KEYS40, SN, _windows(KEYS40), LEAF)
    plain = e.geometric_verification_batch_from_store(*args, 64, THR, RATIO, SEED, min_src_points=300, min_tgt_points=1000)
    got = e.geometric_verification_batch_from_store_guess(*args, G, 64, THR, RATIO, SEED, min_src_points=300, min_tgt_points=1000)
    _assert_store_entries(got, _store_singles(e, received, KEYS40, G, 64, 300, 1000), G)
    assert got[2] == plain[2] and np.array_equal(got[3], plain[3])    # the sizes are the unguessed form's
    assert got[1].any() and not got[1].all() and got[2] >= 300
    wrong = np.arange(40) % 8 == 5
    print("verified", got[1].astype(int), "inliers", got[5])
    assert not got[1][wrong & (got[3] >= 1000)].any()
    sizes = sorted(set(int(x) for x in got[3]))
    cut = sizes[len(sizes) // 2]                                      # gates the candidates with the smaller submaps only
    gated = e.geometric_verification_batch_from_store_guess(*args, G, 64, THR, RATIO, SEED, min_src_points=300, min_tgt_points=cut)
    _assert_store_entries(gated, _store_singles(e, received, KEYS40, G, 64, 300, cut), G)
    small = gated[3] < cut
    assert small.any() and not small.all() and np.array_equal(gated[3], got[3])
    assert not gated[1][small].any() and not gated[4][small].any() and not gated[5][small].any()
    assert np.array_equal(gated[0][small], np.broadcast_to(IDENT, gated[0][small].shape))      # T = T_fit = identity, not the guess
    assert np.array_equal(gated[6][small], np.broadcast_to(IDENT, gated[6][small].shape))
    assert np.array_equal(gated[0][~small].view(np.uint32), got[0][~small].view(np.uint32))
    none = e.geometric_verification_batch_from_store_guess(*args, G, 64, THR, RATIO, SEED, min_src_points=10 ** 7, min_tgt_points=1000)
    assert not none[1].any() and not none[4].any() and none[2] == got[2] and np.array_equal(none[3], got[3])
    assert np.array_equal(none[0], np.broadcast_to(IDENT, none[0].shape)) and np.array_equal(none[6], none[0])
    empty = e.geometric_verification_batch_from_store_guess(received, SRC_LEAF, 0, [], SN, _windows([]), LEAF, _store_guesses(0), 64, THR, RATIO, SEED)
    assert empty[0].shape == empty[6].shape == (0, 4, 4) and empty[2] == got[2]


# ---- 9. end to end: search -> shift -> guess -> verification ----------------------------------------------------------------------------
def test_search_shift_guess_verification_end_to_end():
    """Two robots on the 20 x 60 grid.  Robot 0's keyframe 1 is a scan at pose_pre in its world frame; the received keyframe is the
    same place seen with the sensor turned by 7 sectors, at pose_cur in the other robot's world frame (the received cloud is in that
    frame, DM.h:1333).  The ranked search reports the shift, scl_loop_guess_from_shift turns it and the two poses into the guess, and
    with it the store form verifies the candidate it cannot verify without."""
    cloud, turned, want_shift = sign_case()
    pose_pre = np.float32([14.0, -6.5, 0.4, 0.02, -0.015, 1.1])
    pose_cur = np.float32([-35.0, 22.0, -0.3, -0.01, 0.025, -2.3])
    e = ScanContextEngine(num_ring=20, num_sector=60)
    try:
        M_pre, M_cur = e.pose_to_matrix(*[float(v) for v in pose_pre]), e.pose_to_matrix(*[float(v) for v in pose_cur])
        other = synth_scan(20000, seed=11)
        for k, c in enumerate((other, cloud)):                         # robot 0's keyframes: descriptors and clouds, sensor frame
            e.make_and_save(c, 0, k)
            e.keyframe_put(0, k, c)
        e.make_and_save(turned, 1, 0)                                 # the received keyframe's descriptor: key 2
        ids, shifts, dists, found = e.sc_search_range([2], 0, 2, 2)
        print("search", ids, shifts, dists, found)
        assert found[0] == 2 and ids[0, 0] == 1 and shifts[0, 0] == want_shift and want_shift == SECTORS_TURNED
        assert e.get_index(int(ids[0, 0])) == (0, 1)
        received = e.transform_cloud(turned, M_cur)                   # what the other robot sends
        received[::400, 0] = np.nan                                   # rows the voxel filter drops
        G = np.stack([e.loop_guess_from_shift(int(shifts[0, j]), 60, pose_cur, pose_pre if ids[0, j] == 1 else np.zeros(6)) for j in range(2)])
        keys = [int(e.get_index(int(i))[1]) for i in ids[0]]
        windows = np.stack([M_pre if k == 1 else IDENT for k in keys]).reshape(2, 1, 4, 4)
        args = (received, 0.1, 0, keys, 0, windows, 0.1)             # (a 0.05 m leaf overflows the voxel index here: the filter would pass the cloud on)
        got = e.geometric_verification_batch_from_store_guess(*args, G, 300, THR, RATIO, SEED)
        plain = e.geometric_verification_batch_from_store(*args, 300, THR, RATIO, SEED)
        print("guessed", got[1], got[2], got[3], got[4], got[5], "unguessed", plain[1], plain[4], plain[5])
        assert 300 <= got[2] == plain[2] <= int(np.isfinite(received[:, 0]).sum()) and np.array_equal(got[3], plain[3])
        assert got[1][0] and got[4][0] == got[5][0] == got[2]         # every row the filter kept is a pair and an inlier
        assert not got[1][1]                                          # the other place stays unverified
        assert not plain[1][0]                                        # the same inputs without the guess
        assert np.abs(got[6][0] - IDENT).max() < 0.05                 # the fit is the residual; T is the whole motion
        assert np.array_equal(got[0][0].view(np.uint32), compose(got[6][0], G[0]).view(np.uint32))
        back = received[np.isfinite(received[:, 0]), :3].astype(np.float64) @ got[0][0, :3, :3].astype(np.float64).T + got[0][0, :3, 3]
        there = e.transform_cloud(cloud, M_pre)[np.isfinite(received[:, 0]), :3]
        assert np.linalg.norm(back - there, axis=1).max() < 0.05
    finally:
        e.close()


# ---- 10. errors write nothing; state ---------------------------------------------------------------------------------------------------
def _raw_batch(e, src, tgts, G, iters, stride=None, n=None, null_T=False, null_target=None, n_src=None, null_G=False):
    s = np.ascontiguousarray(src, np.float32)
    arrs = [np.ascontiguousarray(t, np.float32) for t in tgts]
    ptrs = (c_void_p * max(1, len(arrs)))(*[a.ctypes.data for a in arrs])
    if null_target is not None:
        ptrs[null_target] = None
    counts = np.asarray([len(a) for a in arrs], np.int32)
    m = len(arrs) if n is None else n
    g = np.ascontiguousarray(G, np.float32)
    fp, ip = (lambda a: a.ctypes.data_as(POINTER(c_float))), (lambda a: a.ctypes.data_as(POINTER(c_int)))
    out = [np.full((max(len(arrs), 1), 16), 7.0, np.float32) for _ in range(2)] + [np.full(max(len(arrs), 1), 7, np.int32) for _ in range(3)]
    rc = e._lib.scl_geometric_verification_batch_guess(e._h, s.ctypes.data_as(c_void_p), len(s) if n_src is None else n_src, ptrs, ip(counts), m,
                                                       s.shape[1] * 4 if stride is None else stride, None if null_G else fp(g), iters, THR, RATIO, SEED,
                                                       None if null_T else fp(out[0]), fp(out[1]), ip(out[2]), ip(out[3]), ip(out[4]))
    return rc, all((o == 7).all() for o in out)


def _raw_store(e, received, robot, keys, sn, G, iters, stride=None, n=None, null_T=False, null_G=False):
    s = np.ascontiguousarray(received, np.float32)
    k = np.asarray(keys, np.int32)
    poses = _windows(keys, sn).astype(np.float32).reshape(-1)
    m = len(k) if n is None else n
    g = np.ascontiguousarray(G, np.float32)
    fp, ip = (lambda a: a.ctypes.data_as(POINTER(c_float))), (lambda a: a.ctypes.data_as(POINTER(c_int)))
    out = [np.full((max(len(k), 1), 16), 7.0, np.float32) for _ in range(2)] + [np.full(max(len(k), 1), 7, np.int32) for _ in range(4)]
    ns = c_int(7)
    rc = e._lib.scl_geometric_verification_batch_from_store_guess(e._h, s.ctypes.data_as(c_void_p), len(s), s.shape[1] * 4 if stride is None else stride,
                                                                  SRC_LEAF, robot, m, ip(k), sn, fp(poses), LEAF, None if null_G else fp(g), 300, 1000,
                                                                  iters, THR, RATIO, SEED, None if null_T else fp(out[0]), fp(out[1]),
                                                                  ip(out[2]), byref(ns), ip(out[3]), ip(out[4]), ip(out[5]))
    return rc, all((o == 7).all() for o in out) and ns.value == 7


def _bad_guesses(G):
    for c, r, k, v in ((0, 0, 0, np.nan), (len(G) - 1, 2, 3, np.inf), (1 % len(G), 1, 2, -np.inf)):
        B = G.copy(); B[c, r, k] = v
        yield B


def test_errors_write_nothing(store):
    e, received = store
    src, tgts, G = gc.source()[0], gc.clouds()[:3], gc.guesses()[:3]
    G2 = _store_guesses(2)
    assert _raw_batch(e, src, tgts, G, 9, null_G=True) == (INVALID_ARG, True)
    assert _raw_store(e, received, 0, [3, 5], SN, G2, 9, null_G=True) == (INVALID_ARG, True)
    for B in _bad_guesses(G):
        assert _raw_batch(e, src, tgts, B, 9) == (INVALID_ARG, True)
    for B in _bad_guesses(G2):
        assert _raw_store(e, received, 0, [3, 5], SN, B, 9) == (INVALID_ARG, True)
    # everything the unguessed pair refuses (tests/test_gpu_verification_batch.py)
    for kw in (dict(null_T=True), dict(n=-1), dict(stride=10), dict(stride=14), dict(stride=8), dict(null_target=1), dict(n_src=-1)):
        assert _raw_batch(e, src, tgts, G, 9, **kw) == (INVALID_ARG, True), kw
    for iters in (0, -5, 2 ** 20 + 1):
        assert _raw_batch(e, src, tgts, G, iters) == (INVALID_ARG, True), iters
        assert _raw_store(e, received, 0, [3, 5], SN, G2, iters) == (INVALID_ARG, True), iters
    for kw in (dict(null_T=True), dict(n=-1), dict(stride=16), dict(stride=12)):         # (the store's records are 32 bytes)
        assert _raw_store(e, received, 0, [3, 5], SN, G2, 9, **kw) == (INVALID_ARG, True), kw
    assert _raw_store(e, received, 1, [0, 1, 0], 0, _store_guesses(3), 9) == (INVALID_ARG, True)   # keyframe 1 of robot 1 was never stored
    assert _raw_store(e, received, 1, [0, 2, 2], 1, _store_guesses(3), 9) == (INVALID_ARG, True)   # ... and lies inside these windows
    # a non-finite LAST row is not read; no candidate needs no guesses
    L = G.copy(); L[:, 3] = np.nan
    rc, untouched = _raw_batch(e, src, tgts, L, 9)
    assert rc == 0 and not untouched
    assert _raw_batch(e, src, [], np.zeros((0, 4, 4)), 9, null_G=True) == (0, True)
    rc, untouched = _raw_store(e, received, 1, [0, 2], 0, G2, 9)
    assert rc == 0 and not untouched
    got = e.geometric_verification_batch_guess(src, tgts, L, 9, THR, RATIO, SEED)        # and the engine afterwards
    _assert_entries(got, _list_singles(9)[:3], G)


def test_an_unguessed_batch_around_a_guessed_one():
    """the guessed call grows per-candidate clouds (a larger n_src here): the unguessed batch before and after it answers alike, and
    like an engine that never took a guess"""
    src, tgts = bc.source()[0], bc.clouds()
    big = _long_source(5000)
    e = ScanContextEngine()
    try:
        before = e.geometric_verification_batch(src, tgts, 9, THR, RATIO, SEED)
        G = gc.guesses()
        got = e.geometric_verification_batch_guess(big, gc.clouds(), G, 9, THR, RATIO, SEED)
        after = e.geometric_verification_batch(src, tgts, 9, THR, RATIO, SEED)
        assert np.array_equal(before[0].view(np.uint32), after[0].view(np.uint32)) and all(np.array_equal(before[i], after[i]) for i in (1, 2, 3))
        _assert_entries(got, _singles(e, big, gc.clouds(), G, 9, THR, RATIO, SEED), G)
        again = e.geometric_verification_batch_guess(src, gc.clouds(), G, 9, THR, RATIO, SEED)   # a smaller one in the grown buffers
        _assert_entries(again, _list_singles(9), G)
    finally:
        e.close()


def test_icp_batch_after_a_guessed_verification_batch():
    """scl_loop_icp_batch_from_store shares the candidates' workspaces (their working clouds too): after guessed batches it answers what
    a twin engine that never verified answers"""
    keys = [3, 6, 10, 1]
    out = []
    for verify_first in (False, True):
        e = ScanContextEngine()
        try:
            received = _fill_store(e)
            if verify_first:
                e.geometric_verification_batch_from_store_guess(received, SRC_LEAF, 0, KEYS40[:9], SN, _windows(KEYS40[:9]), LEAF, _store_guesses(9),
                                                                64, THR, RATIO, SEED)
                e.geometric_verification_batch_guess(gc.source()[0], gc.clouds(), gc.guesses(), 9, THR, RATIO, SEED)
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
        G = _store_guesses(7)
        a = sh.geometric_verification_batch_from_store_guess(received, SRC_LEAF, 0, keys, SN, _windows(keys), LEAF, G, 64, THR, RATIO, SEED)
        b = e.geometric_verification_batch_from_store_guess(received, SRC_LEAF, 0, keys, SN, _windows(keys), LEAF, G, 64, THR, RATIO, SEED)
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[6].view(np.uint32), b[6].view(np.uint32)) and a[2] == b[2]
        assert all(np.array_equal(a[i], b[i]) for i in (1, 3, 4, 5))
        _assert_entries(sh.geometric_verification_batch_guess(gc.source()[0], gc.clouds(), gc.guesses(), 9, THR, RATIO, SEED), _list_singles(9), gc.guesses())
    finally:
        sh.close()
