"""scl_target_normals, scl_registration_eval_plane_batch and its two store forms (csrc/icp.hip, eval_plane_reduce_batch_kernel;
include/scl_engine.h "POINT-TO-PLANE REGISTRATION SCORING") on the inputs of tests/registration_plane_cases.py, which
tests/test_registration_plane_cases.py pins on the CPU checker and shows to be off the inlier knife edge and off the edge of every
normal's ball.

Bars.  The normals: the points without one are icpo_normals', every other normal n has | |n| - 1 | <= 2^-23 and
||C n - l_min n|| <= 2^-23 l_max for the float64 covariance C of its neighbours by brute force (an exact eigenvector rounded to
float meets 2^-24 l_max; the factor 2 covers the fp64 solver).  The eval: n_valid, n_inliers and sums[28] are
registration_eval_batch's, bit for bit; n_planar is the checker's; each of the 28 plane sums is within (n_planar + 10) * 2^-53 * M of
the checker's exact rational, the checker fed with the DEVICE's normals (the derivation is in the header; the comparison is made in
rationals).  The same call twice, around other batches, and the store forms against the host form agree bit for bit."""
from ctypes import POINTER, byref, c_double, c_float, c_int, c_void_p
from fractions import Fraction

import numpy as np
import pytest

import registration_plane_cases as pc
from scl_slam_amd import ScanContextEngine
from scl_slam_amd.synth import rigid_transform
from test_gpu_verification_batch import KEYS40, LEAF, N_KF, SN, SRC_LEAF, _fill_store, _windows
from test_registration_plane_cases import eigen_residuals

pytestmark = pytest.mark.gpu
INVALID_ARG = -1                                                      # include/scl_engine.h
IDENT = np.eye(4, dtype=np.float32)
STORE_MAX_DIST = 0.3
STORE_RADIUS = 1.5


@pytest.fixture(scope="module")
def eng():
    e = ScanContextEngine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def store():
    e = ScanContextEngine()
    received = _fill_store(e)
    yield e, received
    e.close()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(a, b):
    return (np.array_equal(a.n_valid, b.n_valid) and np.array_equal(a.n_inliers, b.n_inliers) and np.array_equal(a.n_planar, b.n_planar)
            and np.array_equal(_bits(a.sums), _bits(b.sums)))


_DEVICE_NORMALS = {}


def _device_normals(e, tgt, radius, width):
    """target_normals once per cloud object, radius and record width (the reference every candidate of every case shares)"""
    key = (id(tgt), radius, width)
    if key not in _DEVICE_NORMALS:
        _DEVICE_NORMALS[key] = (tgt, e.target_normals(np.ascontiguousarray(tgt[:, :width]), radius))
    return _DEVICE_NORMALS[key][1]


def _run_case(e, name, width=8):
    src, tgts, Ts, max_dist, radius = pc.case(name)
    s = np.ascontiguousarray(src[:, :width]); ts = [np.ascontiguousarray(t[:, :width]) for t in tgts]
    got = e.registration_eval_plane_batch(s, ts, Ts, max_dist, radius)
    point = e.registration_eval_batch(s, ts, Ts, max_dist)
    assert got.n_src == len(src) and len(got) == len(tgts) and got.sums.shape == (len(tgts), 29)
    assert np.array_equal(got.n_valid, point.n_valid) and np.array_equal(got.n_inliers, point.n_inliers)
    assert np.array_equal(_bits(got.sums[:, 28]), _bits(point.moments[:, 9]))
    worst = Fraction(0)
    for c, (t, T) in enumerate(zip(tgts, Ts)):
        nrm = _device_normals(e, t, radius, width) if len(t) else np.zeros((0, 3), np.float32)
        chk = pc.checker(src, t, T, max_dist, nrm)
        assert (int(got.n_valid[c]), int(got.n_inliers[c]), int(got.n_planar[c])) == (chk.n_valid, chk.n_inliers, chk.n_planar), (name, c)
        for k, (err, bound) in enumerate(pc.within_bound(got.sums[c], chk)):
            assert err <= bound, (name, c, k, float(err), float(bound))
            if bound:
                worst = max(worst, err / bound)
    print(name, "valid", got.n_valid.tolist()[:6], "inliers", got.n_inliers.tolist()[:6], "planar", got.n_planar.tolist()[:6],
          "worst error / bound", float(worst))
    assert _same(got, e.registration_eval_plane_batch(s, ts, Ts, max_dist, radius)), name
    return got


# ---- 1. the normals -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1.0, 0.5])
def test_target_normals_meet_the_eigen_residual_bound(eng, radius):
    tgt = pc.place()
    nrm = eng.target_normals(tgt, radius)
    assert nrm.shape == (len(tgt), 3) and nrm.dtype == np.float32
    few, unit, res = eigen_residuals(tgt, radius, nrm)
    ora = pc.cpu_normals_once(tgt, radius)
    assert np.array_equal(~(nrm != 0).any(1), ~(ora != 0).any(1)) and np.array_equal(~(nrm != 0).any(1), few)
    equal = (nrm == ora).all(1) | (nrm == -ora).all(1)
    print(f"radius {radius}: {int(few.sum())} without a normal, {equal[~few].mean():.4f} equal to the checker's up to a common sign, "
          f"worst | |n| - 1 | {unit[~few].max() * 2 ** 23:.3f} x 2^-23, worst residual {res[~few].max() * 2 ** 23:.3f} x 2^-23 l_max")
    assert (unit[~few] <= 2.0 ** -23).all() and (res[~few] <= 2.0 ** -23).all()


def test_target_normals_repeat_also_around_an_icp_batch(eng):
    tgt = pc.place()
    a = eng.target_normals(tgt, 1.0)
    assert np.array_equal(_bits(a), _bits(eng.target_normals(tgt, 1.0)))
    src, tgts, _, _, _ = pc.case("list")
    p = eng.icp_default_params(); p.max_iterations = 5; p.estimator = 1; p.normal_radius = 0.7
    eng.icp_align_batch(src, tgts[:3], p)
    eng.transform_cloud(src, IDENT)                                 # (writes the slot the normals share)
    assert np.array_equal(_bits(a), _bits(eng.target_normals(tgt, 1.0)))
    assert not np.array_equal(_bits(a), _bits(eng.target_normals(tgt, 0.5)))


@pytest.mark.parametrize("width", [3, 4, 8])
def test_target_normals_sizes_and_strides(eng, width):
    tgt = np.ascontiguousarray(pc.place()[:, :width])
    want = eng.target_normals(pc.place(), 1.0)
    assert np.array_equal(_bits(eng.target_normals(tgt, 1.0)), _bits(want))
    for n in (0, 1, 2):
        got = eng.target_normals(tgt[:n], 1.0)
        assert got.shape == (n, 3) and not got.any()
    three = eng.target_normals(tgt[:3], 100.0)                      # three points are a plane
    assert (np.abs(np.linalg.norm(three.astype(np.float64), axis=1) - 1) <= 2.0 ** -23).all()


# ---- 2. the eval on every case ----------------------------------------------------------------------------------------------------------
def test_the_list(eng):
    got = _run_case(eng, "list")
    assert got.n_valid[3] == 0 and not got.sums[3].any() and 0 < got.n_planar[0] < got.n_inliers[0] < 1500
    info = got.information(0)
    assert np.array_equal(info, info.T) and np.linalg.eigvalsh(info).min() > 0      # walls in two directions and a floor: all six axes
    assert got.gradient(0).tolist() == got.sums[0, 21:27].tolist() and 0 < got.rmse_plane(0) < pc.MAX_DIST and np.isnan(got.rmse_plane(3))


@pytest.mark.parametrize("n", [0, 1, 32, 33])
def test_candidate_counts_with_distinct_transforms(eng, n):
    if n == 0:
        got = eng.registration_eval_plane_batch(pc.source(), [], np.zeros((0, 4, 4), np.float32), pc.MAX_DIST, pc.RADIUS)
        assert len(got) == 0 and got.sums.shape == (0, 29)
        return
    got = _run_case(eng, f"n{n}")
    if n == 33:
        assert not np.array_equal(_bits(got.sums[32]), _bits(got.sums[2]))             # (candidate 32 is the list's third cloud again)


@pytest.mark.parametrize("n_src", (0,) + pc.SIZES + pc.SIZES_ONE)
def test_source_sizes(eng, n_src):
    """around the empty source, one workgroup of the reduction (256), several (4 097: 17), a lane's second trip (16 385) and the
    four-trip loop's second pass (65 537)"""
    if n_src == 0:
        _, tgts, Ts, max_dist, radius = pc.case("list")
        got = eng.registration_eval_plane_batch(pc.source()[:0], tgts, Ts, max_dist, radius)
        assert got.n_src == 0 and not got.n_valid.any() and not got.n_inliers.any() and not got.n_planar.any() and not got.sums.any()
        return
    got = _run_case(eng, f"src_{n_src}")
    assert got.n_valid.tolist() == ([n_src, n_src, n_src, 0, n_src] if n_src in pc.SIZES else [n_src])


@pytest.mark.parametrize("width", [3, 4])
def test_record_strides(eng, width):
    _run_case(eng, "list", width)


def test_isolated_target_points_are_inliers_without_a_plane(eng):
    got = _run_case(eng, "sparse")
    assert got.n_inliers[0] - got.n_planar[0] >= 40


def test_a_tiny_and_a_huge_radius(eng):
    tiny = _run_case(eng, "tiny_radius")
    assert not tiny.n_planar.any() and not tiny.sums[:, :28].any() and (tiny.sums[:, 28] > 0).all() and (tiny.n_inliers > 1000).all()
    huge = _run_case(eng, "huge_radius")
    assert np.array_equal(huge.n_planar, huge.n_inliers)


@pytest.mark.parametrize("name", ["tgt1", "tgt2"])
def test_targets_of_one_and_two_points(eng, name):
    got = _run_case(eng, name)
    assert (got.n_valid == 1500).all() and (got.n_inliers >= 1).all() and not got.n_planar.any() and not got.sums[:, :28].any()


@pytest.mark.parametrize("name", ["nan", "overflow", "maxd0", "all"])
def test_the_point_forms_edge_inputs(eng, name):
    got = _run_case(eng, name)
    if name == "maxd0":
        assert not got.n_inliers.any() and not got.sums.any()
    if name == "all":
        assert np.array_equal(got.n_inliers, got.n_valid)


def test_the_lattice_on_the_edge_is_kept(eng):
    got = _run_case(eng, pc.LATTICE)
    assert got.n_inliers.tolist() == [500] * 3 and got.n_planar.tolist() == [500] * 3 and got.sums[:, 28].tolist() == [125.0] * 3
    src, tgts, Ts, max_dist, radius = pc.case(pc.LATTICE)
    below = eng.registration_eval_plane_batch(src, tgts, Ts, float(np.nextafter(np.float32(max_dist), np.float32(0))), radius)
    assert below.n_valid.tolist() == [500] * 3 and not below.n_inliers.any() and not below.sums.any()


def test_the_corridor_is_free_along_x(eng):
    got = _run_case(eng, "corridor")
    for c in range(len(got)):
        lam, vec = np.linalg.eigh(got.information(c))
        print("corridor", c, "smallest : largest eigenvalue", lam[0] / lam[5], "eigenvector", np.round(vec[:, 0], 3).tolist())
        assert 0 <= lam[0] < 1e-3 * lam[5] and abs(vec[3, 0]) > 0.99


# ---- 3. state ------------------------------------------------------------------------------------------------------------------------
def test_other_calls_around_an_eval_answer_as_alone():
    """a point-to-plane ICP batch (whose normals live where these calls keep theirs), transform_cloud (which writes that slot of the
    single workspace) and a guessed verification batch answer the same before and after, and the eval the same around them"""
    e = ScanContextEngine()
    try:
        src, tgts, Ts, max_dist, radius = pc.case("src_4097")
        small = pc.case("list")[0]
        live = [t for t in tgts if len(t)]
        p = e.icp_default_params(); p.max_iterations = 8; p.estimator = 1; p.normal_radius = 0.8
        G = Ts[:3]

        def others():
            icp = e.icp_align_batch(small, live, p)
            moved = e.transform_cloud(small, Ts[0])
            ver = e.geometric_verification_batch_guess(small, live[:3], G, 9, 0.25, 0.45, 1)
            return [np.ascontiguousarray(x) for x in tuple(icp) + (moved,) + tuple(ver)]
        before = others()
        big = e.registration_eval_plane_batch(src, tgts, Ts, max_dist, radius)
        after = others()
        assert len(before) == len(after) and all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
        s2, t2, T2, m2, r2 = pc.case("src_255")                       # a smaller one in the grown buffers
        little = e.registration_eval_plane_batch(s2, t2, T2, m2, r2)
        assert _same(big, e.registration_eval_plane_batch(src, tgts, Ts, max_dist, radius))
        fresh = ScanContextEngine()
        try:
            assert _same(little, fresh.registration_eval_plane_batch(s2, t2, T2, m2, r2))
            assert _same(big, fresh.registration_eval_plane_batch(src, tgts, Ts, max_dist, radius))
        finally:
            fresh.close()
    finally:
        e.close()


# ---- 4. the store forms are the host form on the materialised clouds -------------------------------------------------------------------
def _store_transforms(n):
    return np.stack([rigid_transform(0, 0, np.radians(30.0 if c % 8 == 5 else 0.02 * c), 0.002 * c, -0.001 * c, 0).astype(np.float32)
                     for c in range(n)]) if n else np.zeros((0, 4, 4), np.float32)


def _submaps(e, keys, sn):
    subs = {}
    for k in keys:
        if k not in subs:
            subs[k] = e.submap_from_store(0, int(k), sn, _windows([k], sn)[0], LEAF, N_KF * 12000)
    return [subs[k] for k in keys]


def _assert_store_equals_host(got, host, src, subs, min_src_points, min_tgt_points):
    assert got.n_src == len(src) and got.n_tgts.tolist() == [len(s) for s in subs]
    gated = np.array([len(src) < min_src_points or len(s) < min_tgt_points for s in subs])
    for c in range(len(subs)):
        if gated[c]:
            assert got.n_valid[c] == 0 and got.n_inliers[c] == 0 and got.n_planar[c] == 0 and not got.sums[c].any(), c
        else:
            assert (got.n_valid[c], got.n_inliers[c], got.n_planar[c]) == (host.n_valid[c], host.n_inliers[c], host.n_planar[c]), c
            assert np.array_equal(_bits(got.sums[c]), _bits(host.sums[c])), c
    return gated


def _store_form(call, args, host, src, subs):
    got = call(*args, min_src_points=300, min_tgt_points=1000)
    _assert_store_equals_host(got, host, src, subs, 300, 1000)
    assert got.n_src >= 300 and got.n_planar.any() and len(set(got.n_tgts.tolist())) >= 5
    point = (call.__self__.registration_eval_batch_from_store if "registration" in call.__name__ else call.__self__.loop_eval_batch_from_store)(
        *args[:-1], min_src_points=300, min_tgt_points=1000)
    assert np.array_equal(got.n_valid, point.n_valid) and np.array_equal(got.n_inliers, point.n_inliers)
    assert np.array_equal(_bits(got.sums[:, 28]), _bits(point.moments[:, 9]))
    sizes = sorted(set(int(x) for x in got.n_tgts))
    cut = sizes[len(sizes) // 2]                                      # gates the candidates with the smaller submaps only
    some = call(*args, min_src_points=300, min_tgt_points=cut)
    gated = _assert_store_equals_host(some, host, src, subs, 300, cut)
    assert gated.any() and not gated.all()
    none = call(*args, min_src_points=10 ** 7, min_tgt_points=1000)
    assert _assert_store_equals_host(none, host, src, subs, 10 ** 7, 1000).all()
    return got


def test_received_form_forty_candidates(store):
    e, received = store
    Ts = _store_transforms(40)
    filt = e.voxel_grid(received, SRC_LEAF)
    subs = _submaps(e, KEYS40, SN)
    host = e.registration_eval_plane_batch(filt, subs, Ts, STORE_MAX_DIST, STORE_RADIUS)
    got = _store_form(e.registration_eval_plane_batch_from_store,
                      (received, SRC_LEAF, 0, KEYS40, SN, _windows(KEYS40), LEAF, Ts, STORE_MAX_DIST, STORE_RADIUS), host, filt, subs)
    print("n_src", got.n_src, "n_tgts", got.n_tgts.tolist(), "planar", got.n_planar.tolist())
    empty = e.registration_eval_plane_batch_from_store(received, SRC_LEAF, 0, [], SN, _windows([]), LEAF, _store_transforms(0), STORE_MAX_DIST, STORE_RADIUS)
    assert len(empty) == 0 and empty.n_src == got.n_src


def test_loop_form_forty_candidates(store):
    e, _ = store
    Ts = _store_transforms(40)
    src = e.submap_from_store(0, 4, 0, IDENT[None], LEAF, N_KF * 12000)
    subs = _submaps(e, KEYS40, 1)
    host = e.registration_eval_plane_batch(src, subs, Ts, STORE_MAX_DIST, STORE_RADIUS)
    _store_form(e.loop_eval_plane_batch_from_store, (0, 4, IDENT, KEYS40, 1, _windows(KEYS40, 1), LEAF, Ts, STORE_MAX_DIST, STORE_RADIUS), host, src, subs)
    empty = e.loop_eval_plane_batch_from_store(0, 4, IDENT, [], 1, _windows([], 1), LEAF, _store_transforms(0), STORE_MAX_DIST, STORE_RADIUS)
    assert len(empty) == 0 and empty.n_src == len(src)


def test_sharded_engine_equals_plain(store):
    """a 2-shard engine on one device: the calls run on the shard that owns the keyframe store"""
    e, received = store
    sh = ScanContextEngine(devices=[0, 0], exchange=1)
    try:
        _fill_store(sh)
        keys = KEYS40[:7]
        Ts = _store_transforms(7)
        args = (received, SRC_LEAF, 0, keys, SN, _windows(keys), LEAF, Ts, STORE_MAX_DIST, STORE_RADIUS)
        a, b = sh.registration_eval_plane_batch_from_store(*args), e.registration_eval_plane_batch_from_store(*args)
        assert _same(a, b) and a.n_src == b.n_src and np.array_equal(a.n_tgts, b.n_tgts) and b.n_planar.any()
        largs = (0, 4, IDENT, keys, 1, _windows(keys, 1), LEAF, Ts, STORE_MAX_DIST, STORE_RADIUS)
        a, b = sh.loop_eval_plane_batch_from_store(*largs), e.loop_eval_plane_batch_from_store(*largs)
        assert _same(a, b) and a.n_src == b.n_src and np.array_equal(a.n_tgts, b.n_tgts)
        src, tgts, T, max_dist, radius = pc.case("list")
        assert _same(sh.registration_eval_plane_batch(src, tgts, T, max_dist, radius), e.registration_eval_plane_batch(src, tgts, T, max_dist, radius))
        assert np.array_equal(_bits(sh.target_normals(pc.place(), 1.0)), _bits(e.target_normals(pc.place(), 1.0)))
    finally:
        sh.close()


# ---- 5. errors write nothing ---------------------------------------------------------------------------------------------------------------
def _outs(m, want):
    nv = np.full(max(m, 1), 7, np.int32); ni = np.full(max(m, 1), 7, np.int32); npl = np.full(max(m, 1), 7, np.int32)
    su = np.full((max(m, 1), 29), 7.0)
    ptrs = [a.ctypes.data_as(POINTER(c_int)) if w else None for a, w in zip((nv, ni, npl), want)]
    ptrs.append(su.ctypes.data_as(POINTER(c_double)) if want[3] else None)
    return (nv, ni, npl, su), ptrs


def _raw_host(e, src, tgts, Ts, max_dist, radius, stride=None, n=None, null_target=None, n_src=None, null_T=False, want=(True,) * 4):
    s = np.ascontiguousarray(src, np.float32)
    arrs = [np.ascontiguousarray(t, np.float32) for t in tgts]
    ptrs = (c_void_p * max(1, len(arrs)))(*[a.ctypes.data for a in arrs])
    if null_target is not None:
        ptrs[null_target] = None
    counts = np.asarray([len(a) for a in arrs] or [0], np.int32)
    m = len(arrs) if n is None else n
    T = np.ascontiguousarray(Ts, np.float32)
    out, op = _outs(len(arrs), want)
    rc_ = e._lib.scl_registration_eval_plane_batch(e._h, s.ctypes.data_as(c_void_p), len(s) if n_src is None else n_src, ptrs,
                                                   counts.ctypes.data_as(POINTER(c_int)), m, s.shape[1] * 4 if stride is None else stride,
                                                   None if null_T else T.ctypes.data_as(POINTER(c_float)), max_dist, radius, *op)
    return rc_, all((o == 7).all() for o in out), out


def _raw_store(e, received, robot, keys, sn, Ts, max_dist, radius, stride=None, n=None, null_T=False, want=(True,) * 4, loop=False, key_cur=4):
    s = np.ascontiguousarray(received, np.float32)
    k = np.asarray(keys, np.int32)
    poses = _windows(keys, sn).astype(np.float32).reshape(-1)
    m = len(k) if n is None else n
    T = np.ascontiguousarray(Ts, np.float32)
    fp, ip = (lambda a: a.ctypes.data_as(POINTER(c_float))), (lambda a: a.ctypes.data_as(POINTER(c_int)))
    out, op = _outs(len(k), want)
    ns = c_int(7); nt = np.full(max(len(k), 1), 7, np.int32)
    if loop:
        rc_ = e._lib.scl_loop_eval_plane_batch_from_store(e._h, robot, key_cur, fp(IDENT.reshape(16).copy()), m, ip(k), sn, fp(poses), LEAF,
                                                          None if null_T else fp(T), 300, 1000, max_dist, radius, *op, byref(ns), ip(nt))
    else:
        rc_ = e._lib.scl_registration_eval_plane_batch_from_store(e._h, s.ctypes.data_as(c_void_p), len(s), s.shape[1] * 4 if stride is None else stride,
                                                                  SRC_LEAF, robot, m, ip(k), sn, fp(poses), LEAF, None if null_T else fp(T), 300, 1000,
                                                                  max_dist, radius, *op, byref(ns), ip(nt))
    return rc_, all((o == 7).all() for o in out) and ns.value == 7 and (nt == 7).all()


def _raw_normals(e, tgt, n, stride, radius, null_tgt=False, null_out=False):
    t = np.ascontiguousarray(tgt, np.float32)
    out = np.full((max(len(t), 1), 3), 7.0, np.float32)
    rc_ = e._lib.scl_target_normals(e._h, None if null_tgt else t.ctypes.data_as(c_void_p), n, stride, radius,
                                    None if null_out else out.ctypes.data_as(POINTER(c_float)))
    return rc_, bool((out == 7).all())


BAD_RADII = (np.nan, 0.0, -0.0, -1.0, -np.inf)                       # what the ICP's parameter check refuses in normal_radius


def test_errors_write_nothing(store):
    e, received = store
    src, tgts, Ts, max_dist, radius = pc.case("list")
    tgts, Ts = tgts[:3], Ts[:3]
    T2 = _store_transforms(2)
    for loop in (False, True):
        assert _raw_store(e, received, 0, [3, 5], SN, T2, 0.3, 1.5, null_T=True, loop=loop) == (INVALID_ARG, True)
        assert _raw_store(e, received, 0, [3, 5], SN, T2, 0.3, 1.5, want=(False,) * 4, loop=loop) == (INVALID_ARG, True)
        assert _raw_store(e, received, 0, [3, 5], SN, T2, 0.3, 1.5, n=-1, loop=loop) == (INVALID_ARG, True)
        for bad in (np.nan, np.inf, -1.0):
            assert _raw_store(e, received, 0, [3, 5], SN, T2, bad, 1.5, loop=loop) == (INVALID_ARG, True), bad
        for bad in BAD_RADII:
            assert _raw_store(e, received, 0, [3, 5], SN, T2, 0.3, bad, loop=loop) == (INVALID_ARG, True), bad
        B = T2.copy(); B[1, 2, 3] = np.inf
        assert _raw_store(e, received, 0, [3, 5], SN, B, 0.3, 1.5, loop=loop) == (INVALID_ARG, True)
        assert _raw_store(e, received, 1, [0, 1, 0], 0, _store_transforms(3), 0.3, 1.5, loop=loop, key_cur=0) == (INVALID_ARG, True)   # never stored
    assert _raw_store(e, received, 0, [3, 5], SN, T2, 0.3, 1.5, stride=16) == (INVALID_ARG, True)             # (the store's records are 32 bytes)
    assert _raw_host(e, src, tgts, Ts, max_dist, radius, null_T=True)[:2] == (INVALID_ARG, True)
    assert _raw_host(e, src, tgts, Ts, max_dist, radius, want=(False,) * 4)[:2] == (INVALID_ARG, True)
    for bad in (np.nan, np.inf, -np.inf, -1.0, -1e-300):
        assert _raw_host(e, src, tgts, Ts, bad, radius)[:2] == (INVALID_ARG, True), bad
    for bad in BAD_RADII:
        assert _raw_host(e, src, tgts, Ts, max_dist, bad)[:2] == (INVALID_ARG, True), bad
    B = Ts.copy(); B[0, 0, 0] = np.nan
    assert _raw_host(e, src, tgts, B, max_dist, radius)[:2] == (INVALID_ARG, True)
    for kw in (dict(n=-1), dict(stride=10), dict(stride=14), dict(stride=8), dict(null_target=1), dict(n_src=-1)):
        assert _raw_host(e, src, tgts, Ts, max_dist, radius, **kw)[:2] == (INVALID_ARG, True), kw
    place = pc.place()
    for bad in BAD_RADII:
        assert _raw_normals(e, place, len(place), 32, bad) == (INVALID_ARG, True), bad
    for kw in (dict(stride=10), dict(stride=8), dict(stride=14)):
        assert _raw_normals(e, place, len(place), radius=1.0, **kw) == (INVALID_ARG, True), kw
    assert _raw_normals(e, place, -1, 32, 1.0) == (INVALID_ARG, True)
    assert _raw_normals(e, place, len(place), 32, 1.0, null_tgt=True) == (INVALID_ARG, True)
    assert _raw_normals(e, place, len(place), 32, 1.0, null_out=True)[0] == INVALID_ARG
    assert _raw_normals(e, place, 0, 32, 1.0, null_tgt=True, null_out=True) == (0, True)
    # no candidate needs no transforms and no outputs; one output alone is enough
    assert _raw_host(e, src, [], np.zeros((0, 4, 4)), max_dist, radius, null_T=True, want=(False,) * 4)[:2] == (0, True)
    ref = e.registration_eval_plane_batch(src, tgts, Ts, max_dist, radius)
    for only in range(4):
        code, _, out = _raw_host(e, src, tgts, Ts, max_dist, radius, want=tuple(k == only for k in range(4)))
        assert code == 0 and [(o == 7).all() for o in out] == [k != only for k in range(4)]
        want = (ref.n_valid, ref.n_inliers, ref.n_planar, ref.sums)[only]
        assert out[only][:3].tobytes() == np.ascontiguousarray(want).tobytes()
    code, untouched = _raw_store(e, received, 1, [0, 2], 0, T2, 0.3, 1.5)
    assert code == 0 and not untouched
    assert _same(ref, e.registration_eval_plane_batch(src, tgts, Ts, max_dist, radius))                     # and the engine afterwards
