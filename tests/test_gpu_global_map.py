"""The global voxel map (include/scl_engine.h "GLOBAL MAP") on the device against the checker of tests/global_map_cases.py, bit for bit:
records as bytes, and the stats the checker has (keyframes, points added and skipped, occupied voxels).  The inputs are pinned without
a GPU by tests/test_global_map_cases.py."""
from ctypes import POINTER, byref, c_double, c_int, c_void_p

import numpy as np
import pytest

import global_map_cases as gm
from scl_slam_amd import SclError, ScanContextEngine

pytestmark = pytest.mark.gpu
INVALID_ARG = -1


@pytest.fixture(scope="module")
def eng():
    e = ScanContextEngine(num_ring=20, num_sector=60)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng2():
    """a second engine: the fresh builds the updates are compared with, and the twin that never builds a map of its own until asked"""
    e = ScanContextEngine(num_ring=20, num_sector=60)
    yield e
    e.close()


def ids(kfs):
    return [k[0] for k in kfs], [k[1] for k in kfs]


def put(e, kfs):
    for k in kfs:
        e.keyframe_put(k[0], k[1], k[2])


def set_all(e, kfs, poses=None):
    e.map_set_keyframes(*ids(kfs), [k[3] for k in kfs] if poses is None else poses)


def fresh(e, leaf, kfs, slots=0):
    """the clouds into the store, a new map of `slots` starting slots (0: the default), every keyframe set in one call"""
    put(e, kfs)
    e.selftest_map_capacity(slots)
    e.map_reset(leaf)
    set_all(e, kfs)
    e.selftest_map_capacity(0)


def same(e, m, box=None):
    got, want = e.map_extract(box), m.records(box)
    assert len(got) == len(want), (len(got), len(want))
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(got.view("<u4").reshape(-1, 4) != want.view("<u4").reshape(-1, 4))[:1]
        raise AssertionError(f"records differ, first at word {bad}: {got[bad // 4]} vs {want[bad // 4]}")
    st = e.map_stats().as_dict()
    assert {k: st[k] for k in m.stats()} == m.stats(), (st, m.stats())
    assert st["capacity"] & (st["capacity"] - 1) == 0 and 2 * st["occupied_voxels"] <= st["capacity"]
    return got


def lattice_kfs(coords, per_voxel=2, leaf=0.5):
    return [(0, 0, gm.lattice_voxels(coords, leaf, per_voxel), gm.IDENTITY.copy())]


# ---- table and growth ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 1000])
def test_maps_of_so_many_voxels_from_64_slots(eng, count):
    kfs = lattice_kfs(gm.spread_voxels(count, count)) if count else [(0, 0, np.zeros((0, 4), np.float32), gm.IDENTITY.copy())]
    fresh(eng, 0.5, kfs, slots=64)
    rec = same(eng, gm.build(0.5, kfs))
    assert len(rec) == count and (rec["n"] == 2).all()
    st = eng.map_stats().as_dict()
    assert st["capacity"] == max(64, gm.capacity_for(count)) and 64 << st["growths"] == st["capacity"]
    if count == 1000:
        assert st["growths"] >= 2                                      # growth inside ONE call, more than once


def test_one_voxel_takes_5000_points_from_40_keyframes(eng):
    rs = np.random.RandomState(21)
    kfs = []
    for k in range(40):
        pose = gm.IDENTITY.copy(); pose[:3] = rs.randint(-64, 64, 3) * 0.25          # dyadic: p + t is exact
        cloud = np.zeros((125, 4), np.float32)
        cloud[:, :3] = (np.array([3.0, -2.0, 1.0]) * 0.5 + rs.uniform(0.05, 0.45, (125, 3)) - pose[:3]).astype(np.float32)
        kfs.append((0, k, cloud, pose))
    m = gm.build(0.5, kfs)
    assert list(m.table) == [gm.make_key(3, -2, 1)]
    fresh(eng, 0.5, kfs, slots=64)
    rec = same(eng, m)
    assert rec["n"].tolist() == [5000]


def test_keys_that_collide_into_one_probe_chain(eng):
    chain = gm.colliding_voxels(20, 64)
    kfs = lattice_kfs(chain, per_voxel=3)
    fresh(eng, 0.5, kfs, slots=64)
    same(eng, gm.build(0.5, kfs))
    st = eng.map_stats().as_dict()
    assert (st["capacity"], st["growths"], st["occupied_voxels"]) == (64, 0, 20)     # 20 keys behind each other from one slot, no growth


def test_the_same_records_whatever_the_starting_capacity(eng):
    leaf, kfs = gm.gpu_inputs("overlap")
    want = gm.build(leaf, kfs)
    seen = []
    for slots in (64, 4096, 0):
        fresh(eng, leaf, kfs, slots=slots)
        seen.append((same(eng, want).tobytes(), eng.map_stats().as_dict()["capacity"]))
    assert len({s[0] for s in seen}) == 1 and seen[2][1] == 1 << 20 and seen[1][1] >= 4096


# ---- determinism ------------------------------------------------------------------------------------------------------------------

def test_the_same_bits_twice_and_in_reverse_order(eng):
    leaf, kfs = gm.gpu_inputs("overlap")
    want = gm.build(leaf, kfs)
    fresh(eng, leaf, kfs, slots=64)
    a = same(eng, want).tobytes()
    fresh(eng, leaf, kfs, slots=64)
    assert same(eng, want).tobytes() == a
    fresh(eng, leaf, kfs[::-1], slots=64)
    assert same(eng, want).tobytes() == a


def test_one_call_of_257_keyframes_against_257_calls_of_one(eng):
    leaf, kfs = gm.gpu_inputs("kf257")
    want = gm.build(leaf, kfs)
    fresh(eng, leaf, kfs, slots=4096)
    a = same(eng, want).tobytes()
    eng.map_reset(leaf)
    for k in kfs:
        set_all(eng, [k])
    assert same(eng, want).tobytes() == a


# ---- updates ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["one", "half", "all"])
def test_a_repose_equals_a_fresh_build_at_the_final_poses(eng, eng2, which):
    leaf, kfs = gm.gpu_inputs("repose64")
    moved = {"one": [17], "half": list(range(0, 64, 2)), "all": list(range(64))}[which]
    fresh(eng, leaf, kfs, slots=64)
    sub = [kfs[i] for i in moved]
    set_all(eng, sub, [k[4][0] for k in sub])
    final = [k[:3] + ((k[4][0] if i in moved else k[3]),) for i, k in enumerate(kfs)]
    fresh(eng2, leaf, final)
    want = gm.build(leaf, final)
    a, b = same(eng, want), same(eng2, want)
    assert a.tobytes() == b.tobytes()
    sa, sb = eng.map_stats().as_dict(), eng2.map_stats().as_dict()
    assert all(sa[k] == sb[k] for k in ("keyframes", "points_added", "points_skipped", "occupied_voxels"))


def test_remove_everything_then_build_again(eng):
    leaf, kfs = gm.gpu_inputs("overlap")
    fresh(eng, leaf, kfs, slots=64)
    eng.map_remove_keyframes(*ids(kfs))
    st = eng.map_stats().as_dict()
    assert (st["keyframes"], st["points_added"], st["points_skipped"], st["occupied_voxels"]) == (0, 0, 0, 0)
    out = np.full(8, 0xABABABAB, np.uint32); n = c_int(-5)
    assert eng._lib.scl_map_extract(eng._h, None, out.ctypes.data_as(c_void_p), 2, byref(n)) == 0
    assert n.value == 0 and (out == 0xABABABAB).all()                  # nothing to write, nothing written
    set_all(eng, kfs)
    same(eng, gm.build(leaf, kfs))


def test_a_pose_given_twice_bitwise_is_skipped(eng):
    leaf, kfs = gm.gpu_inputs("overlap")
    fresh(eng, leaf, kfs)
    before = (eng.map_extract().tobytes(), eng.map_stats().as_dict())
    set_all(eng, kfs)
    set_all(eng, kfs[3:5])
    assert (eng.map_extract().tobytes(), eng.map_stats().as_dict()) == before


def test_a_repose_after_a_growth_that_dropped_emptied_voxels(eng):
    """Three sets of poses A, B, C of about 1 550 voxels each, from 64 slots.  A: 4 096 slots.  A -> B: 3 100 keys pass the load bound, a
    growth (nothing is emptied yet: the subtraction follows the reserve pass).  B -> C: 4 650 keys pass it again, and this growth drops
    the voxels of A, empty since the step before.  C -> A then inserts them anew."""
    leaf, kfs = gm.gpu_inputs("regrow")
    A = [k[:4] for k in kfs]; B = [k[:3] + (k[4][0],) for k in kfs]; C = [k[:3] + (k[4][1],) for k in kfs]
    sizes = [len(gm.build(leaf, X).table) for X in (A, B, C)]
    assert max(sizes) <= 2048 < sizes[0] + sizes[1] - 200 and sizes[0] + sizes[1] + sizes[2] - 400 > 4096    # what the steps below rely on
    fresh(eng, leaf, A, slots=64)
    g = [eng.map_stats().as_dict()["growths"]]
    for X in (B, C):
        set_all(eng, X)
        same(eng, gm.build(leaf, X))
        g.append(eng.map_stats().as_dict()["growths"])
    assert g[0] < g[1] < g[2], g
    set_all(eng, A[:9])                                                # back, in two steps
    same(eng, gm.build(leaf, A[:9] + C[9:]))
    set_all(eng, A[9:])
    same(eng, gm.build(leaf, A))


# ---- geometry ---------------------------------------------------------------------------------------------------------------------

def test_points_on_faces_and_negative_coordinates(eng):
    cloud = gm.face_lattice(0.5)
    kfs = [(0, 0, cloud, gm.IDENTITY.copy()), (0, 1, cloud, gm.HALF_TURN_Z.copy())]
    fresh(eng, 0.5, kfs, slots=64)
    rec = same(eng, gm.build(0.5, kfs))
    assert (rec["x"] < 0).any() and (rec["z"] < 0).any()


def test_poses_8_km_from_the_origin(eng):
    leaf, kfs = gm.gpu_inputs("far8km")
    fresh(eng, leaf, kfs)
    rec = same(eng, gm.build(leaf, kfs))
    assert rec["x"].min() > 7900 and rec["y"].max() < -7900


def test_both_ends_of_the_range_and_every_kind_of_skipped_point(eng):
    pts = [(1048575.5, 0.5, 0.5), (1048576.5, 0.5, 0.5), (-1048575.5, 0.5, -1048575.5), (-1048576.5, 0.5, 0.5),
           (np.nan, 0.0, 0.0), (0.0, np.inf, 0.0), (0.0, 0.0, -np.inf), (0.5, 0.5, 0.5), (0.25, 1048575.25, 0.75)]
    cloud = np.zeros((len(pts), 4), np.float32); cloud[:, :3] = pts
    far = gm.IDENTITY.copy(); far[0] = 1048576.0                       # in range in the sensor frame, out of it after the move
    inside = np.zeros((2, 4), np.float32); inside[:, :3] = [(0.5, 1.5, 0.5), (-0.5, 1.5, 0.5)]
    empty = np.zeros((0, 4), np.float32)
    kfs = [(0, 0, cloud, gm.IDENTITY.copy()), (0, 1, inside, far), (0, 2, empty, gm.IDENTITY.copy()), (1, 0, empty, far)]
    m = gm.build(1.0, kfs)
    assert m.stats() == {"keyframes": 4, "points_added": 5, "points_skipped": 6, "occupied_voxels": 5}
    fresh(eng, 1.0, kfs, slots=64)
    rec = same(eng, m)
    assert rec["x"].max() == np.float32(1048575.5) and rec["x"].min() == np.float32(-1048575.5)
    eng.map_remove_keyframes([0, 0], [1, 0]); m.remove(0, 1); m.remove(0, 0)       # the skipped points' count is undone with them
    assert m.stats()["points_skipped"] == 0
    same(eng, m)


@pytest.mark.parametrize("floats", [3, 4, 8])
def test_strides_12_16_and_32(floats):
    leaf, kfs = gm.gpu_inputs(f"stride{4 * floats}")
    with ScanContextEngine(num_ring=20, num_sector=60) as e:
        fresh(e, leaf, kfs, slots=64)
        same(e, gm.build(leaf, kfs))


# ---- size -------------------------------------------------------------------------------------------------------------------------

def test_past_the_int32_index_of_the_submap_call(eng):
    leaf, kfs = gm.gpu_inputs("overflow")
    cloud = kfs[0][2]
    span = cloud[:, :3].max(axis=0) - cloud[:, :3].min(axis=0)
    assert np.prod(np.floor(span / leaf) + 1) > 2 ** 31                # PCL's linear index does not fit: "Leaf size is too small"
    sub = eng.assemble_submap([cloud], [np.eye(4, dtype=np.float32)], leaf)
    assert len(sub) == len(cloud) and np.array_equal(sub, cloud)       # the parent's route hands the input back unfiltered
    fresh(eng, leaf, kfs)
    rec = same(eng, gm.build(leaf, kfs))
    assert 0 < len(rec) <= len(cloud)


def test_70000_points_in_one_keyframe(eng):
    leaf, kfs = gm.gpu_inputs("big70k")
    assert len(kfs[0][2]) > 65536
    fresh(eng, leaf, kfs, slots=4096)
    same(eng, gm.build(leaf, kfs))


# ---- extract ----------------------------------------------------------------------------------------------------------------------

def test_the_box_is_closed_a_box_of_nothing_count_only_and_a_short_buffer(eng):
    cloud = gm.face_lattice(0.5)
    kfs = [(0, 0, cloud, gm.IDENTITY.copy())]
    fresh(eng, 0.5, kfs)
    m = gm.build(0.5, kfs)
    rec = m.records()
    lo, hi = rec[10], rec[-10]                                          # the box's corners ARE centroids (exact: the lattice is dyadic)
    box = [float(min(lo[a], hi[a])) for a in "xyz"] + [float(max(lo[a], hi[a])) for a in "xyz"]
    got = same(eng, m, box)
    assert 0 < len(got) < len(rec) and lo.tobytes() in {r.tobytes() for r in got} and hi.tobytes() in {r.tobytes() for r in got}
    open_box = [np.nextafter(box[0], np.inf)] + box[1:]                # one ulp inside the lower x face: that plane of centroids leaves
    assert len(same(eng, m, open_box)) < len(got)
    assert len(same(eng, m, [100, 100, 100, 200, 200, 200])) == 0 and len(same(eng, m, [1, 1, 1, -1, -1, -1])) == 0
    assert eng.map_extract(count_only=True) == len(rec) and eng.map_extract(box, count_only=True) == len(got)
    out = np.full(4 * len(rec), 0xABABABAB, np.uint32); n = c_int(-5)
    rc = eng._lib.scl_map_extract(eng._h, None, out.ctypes.data_as(c_void_p), len(rec) - 1, byref(n))
    assert rc == INVALID_ARG and n.value == -5 and (out == 0xABABABAB).all()      # one too small: an error that writes nothing
    assert eng._lib.scl_map_extract(eng._h, None, out.ctypes.data_as(c_void_p), len(rec), byref(n)) == 0 and n.value == len(rec)
    assert out.tobytes() == rec.tobytes()


def test_ascending_keys_across_the_32_bit_border_of_the_key(eng):
    coords = [(0, 0, 0), (5, 0, 0), (0, 2048, 0), (0, -2048, 0), (3, 2047, 0), (0, 0, 1), (0, 0, -1), (0, 0, 2), (7, -1, -1), (-7, 1, 1),
              (0, 0, -3), (0, 0, 3), (1, 0, -2)]
    keys = [gm.make_key(*c) for c in coords]
    assert len({k & 0xffffffff for k in keys}) < len(keys) and len({k >> 32 for k in keys}) > 5     # equal low words, many high words
    kfs = lattice_kfs(coords, per_voxel=1)
    fresh(eng, 0.5, kfs, slots=64)
    rec = same(eng, gm.build(0.5, kfs))
    order = sorted(range(len(coords)), key=lambda i: keys[i])
    assert [tuple(np.floor(np.array([r["x"], r["y"], r["z"]]) / 0.5).astype(int)) for r in rec] == [coords[i] for i in order]


# ---- errors and state -------------------------------------------------------------------------------------------------------------

def test_every_error_leaves_the_map_as_it_was(eng):
    leaf, kfs = gm.gpu_inputs("overlap")
    with ScanContextEngine(num_ring=20, num_sector=60) as e:           # no map yet
        put(e, kfs[:1])
        for call in (lambda: set_all(e, kfs[:1]), lambda: e.map_remove_keyframes([0], [0]), e.map_extract, e.map_stats):
            with pytest.raises(SclError) as err:
                call()
            assert err.value.status == INVALID_ARG and "no map yet" in str(err.value)
    fresh(eng, leaf, kfs[:8], slots=64)
    put(eng, kfs[8:])
    before = (eng.map_extract().tobytes(), eng.map_stats().as_dict())
    r, x = ids(kfs)
    good = [k[3] for k in kfs]

    def pose_with(i, **kw):
        p = [v.copy() for v in good]
        for name, v in kw.items():
            if name == "at":
                p[i][v[0]] = v[1]
            else:
                p[i][3:] *= np.sqrt(v) / np.linalg.norm(p[i][3:])
        return p
    lib, h = eng._lib, eng._h
    ip = lambda a: np.ascontiguousarray(a, np.int32).ctypes.data_as(POINTER(c_int))
    bad_calls = [
        lambda: eng.map_set_keyframes(r, x, pose_with(9, at=(2, np.nan))), lambda: eng.map_set_keyframes(r, x, pose_with(2, at=(5, np.inf))),
        lambda: eng.map_set_keyframes(r, x, pose_with(10, norm2=0.24)), lambda: eng.map_set_keyframes(r, x, pose_with(1, norm2=4.1)),
        lambda: eng.map_set_keyframes(r + [r[3]], x + [x[3]], good + [good[3]]),                   # listed twice
        lambda: eng.map_set_keyframes(r[:9] + [0], x[:9] + [500], good[:10]),                       # not in the store
        lambda: eng.map_set_keyframes(r[:9] + [7], x[:9] + [0], good[:10]),
        lambda: eng.map_set_keyframes(r[:9] + [-1], x[:9] + [0], good[:10]),
        lambda: eng.map_remove_keyframes(r[:9], x[:9]),                                             # keyframe 8 is not in the map
        lambda: eng.map_remove_keyframes([0, 0], [2, 2]),
        lambda: eng.map_reset(0.0), lambda: eng.map_reset(-0.4), lambda: eng.map_reset(np.nan), lambda: eng.map_reset(np.inf),
        lambda: eng.map_extract([0, 0, 0, np.nan, 1, 1]),
        lambda: eng._check(lib.scl_map_set_keyframes(h, ip(r), ip(x), None, 3), "NULL poses"),
        lambda: eng._check(lib.scl_map_set_keyframes(h, None, ip(x), np.concatenate(good).ctypes.data_as(POINTER(c_double)), 3), "NULL robots"),
        lambda: eng._check(lib.scl_map_set_keyframes(h, ip(r), ip(x), np.concatenate(good).ctypes.data_as(POINTER(c_double)), -1), "n < 0"),
        lambda: eng._check(lib.scl_map_remove_keyframes(h, ip(r), None, 2), "NULL indices"),
        lambda: eng._check(lib.scl_map_remove_keyframes(h, ip(r), ip(x), -2), "n < 0"),
        lambda: eng._check(lib.scl_map_extract(h, None, None, 0, None), "NULL n_out"),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(SclError) as err:
            call()
        assert err.value.status == INVALID_ARG, (i, str(err.value))
        assert (eng.map_extract().tobytes(), eng.map_stats().as_dict()) == before, i
    set_all(eng, kfs)                                                  # and the map still works
    same(eng, gm.build(leaf, kfs))


def test_a_replaced_stored_cloud_is_refused_until_reset(eng):
    leaf, kfs = gm.gpu_inputs("overlap")
    fresh(eng, leaf, kfs[:4])
    before = (eng.map_extract().tobytes(), eng.map_stats().as_dict())
    eng.keyframe_put(0, 2, kfs[5][2])                                  # keyframe 2's cloud replaced: its old points cannot be subtracted
    for call in (lambda: eng.map_set_keyframes([0], [2], [kfs[5][3]]), lambda: eng.map_remove_keyframes([0], [2]),
                 lambda: eng.map_set_keyframes([0, 0], [1, 2], [kfs[1][3], kfs[2][3]])):
        with pytest.raises(SclError) as err:
            call()
        assert err.value.status == INVALID_ARG and "reset" in str(err.value)
        assert (eng.map_extract().tobytes(), eng.map_stats().as_dict()) == before
    set_all(eng, [kfs[0], kfs[1], kfs[3]])                             # the others go on (skipped: same poses)
    eng.map_reset(leaf)
    now = [kfs[0], kfs[1], (0, 2, kfs[5][2], kfs[5][3]), kfs[3]]
    set_all(eng, now)
    same(eng, gm.build(leaf, now))


def test_a_twin_engine_answers_the_same_before_and_after_map_calls(eng, eng2):
    from scl_slam_amd.synth import rigid_transform, synth_structured_cloud
    src = synth_structured_cloud(3000, seed=3, stride_floats=4)
    T = rigid_transform(0.01, -0.02, 0.05, 0.3, -0.2, 0.05)
    tgts = []
    for k in range(2):
        t = src.copy()
        t[:, :3] = (src[:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3] * (k + 1)).astype(np.float32)
        tgts.append(t)

    def answers(e):
        icp = e.icp_align_batch(src, tgts)
        return [np.asarray(a).tobytes() for a in icp] + [e.voxel_grid(src, 0.4).tobytes()]
    a0, b0 = answers(eng), answers(eng2)
    assert a0 == b0
    leaf, kfs = gm.gpu_inputs("overlap")
    fresh(eng, leaf, kfs, slots=64)
    eng.map_extract(); eng.map_remove_keyframes(*ids(kfs[:3]))
    assert answers(eng) == a0 and answers(eng2) == b0
    same(eng, gm.build(leaf, kfs[3:]))                                 # and the ICP and the filter left the map alone


def test_two_shards_keep_the_map_on_the_primary():
    leaf, kfs = gm.gpu_inputs("robots2")
    with ScanContextEngine(num_ring=20, num_sector=60, devices=[0, 0], exchange=1) as e:
        fresh(e, leaf, kfs, slots=64)
        same(e, gm.build(leaf, kfs))
        with pytest.raises(SclError) as err:
            e.map_remove_keyframes([1], [400])
        assert err.value.status == INVALID_ARG and "not in the store" in str(err.value)      # the primary's message reaches the front
        e.map_remove_keyframes(*ids(kfs[:4]))
        same(e, gm.build(leaf, kfs[4:]))


def test_timing_is_reported_under_profiling(eng):
    leaf, kfs = gm.gpu_inputs("overlap")
    put(eng, kfs)
    eng.selftest_map_capacity(64); eng.map_reset(leaf); eng.selftest_map_capacity(0)
    eng.profile_enable(1)
    try:
        set_all(eng, kfs)
        integrate, grow, _ = eng.map_last_timing()
        eng.map_extract()
        extract = eng.map_last_timing()[2]
    finally:
        eng.profile_enable(0)
    assert integrate > 0 and grow > 0 and extract > 0


# ---- end to end -------------------------------------------------------------------------------------------------------------------

def test_the_chain_from_search_to_the_map():
    """The chain of tests/test_gpu_pgo_chain.py restated (five places, inter-robot search -> guessed ICP from the store -> scoring ->
    scl_loop_pose_between -> scl_loop_covariance -> scl_pcm_select -> scl_pgo_optimize), its poses_out handed to
    scl_map_set_keyframes.  Both robots' clouds are in the store, robot 1's as it saw the place (turned by its sector shift): at the
    planted truth A_k = B_k Rz_k^-1 its cloud falls onto robot 0's point for point, so a solved graph collapses each revisited place
    onto itself and the drifted odometry -- 5 .. 25 cm and 10 .. 50 mrad off -- does not."""
    import icp_guess_cases as gc
    import pcm_cases as pc
    import pgo_cases as pg
    from scl_slam_amd import PgoParams
    from scl_slam_amd.synth import rigid_transform, synth_scan
    from test_gpu_pgo_chain import K, SECTORS, WRONG, _pose7

    W = rigid_transform(0.01, -0.02, 0.7, 40.0, -25.0, 0.5)
    odom_var = [1e-6] * 3 + [1e-4] * 3
    e = ScanContextEngine(num_ring=20, num_sector=60)
    try:
        clouds = [synth_scan(20000, seed=7 + 10 * k) for k in range(K)]
        poses_pre = [np.float32([14.0 + 9 * k, -6.5 + 4 * k, 0.4 - 0.1 * k, 0.02, -0.015, 1.1 + 0.3 * k]) for k in range(K)]
        for k in range(K):
            e.make_and_save(clouds[k], 0, k)
            e.keyframe_put(0, k, clouds[k])
        poses_a, poses_b, zs, covs, truth_a, truth_b, seen = [], [], [], [], [], [], []
        for k in range(K):
            Rz = rigid_transform(0.0, 0.0, np.radians(6.0 * SECTORS[k]), 0, 0, 0)
            M_pre = gc.pose_matrix(poses_pre[k])
            pose_cur = np.float32(e.matrix_to_pose(np.linalg.inv(W) @ M_pre @ np.linalg.inv(Rz)))
            M_cur = gc.pose_matrix(pose_cur)
            turned = clouds[k].copy()
            turned[:, :3] = (clouds[k][:, :3].astype(np.float64) @ Rz[:3, :3].T).astype(np.float32)
            received = turned.copy()
            xyz = turned[:, :3].astype(np.float64) @ M_cur[:3, :3].T + M_cur[:3, 3]
            received[:, :3] = (xyz + gc.NOISE * np.random.RandomState(90 + k).standard_normal(xyz.shape)).astype(np.float32)
            e.make_and_save(turned, 1, k)
            e.keyframe_put(1, k, turned); seen.append(turned)
            ids_, shifts, dists, found = e.sc_search_inter([K + k], 2, robot_pre=0)
            assert found[0] >= 1 and e.get_index(int(ids_[0, 0])) == (0, k) and shifts[0, 0] == SECTORS[k]
            G = e.loop_guess_from_shift(int(shifts[0, 0]), 60, pose_cur, poses_pre[k])[None]
            args = (received, gc.E2E_LEAF, 0, [k], 0, M_pre.astype(np.float32).reshape(1, 1, 4, 4), gc.E2E_LEAF)
            icp = e.icp_align_batch_from_store_guess(*args, G)
            ev = e.registration_eval_batch_from_store(*args, icp[0], 0.5)
            s2 = ev.moments[0, 9] / max(1, int(ev.n_inliers[0]) - 6)
            zs.append(e.loop_pose_between(icp[0][0], pose_cur, poses_pre[k])[0]); covs.append(ScanContextEngine.loop_covariance(ev.information(0), s2))
            poses_a.append(_pose7(M_cur)); poses_b.append(_pose7(M_pre))
            truth_b.append(_pose7(M_pre)); truth_a.append(_pose7(M_pre @ np.linalg.inv(Rz)))
        truth = np.array(truth_a + truth_b)
        idx = np.arange(K, dtype=np.int32)
        z = np.array(zs)
        z[WRONG] = pc.compose(z[WRONG], np.concatenate([[3.0, 0.0, 0.0], pc.rotvec_to_quat([0.0, 0.0, 0.5])]))
        cov = np.array(covs).reshape(K, 36)
        mem, _, _ = e.pcm_select(np.array(poses_a), np.array(poses_b), idx, idx, z, cov, pc.THRESHOLD, odom_var=odom_var)
        assert mem.tolist() == [k for k in range(K) if k != WRONG]
        bias = np.array([0.0, 0.0, 0.01, 0.05, 0.0, 0.0])
        odo_cov_a = np.diag([1e-4] * 3 + [2.5e-3] * 3).ravel(); tight = (1e-8 * np.eye(6)).ravel()
        f_i, f_j, f_z, f_cov = [], [], [], []
        for k in range(K - 1):
            f_i += [k, K + k]; f_j += [k + 1, K + k + 1]
            f_z += [pg.perturb(pg.between(truth[k], truth[k + 1]), bias), pg.between(truth[K + k], truth[K + k + 1])]
            f_cov += [odo_cov_a, tight]
        start = [pg.perturb(truth[0], bias)]
        for k in range(K - 1):
            nxt = pc.compose(start[-1], f_z[2 * k]); nxt[3:] /= np.linalg.norm(nxt[3:])
            start.append(nxt)
        start = np.array(start + [truth[K + k] for k in range(K)])
        prm = PgoParams.defaults(relative_cost_tolerance=1e-14, step_tolerance=1e-14, cg_tolerance=1e-12, cg_max_iterations=4000)
        g = pg.graph(start, f_i + [int(idx[m]) for m in mem], f_j + [K + int(idx[m]) for m in mem],
                     np.vstack([np.array(f_z)] + [z[m][None] for m in mem]), np.vstack([np.array(f_cov)] + [cov[m][None] for m in mem]),
                     [K], truth[K][None], tight[None])
        X, res, _ = e.pgo_optimize(*g, params=prm)
        assert res.final_cost < res.initial_cost
        # the map: pose k of the graph is robot 1's keyframe k, pose K + k robot 0's
        robots = [1] * K + [0] * K; indices = list(range(K)) * 2
        store = seen + clouds
        leaf = 0.4
        solved = gm.build(leaf, [(robots[i], indices[i], store[i], X[i]) for i in range(2 * K)])
        drifted = gm.build(leaf, [(robots[i], indices[i], store[i], start[i]) for i in range(2 * K)])
        print("occupied voxels: at poses_out", len(solved.table), "at the drifted odometry", len(drifted.table))
        assert len(solved.table) < len(drifted.table)                  # the checker shows it first
        e.map_reset(leaf)
        e.map_set_keyframes(robots, indices, start)
        same(e, drifted)
        e.map_set_keyframes(robots, indices, X)                        # the update an optimisation is followed by: robot 1 re-posed, robot 0 as it moved
        same(e, solved)
        assert e.map_stats().occupied_voxels < len(drifted.table)
    finally:
        e.close()
