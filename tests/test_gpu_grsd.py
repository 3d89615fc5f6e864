"""The GRSD plugin on the GPU against the CPU restatement (tests/grsd_checker.py): normals, voxel centroids, radii, classes, the 36
transition counters and the 21 floats bit for bit; batches, bad inputs, both detections against plugin_cases' vectorised 1-NN, a
planted revisit and the C++ adapter."""
import os
import subprocess

import numpy as np
import pytest

import grsd_cases as cs
import grsd_checker as gc
import plugin_cases as pc
from scl_slam_amd.synth import synth_scan

ROOT = os.path.dirname(os.path.abspath(__file__))


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _filtered(n_raw, seed, leaf=0.4):
    from scl_slam_amd import ScanContextEngine
    sc = ScanContextEngine()
    try:
        return np.ascontiguousarray(sc.voxel_grid(synth_scan(n_raw, seed=seed, stride_floats=4), leaf), np.float32)
    finally:
        sc.close()


def _clouds():
    """name -> (cloud, ne_radius, grsd_radius)"""
    rs = np.random.RandomState(5)
    out = {"plane": (cs.plane(), 0.5, 2.0), "sparse": (cs.sparse(), 0.5, 2.0), "lonely": (cs.lonely(), 0.5, 2.0)}
    for n in (1, 2, 3):
        out[f"n{n}"] = (synth_scan(n, seed=40 + n, stride_floats=4), 0.5, 2.0)
    out["one_voxel"] = (np.ascontiguousarray(rs.uniform(0.1, 1.9, (500, 3)), np.float32), 0.5, 2.0)
    c = synth_scan(2000, seed=9, max_range=30.0, stride_floats=8)
    c[17, :3] = (5000.0, -3.0, 2.0)
    out["outlier_5km"] = (c, 0.5, 2.0)
    out["scan_s8"] = (synth_scan(4000, seed=7, max_range=20.0, stride_floats=8), 0.5, 2.0)
    for name, v in cs.restatement_clouds().items():          # the small radii reach the cylinder and edge classes
        out[name] = v
    return out


CLOUDS = _clouds()


def _compare(e, cloud, want):
    nrm, ok = e.normals(cloud)
    assert np.array_equal(ok, want["valid"]), np.nonzero(ok != want["valid"])[0][:5].tolist()
    assert np.isnan(nrm[ok == 0]).all()
    assert np.array_equal(_u32(nrm)[ok == 1], _u32(want["normals"])[ok == 1]), np.argwhere(_u32(nrm) != _u32(want["normals"]))[:5].tolist()
    cent, rmin, rmax, cls = e.voxels(cloud)
    assert cent.shape == want["centroids"].shape and np.array_equal(_u32(cent), _u32(want["centroids"]))
    assert np.array_equal(_u32(rmin), _u32(want["r_min"])) and np.array_equal(_u32(rmax), _u32(want["r_max"]))
    assert np.array_equal(cls, want["classes"])
    assert np.array_equal(e.transitions(cloud), want["T"])
    assert np.array_equal(_u32(e.make(cloud)), _u32(want["values"]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CLOUDS))
def test_every_stage_bit_for_bit(name):
    from scl_slam_amd import GrsdEngine
    cloud, ne, R = CLOUDS[name]
    e = GrsdEngine(ne_radius=ne, grsd_radius=R)
    try:
        _compare(e, cloud, gc.stages(cloud, ne, R))
        assert e.get_size() == 0                                # make and the hooks store nothing
    finally:
        e.close()


@pytest.mark.gpu
def test_known_answers_on_device():
    from scl_slam_amd import GrsdEngine
    e = GrsdEngine()
    try:
        want = np.zeros(21, np.float32); want[6] = 168; want[10] = 332
        assert np.array_equal(e.make(cs.plane()), want)
        want[5] = 26
        assert np.array_equal(e.make(cs.lonely()), want)
        cent, rmin, rmax, cls = e.voxels(cs.sparse())
        assert (cls == 1).all() and int(e.transitions(cs.sparse()).sum()) == 26 * cls.size
    finally:
        e.close()


@pytest.mark.gpu
def test_filtered_scan_bit_for_bit():
    """the production input: a synthetic scan through the 0.4 m voxel filter, every point and voxel against the brute force"""
    from scl_slam_amd import GrsdEngine
    cloud = _filtered(30000, seed=3)
    e = GrsdEngine()
    try:
        want = gc.stages(cloud)
        _compare(e, cloud, want)
        print(f"filtered scan: {cloud.shape[0]} points, {want['classes'].size} voxels, {int(want['valid'].sum())} valid normals")
    finally:
        e.close()


@pytest.mark.gpu
def test_raw_scan_sampled():
    """a raw 120 000-point scan: the brute force is quadratic, so 3 000 sampled points' normals and 400 sampled voxels' radii and
    classes are checked (the first and last of each among them); centroids, counters and values in full -- the checker's
    transition stage is fed the device's normals and classes, which the samples vouch for"""
    from scl_slam_amd import GrsdEngine
    cloud = synth_scan(120000, seed=3, stride_floats=4)
    n = cloud.shape[0]
    e = GrsdEngine()
    try:
        rs = np.random.RandomState(1)
        q = np.sort(rs.choice(n, 3000, replace=False)).astype(np.int32); q[0] = 0; q[-1] = n - 1
        nrm, ok = e.normals(cloud)
        wn, wok = gc.normals(cloud, queries=q)
        assert np.array_equal(ok[q], wok)
        assert np.array_equal(_u32(nrm[q])[wok == 1], _u32(wn)[wok == 1])
        cent, rmin, rmax, cls = e.voxels(cloud)
        wc, vidx, grid = gc.voxels(cloud)
        assert np.array_equal(_u32(cent), _u32(wc))
        nv = wc.shape[0]
        vq = np.sort(rs.choice(nv, min(400, nv), replace=False)).astype(np.int32); vq[0] = 0; vq[-1] = nv - 1
        wmin, wmax, wcls = gc.rsd(cloud, nrm, ok, wc, queries=vq)
        assert np.array_equal(_u32(rmin[vq]), _u32(wmin)) and np.array_equal(_u32(rmax[vq]), _u32(wmax)) and np.array_equal(cls[vq], wcls)
        T = gc.transitions(wc, vidx, cls, grid)
        assert np.array_equal(e.transitions(cloud), T)
        assert np.array_equal(_u32(e.make(cloud)), _u32(gc.histogram(T)))
        print(f"raw scan: {n} points, {nv} voxels, classes {np.bincount(cls, minlength=5).tolist()}")
    finally:
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 7, 16, 37])
def test_batches_equal_single_calls(count):
    from scl_slam_amd import GrsdEngine
    rs = np.random.RandomState(count)
    clouds = [synth_scan(int(rs.randint(1, 4000)) if i % 5 else 1 + i, seed=500 + i, max_range=25.0, stride_floats=4) for i in range(count)]
    a, b = GrsdEngine(), GrsdEngine()
    try:
        got = a.make_and_save_many(clouds, indexs=np.arange(count))
        for i, c in enumerate(clouds):
            one = b.make_and_save(c, 0, i)
            assert np.array_equal(_u32(got[i]), _u32(one)), i
            assert np.array_equal(_u32(a.get_signature(i)), _u32(one))
        assert a.get_size() == count
    finally:
        a.close(); b.close()


@pytest.mark.gpu
def test_bad_inputs_leave_database_unchanged():
    from scl_slam_amd import GrsdEngine, GrsdError
    e = GrsdEngine()
    try:
        good = synth_scan(500, seed=1, max_range=20.0, stride_floats=4)
        e.make_and_save(good, 0, 0)
        before = e.get_signature(0)
        nan = good.copy(); nan[100, 1] = np.nan
        inf = good.copy(); inf[499, 2] = np.inf
        wide = good.copy(); wide[3, :3] = (3.0e9, 3.0e9, 3.0e9)          # 1.5e9 cells per axis: the voxel index overflows int32
        for bad in (good[:0], nan, inf, wide):
            with pytest.raises(GrsdError) as ei:
                e.make_and_save(bad, 0, 1)
            assert ei.value.status == -1                               # SCL_ERR_INVALID_ARG
        for where in (0, 20, 23):
            batch = [good] * 24; batch[where] = nan
            with pytest.raises(GrsdError):
                e.make_and_save_many(batch)
        with pytest.raises(GrsdError):
            e.make_and_save_many([good] * 17 + [wide])
        with pytest.raises(GrsdError):
            e.make(nan)
        with pytest.raises(GrsdError):
            e.make_and_save(good, 1, 0)                                # robot id outside [0, robot_num)
        assert e.get_size() == 1 and np.array_equal(_u32(e.get_signature(0)), _u32(before))
        assert np.array_equal(_u32(e.make_and_save(good, 0, 1)), _u32(before)) and e.get_size() == 2
    finally:
        e.close()


def grsd_rows(n, seed, nonfinite=False):
    """n rows of 21 floats shaped like descriptors: integer counts, mostly in the plane / empty bins; 15 % exact copies of row 0
    (ties); optionally a few rows holding NaN or inf"""
    rs = np.random.RandomState(seed)
    rows = np.zeros((n, 21), np.float32)
    rows[:, 6] = 2 * rs.poisson(900, n); rows[:, 10] = rs.poisson(1200, n); rows[:, 5] = 26 * rs.poisson(3, n)
    rows[:, [7, 9, 11, 14]] = rs.poisson(40, (n, 4))
    rows[rs.rand(n) < 0.15] = rows[0]
    if nonfinite:
        rows[rs.choice(n, 6, replace=False), rs.randint(0, 21, 6)] = [np.nan, np.inf, -np.inf, np.nan, np.inf, np.nan]
        rows[n - 1, 20] = np.nan                                   # a query row with a NaN: nothing is found
    return rows


def _checker(**kw):
    """plugin_cases' vectorised 1-NN checker: over rows of 21 floats its reported distance (the first report_dims = 21 floats) is the
    1-NN's own"""
    kw = dict(kw); kw.pop("ne_radius", None); kw.pop("grsd_radius", None)
    return pc.FpfhChecker(report_dims=21, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("robots", [2, 3])
@pytest.mark.parametrize("inter_mode", [0, 1])
@pytest.mark.parametrize("nonfinite", [False, True])
def test_detections_against_checker(robots, inter_mode, nonfinite):
    from scl_slam_amd import GrsdEngine
    n = 110
    rows = grsd_rows(n, 60 + robots + inter_mode, nonfinite)
    kw = dict(dist_thres=160.0, num_exclude_recent=8, tree_making_period=4, inter_mode=inter_mode, robot_num=robots, this_id=1)
    e = GrsdEngine(**kw); c = _checker(**kw)
    owner = np.random.RandomState(robots).randint(0, robots, n)
    counts = [0] * robots
    loops = 0
    try:
        for i in range(n):
            r = int(owner[i])
            e.save_from_wire(rows[i], r, counts[r]); c.save(rows[i], r, counts[r]); counts[r] += 1
            snap_before = c.snap_n
            g = e.detect_inter(i); w = c.detect_inter(i)
            assert pc.same_detection(g, w, nan_ok=True), (i, g, w)
            loops += g[0] >= 0
            if inter_mode == 0:
                if i + 1 < kw["num_exclude_recent"] + 1:
                    assert g == (-1, np.float32(0.0))                # the early return: nothing before 9 keyframes
                elif (c.counter - 1) % kw["tree_making_period"]:
                    assert c.snap_n == snap_before                   # between rebuilds the snapshot is stale
            if r == 1:
                cur = counts[1] - 1
                g = e.detect_intra(cur); w = c.detect_intra(cur)
                assert pc.same_detection(g, w, nan_ok=True), (i, cur, g, w)
        if inter_mode == 0:
            assert c.counter >= 2 * kw["tree_making_period"]         # at least two rebuilds crossed
        assert loops > 0
    finally:
        e.close()


@pytest.mark.gpu
def test_reference_early_return_and_ties():
    """the defaults: nothing before 31 keyframes (result (-1, 0)); equal rows: the lowest key wins"""
    from scl_slam_amd import GrsdEngine
    e = GrsdEngine()
    try:
        rows = grsd_rows(45, 3)
        rows[2, 7] = 12345.0                                       # a row no other equals, then two copies of it
        rows[5] = rows[2]; rows[40] = rows[2]
        for i in range(45):
            e.save_from_wire(rows[i], 0, i)
            loop, d = e.detect_inter(i)
            if i < 30:
                assert (loop, float(d)) == (-1, 0.0), i
        # this robot's keyframes [0, 10): rows 2 and 5 tie at distance 0
        assert e.detect_intra(40) == (2, np.float32(0.0))
    finally:
        e.close()
    e = GrsdEngine(num_exclude_recent=1, tree_making_period=1)
    try:
        for i in range(45):
            e.save_from_wire(rows[i], 0, i)
        assert e.detect_inter(40) == (2, np.float32(0.0))
    finally:
        e.close()


@pytest.mark.gpu
def test_planted_revisit_found_by_intra():
    from scl_slam_amd import GrsdEngine
    e = GrsdEngine(num_exclude_recent=30)
    try:
        clouds = [synth_scan(3000, seed=900 + i, max_range=30.0, stride_floats=4) for i in range(40)]
        e.make_and_save_many(clouds, indexs=np.arange(40))
        e.make_and_save(clouds[4].copy(), 0, 40)
        loop, d = e.detect_intra(40)
        assert (loop, float(d)) == (4, 0.0), (loop, d)
    finally:
        e.close()


@pytest.mark.gpu
def test_adapter_agrees_with_c_calls():
    exe = os.path.join(ROOT, "cpp", "grsd_adapter_check")
    assert os.path.exists(exe), "build it with `make`"
    r = subprocess.run([exe, "40"], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout + r.stderr
