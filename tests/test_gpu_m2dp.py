"""The M2DP plugin on the GPU against the CPU restatement (tests/m2dp_checker.py): counts bit for bit, frame, signature,
batches, bad inputs, detections, a planted revisit and the C++ adapter."""
import math
import os
import subprocess

import numpy as np
import pytest

import m2dp_checker as mc
from scl_slam_amd.synth import synth_scan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng():
    from scl_slam_amd import M2dpEngine
    e = M2dpEngine()
    yield e
    e.close()


def _check_counts(eng, cloud):
    counts, mean, axes, mr = eng.signature_matrix(cloud)
    want, mr_c = mc.signature_matrix(cloud, (mean, axes))
    assert np.float32(mr_c) == mr
    diff = np.argwhere(counts != want)
    assert diff.size == 0, f"{len(diff)} bins differ, first {diff[:5].tolist()}"
    assert int(counts.sum(axis=1).max()) <= cloud.shape[0]
    return counts, mean, axes


@pytest.mark.gpu
@pytest.mark.parametrize("n", [3, 1000, 12000, 120000, 240000])
@pytest.mark.parametrize("stride_floats", [4, 8])
def test_counts_bit_for_bit(eng, n, stride_floats):
    cloud = synth_scan(n, seed=100 + n % 97, stride_floats=stride_floats)
    _check_counts(eng, cloud)


def _edge_cloud(seed=3):
    """A mirror-symmetric cloud (every point with all 8 sign patterns) on a 2^-10 grid: every fp64 sum of the frame is exact,
    the mean is 0, the covariance diagonal with var x > var y > var z, so the GPU's frame is the identity (up to signs, which map
    the cloud onto itself) and cloudPca = (x, y, -z).  In the elevation-0 planes (rows 0, 16, 32, 48) pcy = (-z) * py2 and in
    plane 0 pcx = x + y * 6e-17: points with z or x at 0 or +-1e-30 put theta within a few ulps of the edges 0, +-pi/2 and
    +-pi, and x = k^2 with y = z = 0 puts rho on the edge rhoList[k] exactly (maxRho = 64 from the points (0, 0, +-64))."""
    rs = np.random.RandomState(seed)
    q = lambda a: np.round(a * 1024.0) / 1024.0
    base = np.stack([q(rs.uniform(0, 30, 2000)), q(rs.uniform(0, 20, 2000)), q(rs.uniform(0, 8, 2000))], axis=1)
    special = [(0.0, 0.0, 64.0)]
    for v in (0.0, 1e-30, 3e-38, 1e-20):
        for w in (1.0, 7.5, 25.0):
            special += [(w, rs.uniform(0, 20), v), (v, rs.uniform(0, 20), w), (v, w, v), (w, v, v)]
    for k in range(1, 6):
        special.append((float(k * k), 0.0, 0.0))
    pts = np.concatenate([base, np.array(special)])
    signs = np.array([[sx, sy, sz] for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)], np.float64)
    cloud = (pts[None, :, :] * signs[:, None, :]).reshape(-1, 3)
    return cloud.astype(np.float32)


@pytest.mark.gpu
def test_edge_cloud_bit_for_bit_and_exact_path(eng):
    cloud = _edge_cloud()
    d0, e0, _ = eng.stats()
    counts, mean, axes = _check_counts(eng, cloud)
    d1, e1, _ = eng.stats()
    assert np.array_equal(np.abs(axes), np.eye(3, dtype=np.float32)), axes
    assert np.float32(eng.signature_matrix(cloud)[3]) == np.float32(64.0)
    _, _, near = mc.signature_matrix(cloud, (mean, axes), return_near=True)
    print(f"edge cloud: {cloud.shape[0]} points, {d1 - d0} decisions, {e1 - e0} took the exact path on the GPU, "
          f"{near} within 1e-9 of an edge in the checker")
    assert d1 - d0 == 64 * cloud.shape[0] and e1 - e0 >= 100


@pytest.mark.gpu
def test_frame_matches_numpy(eng):
    for seed in (1, 2, 3):
        cloud = synth_scan(20000, seed=seed)
        _, mean, axes, _ = eng.signature_matrix(cloud)
        m_c, a_c = mc.frame(cloud)
        assert np.max(np.abs(mean - m_c)) <= 1e-6 * max(1.0, float(np.max(np.abs(m_c))))
        assert np.max(np.abs(axes.astype(np.float64) - a_c.astype(np.float64))) <= 1e-6


@pytest.mark.gpu
def test_signature_matches_svd(eng):
    checked = 0
    for seed, n in ((4, 5000), (5, 30000), (6, 120000), (7, 777)):
        cloud = synth_scan(n, seed=seed)
        counts, mean, axes, _ = eng.signature_matrix(cloud)
        if mc.sigma_ratio(counts) > 0.999:
            continue
        want = mc.signature_from_counts(counts, n)
        got = eng.make(cloud)
        assert np.max(np.abs(got.astype(np.float64) - want)) <= 1e-6
        assert np.all(got >= 0.0)
        checked += 1
    assert checked >= 3


@pytest.mark.gpu
def test_batches_equal_scan_by_scan_and_repeat(eng):
    from scl_slam_amd import M2dpEngine
    rs = np.random.RandomState(8)
    clouds = [synth_scan(int(rs.randint(3, 9000)), seed=200 + i) for i in range(40)]
    singles = np.stack([eng.make(c) for c in clouds])
    b = M2dpEngine()
    start = 0
    for size in (1, 7, 16, 16):                               # ragged: 1, 7, 16 (one group), 16 -> 40 scans
        out = b.make_and_save_many(clouds[start:start + size], robots=[0] * size, indexs=list(range(start, start + size)))
        assert np.array_equal(out.view(np.uint32), singles[start:start + size].view(np.uint32))
        start += size
    assert b.get_size() == 40
    b2 = M2dpEngine()
    out = b2.make_and_save_many(clouds)                       # 40 in one call: groups of 16, 16, 8
    assert np.array_equal(out.view(np.uint32), singles.view(np.uint32))
    for k in (0, 17, 39):
        assert np.array_equal(b2.get_signature(k).view(np.uint32), singles[k].view(np.uint32))
    again = eng.make(clouds[5])
    assert np.array_equal(again.view(np.uint32), singles[5].view(np.uint32))
    b.close(); b2.close()


@pytest.mark.gpu
def test_bad_inputs_are_rejected_and_the_database_is_unchanged():
    from scl_slam_amd import M2dpEngine, M2dpError
    e = M2dpEngine()
    good = synth_scan(500, seed=1)
    e.make_and_save(good)
    for bad in (good[:2], np.where(np.arange(500)[:, None] == 77, np.float32(np.nan), good),
                np.where(np.arange(500)[:, None] == 3, np.float32(np.inf), good)):
        with pytest.raises(M2dpError) as ei:
            e.make_and_save(np.ascontiguousarray(bad, np.float32))
        assert ei.value.status == -1
        with pytest.raises(M2dpError):
            e.make_and_save_many([good, np.ascontiguousarray(bad, np.float32)])
        assert e.get_size() == 1
    with pytest.raises(M2dpError):
        e.make_and_save_many([good] * 20 + [np.ascontiguousarray(good[:2])])
    assert e.get_size() == 1
    e.close()


def _wire_scenario(robot_num, this_id, n_per_robot, seed, excl):
    from scl_slam_amd import M2dpEngine
    rs = np.random.RandomState(seed)
    e = M2dpEngine(robot_num=robot_num, this_id=this_id, num_exclude_recent=excl, dist_thres=0.3)
    c = mc.CheckerDB(robot_num=robot_num, this_id=this_id, num_exclude_recent=excl, dist_thres=0.3)
    protos = np.abs(rs.standard_normal((6, 192))).astype(np.float32) * 0.1
    for k in range(n_per_robot * robot_num):
        r = k % robot_num
        v = protos[rs.randint(6)] + (rs.standard_normal(192).astype(np.float32) * 0.01 if rs.rand() < 0.6 else 0.0)
        v = np.asarray(v, np.float32)
        if rs.rand() < 0.15:                                  # exact duplicates: ties, the lowest key must win
            v = protos[0].copy()
        e.save_from_wire(v, r, k); c.save(v, r, k)
    return e, c


@pytest.mark.gpu
@pytest.mark.parametrize("robot_num,this_id", [(2, 0), (3, 1)])
def test_detection_bit_for_bit(robot_num, this_id):
    e, c = _wire_scenario(robot_num, this_id, 60, seed=robot_num, excl=5)
    n_mine = e.get_size(this_id)
    loops = 0
    for cur in range(n_mine):                                 # includes the exclusion window's edges: cur <= 5 has no history
        g = e.detect_intra(cur); o = c.detect_intra(cur)
        assert g[0] == o[0] and np.float32(g[1]).view(np.uint32) == np.float32(o[1]).view(np.uint32), (cur, g, o)
        loops += g[0] >= 0
    for key in range(e.get_size()):
        g = e.detect_inter(key); o = c.detect_inter(key)
        assert g[0] == o[0] and np.float32(g[1]).view(np.uint32) == np.float32(o[1]).view(np.uint32), (key, g, o)
    assert loops > 0
    e.close()


@pytest.mark.gpu
def test_planted_revisit_is_found():
    from scl_slam_amd import M2dpEngine
    e = M2dpEngine(num_exclude_recent=30)
    clouds = [synth_scan(20000, seed=500 + i) for i in range(40)]
    e.make_and_save_many(clouds, want_values=False)
    rs = np.random.RandomState(9)
    a = math.radians(40.0)
    R = np.array([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]])
    src = clouds[3][:, :3].astype(np.float64)
    again = src @ R.T + np.array([0.3, 0.0, 0.0]) + 0.01 * rs.standard_normal(src.shape)
    revisit = np.zeros_like(clouds[3]); revisit[:, :3] = again
    e.make_and_save(revisit, 0, 40)
    loop, dist = e.detect_intra(40)
    print(f"planted revisit: loop {loop}, distance {dist}")
    assert loop == 3 and dist < 0.3
    e.close()


@pytest.mark.gpu
def test_cpp_adapter_agrees_with_the_c_calls():
    binp = os.path.join(ROOT, "tests", "cpp", "m2dp_adapter_check")
    assert os.path.exists(binp), "build first (make / __graft_entry__.build())"
    out = subprocess.run([binp, "48"], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "ALL OK" in out.stdout
