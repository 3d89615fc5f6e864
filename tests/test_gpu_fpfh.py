"""The FPFH plugin on the GPU against the CPU restatement (tests/fpfh_checker.py): neighbours, normals, counts and values bit for
bit, the device acosf, batches, bad inputs, both detections, the nanoflann golden, a planted revisit and the C++ adapter."""
import json
import os
import subprocess

import numpy as np
import pytest

import fpfh_checker as fc
from golden.gen_fpfh_nn_golden import golden_keys, golden_queries
from scl_slam_amd.synth import synth_scan

ROOT = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(ROOT)


@pytest.fixture(scope="module")
def eng():
    from scl_slam_amd import FpfhEngine
    e = FpfhEngine()
    yield e
    e.close()


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _clouds():
    """name -> (n, 3 | 4 | 8) float32 cloud"""
    rs = np.random.RandomState(5)
    out = {}
    for n in (3, 9, 10, 11, 1000, 20000):
        out[f"scan{n}"] = synth_scan(n, seed=40 + n % 31, stride_floats=4)
    out["scan1000_s8"] = synth_scan(1000, seed=7, stride_floats=8)
    base = rs.uniform(-20, 20, (300, 3)).astype(np.float32)
    out["duplicates"] = np.concatenate([base, base[:120], base[:40]])
    out["same"] = np.tile(np.array([[1.5, -2.0, 0.25]], np.float32), (50, 1))
    t = rs.uniform(0, 50, 400).astype(np.float32)
    out["line"] = np.stack([t, 0.5 * t + 1.0, np.full_like(t, -1.0)], axis=1).astype(np.float32)
    uv = rs.uniform(-30, 30, (2000, 2)).astype(np.float32)
    out["plane"] = np.stack([uv[:, 0], uv[:, 1], 0.1 * uv[:, 0] - 2.0], axis=1).astype(np.float32)
    c = synth_scan(1000, seed=9, stride_floats=4)
    c[17, :3] = (1.0e5, -3.0, 2.0)
    out["outlier"] = c
    a = rs.normal(0, 1.0, (600, 3)).astype(np.float32)
    b = (rs.normal(0, 1.0, (600, 3)) + np.array([5.0e4, -4.0e4, 10.0])).astype(np.float32)
    out["two_clusters"] = np.concatenate([a, b])
    return out


CLOUDS = _clouds()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CLOUDS))
def test_neighbors_normals_counts_bit_for_bit(eng, name):
    cloud = CLOUDS[name]
    idx, d2 = eng.neighbors(cloud)
    ci, cd = fc.knn(cloud)
    assert np.array_equal(idx, ci), f"{np.argwhere(idx != ci)[:5].tolist()}"
    assert np.array_equal(_u32(d2), _u32(cd))
    nrm = eng.normals(cloud)
    cn = fc.normals(cloud)
    assert np.array_equal(_u32(nrm), _u32(cn)), f"{np.argwhere(_u32(nrm) != _u32(cn))[:5].tolist()}"
    counts, skipped = eng.counts(cloud)
    cc, cs = fc.spfh_counts(cloud, cn)
    assert np.array_equal(counts, cc) and skipped == cs, (counts.tolist(), cc.tolist(), skipped, cs)
    n = cloud.shape[0]
    for f in range(3):
        assert int(counts[11 * f:11 * f + 11].sum()) + skipped == n - 1
    v = eng.make(cloud)
    want, _, _ = fc.describe(cloud)
    assert np.array_equal(_u32(v), _u32(want))


@pytest.mark.gpu
def test_filtered_scan_sampled_queries(eng):
    """~96 k points: a 120 k synthetic scan through the 0.4 m voxel filter; 2 000 sampled queries against the brute force"""
    from scl_slam_amd import ScanContextEngine
    raw = synth_scan(120000, seed=3, stride_floats=4)
    sc = ScanContextEngine()
    cloud = np.ascontiguousarray(sc.voxel_grid(raw, 0.4), np.float32)
    sc.close()
    n = cloud.shape[0]
    q = np.random.RandomState(1).choice(n, 2000, replace=False).astype(np.int32)
    q[-1] = n - 1
    idx, d2 = eng.neighbors(cloud)
    ci, cd = fc.knn(cloud, q)
    assert np.array_equal(idx[q], ci) and np.array_equal(_u32(d2[q]), _u32(cd))
    nrm = eng.normals(cloud)
    assert np.array_equal(_u32(nrm[q]), _u32(fc.normals(cloud, q)))
    counts, skipped = eng.counts(cloud)
    cc, cs = fc.spfh_counts(cloud, nrm)
    assert np.array_equal(counts, cc) and skipped == cs
    p0, cand0, _ = eng.stats()
    print(f"filtered scan: {n} points, {cand0} candidate distances so far")


@pytest.mark.gpu
def test_device_acosf_blocks(eng):
    gold = json.load(open(os.path.join(ROOT, "golden", "acosf_blocks.json")))
    assert gold["differences_vs_libm"] == 0
    got = np.concatenate([eng.acosf_blocks(b, 64) for b in range(0, 256, 64)])
    want = np.array([int(h, 16) for h in gold["blocks"]], np.uint64)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"blocks {bad[:8].tolist()} differ"


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 7, 16, 37])
def test_batches_equal_single_calls(count):
    from scl_slam_amd import FpfhEngine
    rs = np.random.RandomState(count)
    clouds = [synth_scan(int(rs.randint(3, 4000)) if i % 5 else 3 + i, seed=500 + i, stride_floats=4) for i in range(count)]
    a, b = FpfhEngine(), FpfhEngine()
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
    from scl_slam_amd import FpfhEngine, FpfhError
    e = FpfhEngine()
    try:
        good = synth_scan(500, seed=1, stride_floats=4)
        e.make_and_save(good, 0, 0)
        before = e.get_signature(0)
        nan = good.copy(); nan[100, 1] = np.nan
        inf = good.copy(); inf[499, 2] = np.inf
        for bad in (good[:2], nan, inf):
            with pytest.raises(FpfhError) as ei:
                e.make_and_save(bad, 0, 1)
            assert ei.value.status != 0
        with pytest.raises(FpfhError):
            e.make_and_save_many([good] * 20 + [nan] + [good] * 3)
        with pytest.raises(FpfhError):
            e.make(nan)
        assert e.get_size() == 1 and np.array_equal(_u32(e.get_signature(0)), _u32(before))
    finally:
        e.close()


def _signatures(n, seed, ties=False):
    rs = np.random.RandomState(seed)
    keys = golden_keys(n, seed, "hist")
    if ties:
        keys[rs.randint(0, n, n // 4)] = keys[rs.randint(0, n, n // 4)]
        keys[5] = keys[2]
    return keys


@pytest.mark.gpu
@pytest.mark.parametrize("robots", [2, 3])
@pytest.mark.parametrize("inter_mode", [0, 1])
@pytest.mark.parametrize("report_dims", [21, 33])
def test_detections_against_checker(robots, inter_mode, report_dims):
    from scl_slam_amd import FpfhEngine
    n = 110
    keys = _signatures(n, 60 + robots + inter_mode, ties=True)
    kw = dict(dist_thres=40.0, num_exclude_recent=8, tree_making_period=4, report_dims=report_dims, inter_mode=inter_mode,
              robot_num=robots, this_id=1)
    e = FpfhEngine(**kw); c = fc.FpfhChecker(**kw)
    owner = np.random.RandomState(robots).randint(0, robots, n)
    counts = [0] * robots
    try:
        for i in range(n):
            r = int(owner[i])
            e.save_from_wire(keys[i], r, counts[r]); c.save(keys[i], r, counts[r]); counts[r] += 1
            g = e.detect_inter(i); w = c.detect_inter(i)
            assert g[0] == w[0] and _u32(g[1]) == _u32(w[1]), (i, g, w)
            if r == 1:
                cur = counts[1] - 1
                g = e.detect_intra(cur); w = c.detect_intra(cur)
                assert g[0] == w[0] and _u32(g[1]) == _u32(w[1]), (i, cur, g, w)
        if inter_mode == 0:
            assert c.counter >= 2 * kw["tree_making_period"]   # at least two rebuilds crossed
    finally:
        e.close()


@pytest.mark.gpu
def test_golden_winners_on_device():
    """the keys through save_from_wire, the query as the last key, num_exclude_recent = 1: the snapshot is the keys alone"""
    from scl_slam_amd import FpfhEngine
    gold = json.load(open(os.path.join(ROOT, "golden", "fpfh_nn_golden.json")))
    for name, case in gold["cases"].items():
        keys = golden_keys(case["N"], case["seed"], case["kind"])
        queries = golden_queries(keys, case["seed"], case["nq"], case["kind"])
        for q, want in zip(queries, case["results"]):
            e = FpfhEngine(num_exclude_recent=1, tree_making_period=1, report_dims=33, dist_thres=1e30)
            try:
                for k in keys:
                    e.save_from_wire(k)
                e.save_from_wire(q)
                loop, d = e.detect_inter(len(keys))
                assert loop == want["idx"], (name, loop, want)
            finally:
                e.close()


@pytest.mark.gpu
def test_planted_revisit_found_by_intra():
    from scl_slam_amd import FpfhEngine
    rs = np.random.RandomState(8)
    e = FpfhEngine(num_exclude_recent=30)
    try:
        clouds = [synth_scan(3000, seed=900 + i, stride_floats=4) for i in range(40)]
        e.make_and_save_many(clouds, indexs=np.arange(40))
        again = clouds[4].copy()
        again[:, :3] += (rs.standard_normal(again[:, :3].shape) * 1e-3).astype(np.float32)
        e.make_and_save(again, 0, 40)
        loop, d = e.detect_intra(40)
        assert loop == 4, (loop, d)
    finally:
        e.close()


@pytest.mark.gpu
def test_adapter_agrees_with_c_calls():
    exe = os.path.join(ROOT, "cpp", "fpfh_adapter_check")
    assert os.path.exists(exe), "build it with `make`"
    r = subprocess.run([exe, "40"], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout + r.stderr
