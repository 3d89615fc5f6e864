"""The voxel filter and the submap assembly (csrc/voxel.hip), single and batched, against the CPU checker at their edges.
Bar: bit-for-bit equality with icpo_voxel_grid (oracle/icp_oracle.c) on every cloud of tests/voxel_cases.py -- which
tests/test_voxel_cases.py pins by hand-written answers and a numpy restatement -- through every entry point that reaches the
filter; the batched form (assemble_submaps_batch, the path of scl_loop_icp_batch_from_store) through scl_selftest_submaps_batch.
Where the checker returns None (the voxel index leaves int32) the input comes back, in bits."""
import numpy as np
import pytest

import oracle_icp_binding as oi
import voxel_cases as vc
from scl_slam_amd import ScanContextEngine, SclError
from scl_slam_amd.synth import rigid_transform, synth_structured_cloud
from test_oracle_icp_kat import moved_copy

pytestmark = pytest.mark.gpu
IDENT = np.eye(4, dtype=np.float32)
_want = {}


def want(name):
    """the checker's answer for a case, computed once: (filtered cloud, or the input itself where the checker says None)"""
    if name not in _want:
        c, leaf = vc.cases()[name]
        o = oi.voxel_grid(c, leaf)
        _want[name] = c if o is None else o
    return _want[name]


def bits_equal(got, wanted):
    """view(np.uint32) equality; where the checker's value is a NaN (an averaged NaN intensity) any NaN will do"""
    return vc.same_bits(got, wanted)


@pytest.fixture(scope="module")
def eng():
    e = ScanContextEngine()
    yield e
    e.close()


@pytest.mark.parametrize("name", vc.names())
def test_voxel_grid_cases(eng, name):
    c, leaf = vc.cases()[name]
    assert bits_equal(eng.voxel_grid(c, leaf), want(name))


@pytest.mark.parametrize("name", vc.names())
def test_assemble_submap_cases(eng, name):
    """one keyframe, identity pose: the checker's transform (which turns -0.0 into +0.0 and a point with an infinite coordinate into
    NaNs) and then its filter"""
    c, leaf = vc.cases()[name]
    moved = oi.transform(c, IDENT)
    o = oi.voxel_grid(moved, leaf)
    assert (o is None) == (name in ("index_2_31", "index_inf_inv"))
    assert bits_equal(eng.assemble_submap([c], [IDENT], leaf), moved if o is None else o)


@pytest.mark.parametrize("stride", vc.STRIDES)
def test_submap_from_store_cases(stride):
    """the same through the keyframe store; an engine per stride, as the store keeps the stride of its first cloud"""
    mine = [n for n in vc.names() if vc.cases()[n][0].shape[1] * 4 == stride]
    assert mine
    with ScanContextEngine() as e:
        for k, name in enumerate(mine):
            e.keyframe_put(0, k, vc.cases()[name][0])
        for k, name in enumerate(mine):
            c, leaf = vc.cases()[name]
            moved = oi.transform(c, IDENT)
            o = oi.voxel_grid(moved, leaf)
            g = e.submap_from_store(0, k, 0, [IDENT], leaf, c.shape[0], floats_per_point=stride // 4)
            assert bits_equal(g, moved if o is None else o), name


def test_make_and_save_filtered_cases():
    """filter + descriptor in one call == scl_voxel_grid, then scl_make_and_save on a second engine: count, wire values, keys"""
    mine = vc.names(("boundaries", "nonfinite", "index"))
    assert len(mine) == 12
    with ScanContextEngine() as e1, ScanContextEngine() as e2:
        for k, name in enumerate(mine):
            c, leaf = vc.cases()[name]
            f = e1.voxel_grid(c, leaf)
            assert bits_equal(f, want(name)), name
            v1 = e1.make_and_save(f, 0, k)
            v2, m = e2.make_and_save_filtered(c, leaf, 0, k)
            assert m == f.shape[0] == want(name).shape[0], name
            assert np.array_equal(v1.view(np.uint32), v2.view(np.uint32)), name
            assert np.array_equal(e1.get_ringkey(k).view(np.uint32), e2.get_ringkey(k).view(np.uint32)), name
            assert np.array_equal(e1.get_sectorkey(k).view(np.uint64), e2.get_sectorkey(k).view(np.uint64)), name
            assert np.array_equal(e1.get_descriptor(k).view(np.uint32), e2.get_descriptor(k).view(np.uint32)), name


def test_workspace_reuse(eng):
    """large, tiny, unfiltered (the result is then the INPUT buffer), ordinary, empty, ordinary again on one workspace: every result
    is the checker's, and the same calls in the opposite order on a fresh engine give the same"""
    seq = ["size_70000", "size_1", "index_2_31", "order", None, "order"]

    def run(e, name):
        if name is None:
            g = e.voxel_grid(np.zeros((0, 8), np.float32), 0.4)
            assert g.shape == (0, 8)
            return g
        g = e.voxel_grid(*vc.cases()[name])
        assert bits_equal(g, want(name)), name
        return g
    first = [run(eng, n) for n in seq]
    with ScanContextEngine() as fresh:
        second = [run(fresh, n) for n in seq[::-1]][::-1]
    for a, b in zip(first, second):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- the batched form ----------------------------------------------------------------------------------------------------------------

LEAF_B = 1.0          # one leaf per call: the 2^31 cloud and the order case are built for leaf 1
BEYOND = 25           # a key whose window (search_num 1) lies behind the store's 20 keyframes


@pytest.fixture(scope="module")
def store():
    """20 keyframes of 32 bytes per point built from the cases.  Poses with small rotations, except for the clouds that are made of
    exact coordinates (index range, order), which keep the identity."""
    cs = vc.cases()
    clouds = [vc._random_cloud(3000, 900)]                                             # 0
    clouds += [vc._random_cloud(10000, 901 + k, extent=(9.0, 9.0, 3.0)) for k in range(7)]   # 1 .. 7: 70 000 points
    clouds += [cs["nonfinite_all"][0], cs["index_2_31"][0], cs["size_1"][0], cs["order"][0], cs["nonfinite_mixed"][0]]   # 8 .. 12
    clouds += [cs[f"boundaries_{leaf}"][0] for leaf in (0.25, 0.5, 0.1)]              # 13 .. 15
    clouds += [cs["nonfinite_fields"][0], cs["subnormal"][0], vc._random_cloud(1500, 910), vc._random_cloud(777, 911)]   # 16 .. 19
    assert len(clouds) == 20 and all(c.shape[1] == 8 for c in clouds)
    e = ScanContextEngine()
    rs = np.random.RandomState(21)
    poses = []
    for k, c in enumerate(clouds):
        exact = k in (9, 11)
        poses.append(IDENT.copy() if exact else e.pose_to_matrix(*(rs.uniform(-1, 1, 3) * [2, 2, 0.2]), *rs.uniform(-0.03, 0.03, 3)))
        e.keyframe_put(0, k, c)
    yield e, clouds, poses, {}
    e.close()


JOBS = [(0, 0), (BEYOND, 1), (8, 0), (9, 0), (4, 3), (10, 0), (11, 0), (0, 0), (12, 0),
        (10, 12), (1, 3), (18, 2)]     # ... then a window that runs off both ends of the store, one off its front, one off its back


def _window(poses, key, sn):
    return [poses[k] if 0 <= k < len(poses) else IDENT for k in range(key - sn, key + sn + 1)]


def _wanted_submap(store, key, sn):
    """oi.transform per keyframe, np.concatenate, oi.voxel_grid; the concatenation itself where the checker says None"""
    e, clouds, poses, cache = store
    if (key, sn) not in cache:
        ks = [k for k in range(key - sn, key + sn + 1) if 0 <= k < len(clouds)]
        merged = np.concatenate([oi.transform(clouds[k], poses[k]) for k in ks]) if ks else np.zeros((0, 8), np.float32)
        o = oi.voxel_grid(merged, LEAF_B) if ks else merged
        cache[(key, sn)] = (merged if o is None else o, o is None)
    return cache[(key, sn)]


def _check_batch(store, jobs, also_one_by_one=True):
    e, clouds, poses, _ = store
    got = e.selftest_submaps_batch(0, [k for k, _ in jobs], [sn for _, sn in jobs], [_window(poses, k, sn) for k, sn in jobs], LEAF_B)
    assert len(got) == len(jobs)
    for j, (key, sn) in enumerate(jobs):
        w, _ = _wanted_submap(store, key, sn)
        assert bits_equal(got[j], w), (j, key, sn, got[j].shape, w.shape)
    if also_one_by_one:
        cap = sum(c.shape[0] for c in clouds)
        for j, (key, sn) in enumerate(jobs):
            one = e.submap_from_store(0, key, sn, _window(poses, key, sn), LEAF_B, cap)
            assert one.shape == got[j].shape and np.array_equal(one.view(np.uint32), got[j].view(np.uint32)), (j, key, sn)
    return got


def test_batch_jobs_are_what_they_claim(store):
    """(CPU side of the batch tests) the empty, the all-non-finite, the unfiltered and the 70 000-point job are those"""
    e, clouds, poses, _ = store
    sizes = [_wanted_submap(store, k, sn)[0].shape[0] for k, sn in JOBS]
    raw = [_wanted_submap(store, k, sn)[1] for k, sn in JOBS]
    assert sizes[1] == 0 and sizes[2] == 0 and sizes[5] == 1 and sizes[3] == 5 and raw[3] and raw[9] and sum(raw) == 2
    assert sum(clouds[k].shape[0] for k in range(1, 8)) == 70000 and 1000 < sizes[4] < 70000
    assert sizes[9] == sum(c.shape[0] for c in clouds)
    assert all(s > 100 for j, s in enumerate(sizes) if j not in (1, 2, 3, 5))


def test_batch_submaps_bit_exact(store):
    _check_batch(store, JOBS)


def test_batch_submaps_in_reverse_order(store):
    _check_batch(store, JOBS[::-1], also_one_by_one=False)


def test_batch_submaps_each_job_alone(store):
    for job in JOBS:
        _check_batch(store, [job], also_one_by_one=False)


def test_batch_of_64_jobs_every_third_empty_and_65_is_an_error(store):
    e, clouds, poses, _ = store
    small = [k for k, c in enumerate(clouds) if 300 <= c.shape[0] <= 2000 and k != 8]
    assert len(small) >= 7
    jobs = [(BEYOND + j, 1) if j % 3 == 2 else (small[j % len(small)], 0) for j in range(64)]
    got = _check_batch(store, jobs, also_one_by_one=False)
    assert all((g.shape[0] == 0) == (j % 3 == 2) for j, g in enumerate(got))
    jobs65 = jobs + [(0, 0)]
    with pytest.raises(SclError) as ei:
        e.selftest_submaps_batch(0, [k for k, _ in jobs65], [sn for _, sn in jobs65], [_window(poses, k, sn) for k, sn in jobs65], LEAF_B)
    assert ei.value.status == -1                                      # SCL_ERR_INVALID_ARG, the callee's own
    _check_batch(store, JOBS[:3])                                     # ... and the engine goes on working


def test_production_batch_of_40_candidates_in_two_rounds():
    """scl_loop_icp_batch_from_store with 40 candidates (two rounds of at most 32): keys behind the store, a window of nothing but
    non-finite points, repeated keys.  Sizes against the checker's submaps, every candidate against the one-by-one call in bits."""
    with ScanContextEngine() as e:
        base = synth_structured_cloud(24000, seed=3)
        clouds = [(base if k < 5 else synth_structured_cloud(24000, seed=40 + k))[k % 3::3][:4000].copy() for k in range(7)]
        clouds += [vc.cases()["nonfinite_all"][0]] * 3                                    # 7 .. 9: the window of key 8 holds no finite point
        clouds.append(moved_copy(base, rigid_transform(0.01, -0.015, 0.04, 0.25, -0.2, 0.05), keep_every=6, noise=0.005))   # 10: the scan
        for k, c in enumerate(clouds):
            e.keyframe_put(0, k, c)
        sn, leaf, cur = 1, 0.3, 10
        poses = [IDENT] * len(clouds)
        keys = ([1, 3, 50, 8, 5, 3, 2, 60, 4, 1] * 4)
        assert len(keys) == 40 and keys[31] != keys[32]
        pp = e.icp_default_params(); pp.max_iterations = 6
        Tb, fb, cb, ib, ns, ntb = e.loop_icp_batch_from_store(0, cur, IDENT, keys, sn, np.stack([np.stack(_window(poses, k, sn)) for k in keys]), leaf, pp)

        def size(key, s):
            ks = [k for k in range(key - s, key + s + 1) if 0 <= k < len(clouds)]
            return oi.voxel_grid(np.concatenate([oi.transform(clouds[k], IDENT) for k in ks]), leaf).shape[0] if ks else 0
        assert ns == size(cur, 0) >= 300
        single = {}
        for c, k in enumerate(keys):
            if k not in single:
                single[k] = (size(k, sn),) + e.loop_icp_from_store(0, cur, IDENT, k, sn, _window(poses, k, sn), leaf, pp)
            n_want, T1, f1, c1, i1, ns1, nt1 = single[k]
            assert ntb[c] == n_want == nt1 and ns1 == ns, (c, k)
            assert np.array_equal(Tb[c].view(np.uint32), T1.view(np.uint32)) and fb[c] == np.float32(f1) and cb[c] == c1 and ib[c] == i1, (c, k)
            if k in (50, 60, 8):                                      # skipped: identity, 0, 0, 0
                assert n_want == 0 and np.array_equal(Tb[c], IDENT) and fb[c] == 0 and not cb[c] and ib[c] == 0
            else:
                assert n_want >= 1000 and ib[c] > 0
