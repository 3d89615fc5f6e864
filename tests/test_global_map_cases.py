"""The checker of the global voxel map (tests/global_map_cases.py) pinned without a GPU: by answers written out by hand, against PCL's
filter (oracle/icp_oracle.c: icpo_transform + icpo_voxel_grid) on keyframes with float-representable poses, and on its own inputs --
every randomised GPU input off every knife edge, the lattice inputs exact, remove-then-add equal to a fresh build."""
import numpy as np
import pytest

import global_map_cases as gm
import oracle_icp_binding as oi


def _cloud(points):
    c = np.zeros((len(points), 4), np.float32)
    c[:, :3] = np.asarray(points, np.float32)
    return c


def _rows(rec):
    return [(float(r["x"]), float(r["y"]), float(r["z"]), int(r["n"])) for r in rec]


def test_identity_faces_negative_coordinates_and_a_known_centroid():
    pts = [(0.5, 0.0, 1.0),                                             # on three faces: c = (1, 0, 2), f = 0
           (-0.25, -0.5, -0.75),                                        # floor, not truncation: c = (-1, -1, -2), f = (2^19, 0, 2^19)
           (0.125, 0.125, 0.125), (0.25, 0.125, 0.375), (0.375, 0.125, 0.25)]   # voxel (0, 0, 0): f / 2^18 = (1,1,1), (2,1,3), (3,1,2)
    kept, c, f = gm.voxels(_cloud(pts), gm.IDENTITY, 0.5)
    assert kept.all()
    assert c.tolist() == [[1, 0, 2], [-1, -1, -2], [0, 0, 0], [0, 0, 0], [0, 0, 0]]
    assert f.tolist() == [[0, 0, 0], [1 << 19, 0, 1 << 19], [1 << 18] * 3, [2 << 18, 1 << 18, 3 << 18], [3 << 18, 1 << 18, 2 << 18]]
    m = gm.build(0.5, [(0, 0, _cloud(pts), gm.IDENTITY)])
    assert m.table == {gm.make_key(1, 0, 2): [1, 0, 0, 0], gm.make_key(-1, -1, -2): [1, 1 << 19, 0, 1 << 19],
                       gm.make_key(0, 0, 0): [3, 6 << 18, 3 << 18, 6 << 18]}
    # ascending key: z first, then y, then x -- and the centroids exactly (every figure is dyadic)
    assert _rows(m.records()) == [(-0.25, -0.5, -0.75, 1), (0.25, 0.125, 0.25, 3), (0.5, 0.0, 1.0, 1)]
    assert m.stats() == {"keyframes": 1, "points_added": 5, "points_skipped": 0, "occupied_voxels": 3}
    assert gm.make_key(0, 0, 0) == (1 << 62) | (1 << 41) | (1 << 20) and gm.make_key(-gm.BIAS, -gm.BIAS, -gm.BIAS) == 0
    assert gm.make_key(gm.BIAS - 1, gm.BIAS - 1, gm.BIAS - 1) == (1 << 63) - 1


def test_a_quarter_turn_with_a_dyadic_translation():
    h = np.sqrt(0.5)
    pose = np.array([0.5, 0.0, -1.0, 0.0, 0.0, 2 * h, 2 * h])          # 90 degrees about z, the quaternion of norm 2
    # (1.25, 0.25, 0.25) -> (-0.25, 1.25, 0.25) + t = (0.25, 1.25, -0.75): voxel (0, 2, -2) of leaf 0.5, mid voxel on every axis
    m = gm.build(0.5, [(0, 0, _cloud([(1.25, 0.25, 0.25)]), pose)])
    assert list(m.table) == [gm.make_key(0, 2, -2)]
    r = m.records()[0]
    assert r["n"] == 1 and np.allclose([r["x"], r["y"], r["z"]], [0.25, 1.25, -0.75], atol=1e-6, rtol=0)
    # the exact half turn: every figure exact
    m = gm.build(0.5, [(0, 0, _cloud([(1.0, 0.5, 0.25)]), gm.HALF_TURN_Z)])
    assert _rows(m.records()) == [(0.5, -0.75, 2.25, 1)]


def test_the_ends_of_the_range_and_what_is_not_finite():
    pts = [(1048575.5, 0.5, 0.5), (1048576.5, 0.5, 0.5), (-1048575.5, 0.5, 0.5), (-1048576.5, 0.5, 0.5),
           (np.nan, 0.0, 0.0), (0.0, np.inf, 0.0), (0.0, 0.0, -np.inf), (0.5, 0.5, 0.5)]
    kept, c, _ = gm.voxels(_cloud(pts), gm.IDENTITY, 1.0)
    assert kept.tolist() == [True, False, True, False, False, False, False, True]
    assert c[0].tolist() == [gm.BIAS - 1, 0, 0] and c[2].tolist() == [-gm.BIAS, 0, 0]
    m = gm.build(1.0, [(0, 0, _cloud(pts), gm.IDENTITY)])
    assert m.stats() == {"keyframes": 1, "points_added": 3, "points_skipped": 5, "occupied_voxels": 3}
    # a point that leaves the range only through the pose's translation
    far = gm.IDENTITY.copy(); far[0] = 1048576.0
    assert gm.voxels(_cloud([(0.5, 0.5, 0.5), (-0.5, 0.5, 0.5)]), far, 1.0)[0].tolist() == [False, True]
    m.remove(0, 0)
    assert m.table == {} and m.stats() == {"keyframes": 0, "points_added": 0, "points_skipped": 0, "occupied_voxels": 0}


def test_a_tiny_negative_coordinate_counts_at_the_upper_face():
    """-1 < s < 0 is where s - floor(s) rounds: the contract's one inexact case, restated bit for bit by the checker"""
    kept, c, f = gm.voxels(_cloud([(-1e-30, 0.25, 0.25)]), gm.IDENTITY, 0.5)
    assert kept.all() and c[0].tolist() == [-1, 0, 0] and f[0].tolist() == [1 << 20, 1 << 19, 1 << 19]


def test_every_randomised_gpu_input_is_off_every_knife_edge():
    checked = 0
    for name in gm.gpu_inputs(None):
        leaf, kfs = gm.gpu_inputs(name)
        for kf in kfs:
            for pose in (kf[3],) + tuple(kf[4] if len(kf) > 4 else ()):
                d = gm.edge_distance(kf[2], pose, leaf)
                assert len(d) and d.min() > gm.EDGE, (name, kf[:2], d.min())
                checked += len(d)
    assert checked > 100000


def test_the_lattice_inputs_are_exact():
    cloud = gm.face_lattice(0.5)
    for pose in (gm.IDENTITY, gm.HALF_TURN_Z):
        s = gm.scaled(cloud, pose, 0.5)
        assert (s * 2 == np.rint(s * 2)).all()                         # every s a multiple of one half: faces are hit exactly
        kept, c, f = gm.voxels(cloud, pose, 0.5)
        assert kept.all() and set(np.unique(f).tolist()) == {0, 1 << 19}
        assert (c.astype(np.float64) + f / 1048576.0 == s).all()
    on_faces = int((gm.voxels(cloud, gm.IDENTITY, 0.5)[2] == 0).all(axis=1).sum())
    assert on_faces == 512                                              # the 8^3 lattice corners
    cloud = gm.lattice_voxels(gm.spread_voxels(1, 1000), per_voxel=3)
    kept, c, f = gm.voxels(cloud, gm.IDENTITY, 0.5)
    assert kept.all() and len({tuple(v) for v in c.tolist()}) == 1000
    chain = gm.colliding_voxels(20, 64)
    assert len({gm.hash_key(gm.make_key(*v)) & 63 for v in chain}) == 1 and len(set(chain)) == 20


def test_remove_then_add_equals_a_fresh_build():
    leaf, kfs = gm.gpu_inputs("repose64")
    m = gm.build(leaf, [kf[:4] for kf in kfs])
    before = m.records().tobytes()
    for kf in kfs[::2]:
        assert m.set(kf[0], kf[1], kf[2], kf[4][0]) == "repose"
    assert m.set(*kfs[1][:4]) == "skip"
    final = [kf[:3] + (kf[4][0] if i % 2 == 0 else kf[3],) for i, kf in enumerate(kfs)]
    fresh = gm.build(leaf, final)
    assert m.records().tobytes() == fresh.records().tobytes() and m.table == fresh.table and m.stats() == fresh.stats()
    assert m.records().tobytes() != before
    for kf in kfs:
        m.remove(kf[0], kf[1])
    assert m.table == {} and len(m.records()) == 0


def test_a_float_transform_places_points_elsewhere_8_km_out():
    leaf, kfs = gm.gpu_inputs("far8km")
    differ = 0
    for _, _, cloud, pose in kfs:
        T = gm.pose_matrix32(pose)
        moved = np.zeros_like(cloud)
        moved[:, :3] = (cloud[:, :3] @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
        c64 = gm.voxels(cloud, pose, leaf)[1]; c32 = gm.voxels(moved, gm.IDENTITY, leaf)[1]
        differ += int((c64 != c32).any(axis=1).sum())
    # a float's ulp at 8 km is 0.49 mm and the leaf 0.1 m: about one point in 400 lands in another voxel, of 3 000
    assert differ >= 1


def _pcl(kfs, leaf):
    moved = np.concatenate([oi.transform(cloud, gm.pose_matrix32(pose)) for _, _, cloud, pose in kfs])
    return moved, oi.voxel_grid(moved, leaf)


@pytest.mark.parametrize("case", gm.PCL_CASES, ids=lambda c: f"seed{c['seed']}")
def test_against_pcls_filter_on_float_representable_poses(case):
    kfs = gm.pcl_case(**case)
    leaf = case.get("leaf", 0.4)
    m = gm.build(leaf, kfs)
    moved, filtered = _pcl(kfs, leaf)
    # PCL's voxel of every moved point (float: floor(x * inverse_leaf_size)) -- the same voxels with the same counts
    ijk = np.floor(moved[:, :3] * (np.float32(1.0) / np.float32(leaf))).astype(np.int64)
    keys, counts = np.unique([gm.make_key(*v) for v in ijk.tolist()], return_counts=True)
    assert {int(k): int(n) for k, n in zip(keys, counts)} == {k: v[0] for k, v in m.table.items()}
    rec = m.records()
    assert filtered is not None and len(filtered) == len(rec)          # and PCL's output, in PCL's order, is the map's
    dev = max(float(np.abs(filtered[:, a].astype(np.float64) - rec[n].astype(np.float64)).max()) for a, n in enumerate("xyz"))
    print(f"largest centroid deviation from PCL's filter: {dev:.3e} m (TAU_PCL = {gm.TAU_PCL:.3e})")
    assert dev <= gm.TAU_PCL
