"""Clouds the GRSD tests share (tests/test_grsd_checker.py on the CPU, tests/test_gpu_grsd.py on the GPU): the three clouds with
known answers and the drawn clouds of the restatement comparison.  A plain module, no fixtures."""
import numpy as np

from scl_slam_amd.synth import synth_scan, synth_structured_cloud


def plane():
    """x, y in {0.05 + 0.1 k : k = 0 .. 79}, z = 1: 16 voxels (4 x 4 x 1), every normal equal, every voxel a plane (class 1)"""
    k = (0.05 + 0.1 * np.arange(80)).astype(np.float32)
    x, y = np.meshgrid(k, k, indexing="ij")
    return np.ascontiguousarray(np.stack([x.ravel(), y.ravel(), np.ones(6400, np.float32)], axis=1), np.float32)


def sparse():
    """a lattice at 1.0 m spacing (8 x 8 x 4 points, 4 x 4 x 2 voxels): no point has 3 neighbours within 0.5 m"""
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(4), indexing="ij"), axis=-1).reshape(-1, 3)
    return np.ascontiguousarray(g.astype(np.float32) + np.float32(0.5))


def lonely():
    """the plane and one point more than 4 m from everything else, the last voxel in index order"""
    return np.ascontiguousarray(np.concatenate([plane(), np.array([[30.0, 30.0, 1.0]], np.float32)]))


# With the reference's radius of 2.0 m the distance bins sit at 0.2 .. 1.8 m and no angle exceeds pi / 2, so every radius is at
# least 1.1 * 0.2 / (pi / 2) = 0.14 > 0.1: a voxel with two neighbours is a plane (class 1), any other is noise (class 0).  The
# other classes need a radius at the scale of the objects: the restatement comparison runs at SMALL = (ne_radius, grsd_radius).
SMALL = (0.06, 0.25)


def small_scene(n, seed, noise=0.0):
    """table-top objects for SMALL: a ground patch, a sphere, a thin cylinder, two walls meeting in an edge, a blob of scattered
    points and three stray points (noise voxels), n points in all, optional Gaussian noise on every coordinate"""
    rs = np.random.RandomState(seed)
    m = n // 6
    g = np.stack([rs.uniform(-0.7, 0.7, 2 * m), rs.uniform(-0.7, 0.7, 2 * m), np.zeros(2 * m)], axis=1)
    u = rs.standard_normal((m, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    sph = 0.07 * u + np.array([0.3, 0.3, 0.3])
    ang = rs.uniform(0, 2 * np.pi, m)
    cyl = np.stack([-0.3 + 0.03 * np.cos(ang), -0.3 + 0.03 * np.sin(ang), rs.uniform(0.0, 0.6, m)], axis=1)
    h = m // 2
    w1 = np.stack([rs.uniform(0.0, 0.4, h) - 0.5, np.full(h, 0.4), rs.uniform(0.0, 0.4, h)], axis=1)
    w2 = np.stack([np.full(m - h, -0.5), 0.4 - rs.uniform(0.0, 0.4, m - h), rs.uniform(0.0, 0.4, m - h)], axis=1)
    blob = rs.uniform(-0.15, 0.15, (n - 5 * m - 3, 3)) + np.array([0.4, -0.4, 0.3])
    stray = np.array([[1.5, 1.5, 1.0], [-1.6, 1.4, 0.8], [1.5, -1.6, 1.2]])
    pts = np.concatenate([g, sph, cyl, w1, w2, blob, stray])
    if noise:
        pts = pts + noise * rs.standard_normal(pts.shape)
    c = np.zeros((n, 4), np.float32)
    c[:, :3] = pts[rs.permutation(n)].astype(np.float32)
    return c


def restatement_clouds():
    """name -> (cloud, ne_radius, grsd_radius)"""
    out = {"scene_a": (small_scene(2400, 11), *SMALL), "scene_b": (small_scene(3000, 12, noise=0.004), *SMALL),
           "structured": (synth_structured_cloud(2500, seed=13, extent=7.0, stride_floats=4), 0.5, 2.0),
           "scan": (synth_scan(2500, seed=14, max_range=9.0, stride_floats=4), 0.5, 2.0)}
    return out
