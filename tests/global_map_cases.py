"""The checker of the global voxel map (include/scl_engine.h "GLOBAL MAP") and the inputs of its GPU tests.

The checker restates the contract in numpy float64 -- normalise_pose's and qrot's operation order of scl_slam_amd/csrc/se3_device.hpp,
one IEEE operation per numpy operation, nothing fused -- with Python integers for keys and sums and a dict for the table.
tests/test_global_map_cases.py pins it by answers written out by hand and against PCL's filter (oracle/icp_oracle.c);
tests/test_gpu_global_map.py holds the device to it bit for bit."""
import numpy as np

BIAS = 1 << 20
RECORD = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("n", "<u4")])
M64 = (1 << 64) - 1
# Centroids of the checker against PCL's filter on a float-moved cloud (test_global_map_cases.py, the cross-check): 16 x the largest
# deviation measured there over PCL_CASES, 3.815e-06 m in each of the three -- one float ulp at the 32 .. 64 m the moved clouds reach:
# the float transform's rounding and the float sums of PCL's centroid; the checker's own truncation, leaf * 2^-20 <= 9.5e-7, is below
# it.  Measured against the oracle, never against the device.
TAU_PCL = 16 * 3.815e-06


def hash_key(x):
    """the table's hash (global_map_plan.hpp): splitmix64's finaliser"""
    x &= M64
    x ^= x >> 30; x = (x * 0xbf58476d1ce4e5b9) & M64
    x ^= x >> 27; x = (x * 0x94d049bb133111eb) & M64
    x ^= x >> 31
    return x


def make_key(cx, cy, cz):
    return ((int(cz) + BIAS) << 42) | ((int(cy) + BIAS) << 21) | (int(cx) + BIAS)


def capacity_for(n):
    c = 16
    while c < 2 * n:
        c <<= 1
    return c


def normalise_pose(pose):
    """(q[4], t[3]) of x, y, z, qx, qy, qz, qw: q divided by its norm, the squares summed left to right"""
    p = np.asarray(pose, np.float64)
    s = np.sqrt(((p[3] * p[3] + p[4] * p[4]) + p[5] * p[5]) + p[6] * p[6])
    return np.array([p[3] / s, p[4] / s, p[5] / s, p[6] / s]), p[:3].copy()


def qrot(q, v):
    """R(q) v for v[n,3] in float64: v + w c + u x c with c = 2 u x v, in se3_device.hpp's order"""
    v0, v1, v2 = v[:, 0], v[:, 1], v[:, 2]
    cx = 2.0 * (q[1] * v2 - q[2] * v1); cy = 2.0 * (q[2] * v0 - q[0] * v2); cz = 2.0 * (q[0] * v1 - q[1] * v0)
    o0 = (v0 + q[3] * cx) + (q[1] * cz - q[2] * cy)
    o1 = (v1 + q[3] * cy) + (q[2] * cx - q[0] * cz)
    o2 = (v2 + q[3] * cz) + (q[0] * cy - q[1] * cx)
    return np.stack([o0, o1, o2], axis=1)


def world(cloud, pose):
    q, t = normalise_pose(pose)
    with np.errstate(all="ignore"):
        return qrot(q, np.asarray(cloud, np.float32)[:, :3].astype(np.float64)) + t


def scaled(cloud, pose, leaf):
    """s = p_w * inv per point and axis"""
    inv = 1.0 / np.float64(np.float32(leaf))
    with np.errstate(all="ignore"):
        return world(cloud, pose) * inv


def voxels(cloud, pose, leaf):
    """(kept[n] bool, c[n,3] int64, f[n,3] int64) of a cloud at a pose; c and f are zero where a point is skipped"""
    s = scaled(cloud, pose, leaf)
    with np.errstate(all="ignore"):
        fl = np.floor(s)
        kept = ((fl >= -1048576.0) & (fl < 1048576.0)).all(axis=1)
        fr = np.floor((s - fl) * 1048576.0)
    c = np.where(kept[:, None], fl, 0.0).astype(np.int64)
    f = np.where(kept[:, None], fr, 0.0).astype(np.int64)
    return kept, c, f


def edge_distance(cloud, pose, leaf):
    """per point the smallest |s - round(s)| / max(1, |s|) over the axes (inf for a point that is not finite)"""
    s = scaled(cloud, pose, leaf)
    with np.errstate(all="ignore"):
        d = np.abs(s - np.rint(s)) / np.maximum(1.0, np.abs(s))
    d = np.where(np.isfinite(d), d, np.inf)
    return d.min(axis=1) if len(d) else np.zeros(0)


class MapChecker:
    """the map as the contract states it: table[key] = [n, Sx, Sy, Sz] in Python integers"""

    def __init__(self, leaf):
        self.leaf = np.float32(leaf)
        self.table, self.entries = {}, {}
        self.points_added = self.points_skipped = 0

    def _apply(self, cloud, pose, sign):
        kept, c, f = voxels(cloud, pose, self.leaf)
        self.points_skipped += sign * int((~kept).sum()); self.points_added += sign * int(kept.sum())
        c, f = c[kept], f[kept]
        if not len(c):
            return
        keys = ((c[:, 2] + BIAS).astype(np.uint64) << np.uint64(42)) | ((c[:, 1] + BIAS).astype(np.uint64) << np.uint64(21)) | (c[:, 0] + BIAS).astype(np.uint64)
        uniq, inverse, counts = np.unique(keys, return_inverse=True, return_counts=True)
        sums = np.zeros((len(uniq), 3), np.int64)
        np.add.at(sums, inverse, f)
        for k, n, s in zip(uniq.tolist(), counts.tolist(), sums.tolist()):
            v = self.table.setdefault(k, [0, 0, 0, 0])
            v[0] += sign * n; v[1] += sign * s[0]; v[2] += sign * s[1]; v[3] += sign * s[2]
            assert v[0] >= 0
            if v[0] == 0:
                assert v[1:] == [0, 0, 0]
                del self.table[k]

    def set(self, robot, index, cloud, pose):
        pose = np.asarray(pose, np.float64)
        old = self.entries.get((robot, index))
        if old is not None:
            if old[1].tobytes() == pose.tobytes():
                return "skip"
            self._apply(old[0], old[1], -1)
        self.entries[(robot, index)] = (np.asarray(cloud, np.float32).copy(), pose.copy())
        self._apply(cloud, pose, +1)
        return "add" if old is None else "repose"

    def remove(self, robot, index):
        cloud, pose = self.entries.pop((robot, index))
        self._apply(cloud, pose, -1)

    def records(self, box=None):
        keys = np.array(sorted(self.table), dtype=np.uint64)
        out = np.zeros(len(keys), RECORD)
        if not len(keys):
            return out
        vals = np.array([self.table[int(k)] for k in keys], dtype=np.int64)
        leaf = np.float64(self.leaf)
        den = vals[:, 0].astype(np.float64) * 1048576.0
        keep = np.ones(len(keys), bool)
        for a, name in enumerate("xyz"):
            c = ((keys >> np.uint64(21 * a)) & np.uint64((1 << 21) - 1)).astype(np.int64) - BIAS
            cen = (c.astype(np.float64) + vals[:, 1 + a].astype(np.float64) / den) * leaf
            out[name] = cen.astype(np.float32)
            if box is not None:
                keep &= (cen >= np.float64(box[a])) & (cen <= np.float64(box[3 + a]))
        out["n"] = np.minimum(vals[:, 0], 0xffffffff).astype(np.uint32)
        return out[keep]

    def stats(self):
        return {"keyframes": len(self.entries), "points_added": self.points_added, "points_skipped": self.points_skipped,
                "occupied_voxels": len(self.table)}


def build(leaf, kfs):
    """the checker's map of a list of (robot, index, cloud, pose)"""
    m = MapChecker(leaf)
    for r, x, cloud, pose in kfs:
        m.set(r, x, cloud, pose)
    return m


# ---- inputs --------------------------------------------------------------------------------------------------------------------

EDGE = 2.0 ** -30           # no randomised input has a coordinate s within EDGE * max(1, |s|) of an integer
IDENTITY = np.array([0, 0, 0, 0, 0, 0, 1.0])


def random_pose(rs, centre, spread):
    """a pose near `centre` whose quaternion is NOT normalised (squared norm in [0.36, 3.24])"""
    q = rs.standard_normal(4); q /= np.linalg.norm(q)
    return np.concatenate([np.asarray(centre, np.float64) + spread * rs.uniform(-1, 1, 3), q * rs.uniform(0.6, 1.8)])


def off_edges(cloud, pose, leaf, extra_poses=()):
    """the cloud without the points that lie within EDGE of a voxel face at the pose (and at every further pose it will be set at)"""
    keep = np.ones(len(cloud), bool)
    for p in (pose,) + tuple(extra_poses):
        keep &= edge_distance(cloud, p, leaf) > 4 * EDGE
    return np.ascontiguousarray(cloud[keep])


def random_keyframes(seed, n_kf, n_pts, leaf, extent=(30.0, 30.0, 6.0), centre=(0.0, 0.0, 0.0), spread=8.0, floats=4, robots=1, n_alt=0):
    """n_kf keyframes of about n_pts points uniform in a box of `extent` around the sensor, at random poses around `centre`: (robot,
    index, cloud[n, floats] float32, pose[7]); with n_alt > 0 a fifth entry, n_alt further poses the keyframe stays off the edges at"""
    rs = np.random.RandomState(seed)
    out = []
    for k in range(n_kf):
        cloud = np.zeros((n_pts, floats), np.float32)
        cloud[:, :3] = (rs.uniform(-0.5, 0.5, (n_pts, 3)) * np.asarray(extent)).astype(np.float32)
        if floats > 3:
            cloud[:, 3:] = rs.uniform(0, 255, (n_pts, floats - 3)).astype(np.float32)
        pose = random_pose(rs, centre, spread)
        alts = tuple(random_pose(rs, centre, spread) for _ in range(n_alt))
        cloud = off_edges(cloud, pose, leaf, alts)
        out.append((k % robots, k // robots, cloud, pose) + ((alts,) if n_alt else ()))
    return out


def lattice_voxels(coords, leaf=0.5, per_voxel=1, floats=4):
    """one keyframe at the identity whose points sit at exactly representable places inside the voxels `coords` (leaf a power of two,
    offsets multiples of leaf / 8): every s is exact"""
    coords = np.asarray(coords, np.int64).reshape(-1, 3)
    offs = np.array([0.5, 0.25, 0.75, 0.125, 0.875, 0.375, 0.625])[:per_voxel]
    pts = (coords[:, None, :].astype(np.float64) + offs[None, :, None]) * leaf
    cloud = np.zeros((len(coords) * len(offs), floats), np.float32)
    cloud[:, :3] = pts.reshape(-1, 3).astype(np.float32)
    assert (cloud[:, :3].astype(np.float64) == pts.reshape(-1, 3)).all()
    return cloud


def spread_voxels(seed, count, reach=200):
    """`count` distinct voxel coordinates in [-reach, reach)^3"""
    rs = np.random.RandomState(seed)
    seen = set()
    while len(seen) < count:
        seen.add(tuple(int(v) for v in rs.randint(-reach, reach, 3)))
    return sorted(seen)


def colliding_voxels(count, capacity, first_slot=5):
    """`count` voxels (cx, 0, 0), cx ascending from 0, whose keys hash to the SAME slot of a table of `capacity` slots: one probe chain"""
    out, cx = [], 0
    while len(out) < count:
        if hash_key(make_key(cx, 0, 0)) & (capacity - 1) == first_slot:
            out.append((cx, 0, 0))
        cx += 1
    return out


def face_lattice(leaf=0.5):
    """points ON voxel faces, edges and corners, negative coordinates included: multiples of the leaf in [-2, 2) on every axis (c = the
    multiple, f = 0), and the same shifted by half a leaf.  With the identity, or a 180 degree turn about z and a dyadic translation,
    every operation of the contract is exact"""
    g = np.arange(-4, 4, dtype=np.float64) * leaf
    on = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    pts = np.concatenate([on, on + leaf / 2])
    cloud = np.zeros((len(pts), 4), np.float32)
    cloud[:, :3] = pts.astype(np.float32)
    return cloud


HALF_TURN_Z = np.array([1.5, -0.25, 2.0, 0.0, 0.0, 1.0, 0.0])      # a 180 degree turn about z, translation dyadic: exact


def pose_matrix32(pose):
    """the float 4 x 4 of a pose, for PCL's float transform"""
    q, t = normalise_pose(pose)
    x, y, z, w = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = t
    return T.astype(np.float32)


def pcl_case(seed, n_kf=6, n_pts=1500, leaf=0.4, margin=1e-3):
    """keyframes with float-representable poses whose points, moved in double AND in float, stay `margin` leaves off every face, so that
    PCL's float placement and the contract's fp64 placement agree on every point's voxel"""
    import oracle_icp_binding as oi
    rs = np.random.RandomState(seed)
    out = []
    for k in range(n_kf):
        cloud = np.zeros((n_pts, 4), np.float32)
        cloud[:, :3] = (rs.uniform(-0.5, 0.5, (n_pts, 3)) * [40.0, 40.0, 8.0]).astype(np.float32)
        q = rs.standard_normal(4); q /= np.linalg.norm(q)
        pose = np.concatenate([rs.uniform(-20, 20, 3), q]).astype(np.float32).astype(np.float64)
        s64 = scaled(cloud, pose, leaf)
        moved = oi.transform(cloud, pose_matrix32(pose))[:, :3]
        s32 = (moved * (np.float32(1.0) / np.float32(leaf))).astype(np.float64)
        keep = np.ones(len(cloud), bool)
        for s in (s64, s32):
            keep &= (np.abs(s - np.rint(s)) > margin).all(axis=1)
        out.append((0, k, np.ascontiguousarray(cloud[keep]), pose))
    return out


PCL_CASES = [dict(seed=11), dict(seed=12, leaf=0.25), dict(seed=13, n_kf=3, n_pts=4000, leaf=1.0)]


def overflow_cloud(seed=7, n=3000):
    """a few thousand points over 2 km x 2 km x 50 m: at a leaf of 0.4 m PCL's linear index needs 5000 * 5000 * 125 > 2^31 voxels"""
    rs = np.random.RandomState(seed)
    cloud = np.zeros((n, 4), np.float32)
    cloud[:, :3] = (rs.uniform(-0.5, 0.5, (n, 3)) * [2000.0, 2000.0, 50.0]).astype(np.float32)
    cloud[0, :3] = (-1000.0, -1000.0, -25.0); cloud[1, :3] = (999.9, 999.9, 24.9)      # the corners: the extent is certain
    return off_edges(cloud, IDENTITY, 0.4)


_inputs = {}


def gpu_inputs(name):
    """the randomised inputs of tests/test_gpu_global_map.py by name: (leaf, keyframes); built once"""
    makers = {
        "overlap": lambda: (0.8, random_keyframes(1, 12, 400, 0.8, extent=(10.0, 10.0, 3.0), spread=2.0)),
        "kf257": lambda: (0.5, random_keyframes(2, 257, 40, 0.5, extent=(10.0, 10.0, 3.0), spread=3.0)),
        "repose64": lambda: (0.4, random_keyframes(3, 64, 150, 0.4, n_alt=1)),
        "far8km": lambda: (0.1, random_keyframes(4, 6, 500, 0.1, extent=(20.0, 20.0, 4.0), centre=(8000.0, -8000.0, 30.0), spread=20.0)),
        "stride12": lambda: (0.4, random_keyframes(5, 5, 300, 0.4, floats=3)),
        "stride16": lambda: (0.4, random_keyframes(5, 5, 300, 0.4, floats=4)),
        "stride32": lambda: (0.4, random_keyframes(5, 5, 300, 0.4, floats=8)),
        "big70k": lambda: (0.4, random_keyframes(6, 1, 70000, 0.4, extent=(60.0, 60.0, 10.0)) + [(0, 1) + random_keyframes(60, 1, 500, 0.4)[0][2:]]),
        "robots2": lambda: (0.4, random_keyframes(8, 10, 200, 0.4, robots=2)),
        "overflow": lambda: (0.4, [(0, 0, overflow_cloud(), IDENTITY.copy())]),
        "regrow": lambda: (0.5, random_keyframes(9, 16, 100, 0.5, extent=(12.0, 12.0, 4.0), spread=4.0, n_alt=2)),
    }
    if name is None:
        return sorted(makers)
    if name not in _inputs:
        _inputs[name] = makers[name]()
    return _inputs[name]
