"""The CPU checker and the named inputs of the batched registration scoring (include/scl_engine.h "BATCHED REGISTRATION SCORING";
numpy on top of the checker's icpo_transform and icpo_nn).

checker(src, tgt, T, max_dist) restates one candidate: the source moved by T in float32 (icpo_transform, scl_transform_cloud's
arithmetic), every moved point's nearest target point and float32 squared distance (icpo_nn; ties -> lowest index), then
  n_valid    points that found a neighbour (a non-finite moved point finds none)
  n_inliers  those with d2 <= maxd2, compared in float32, maxd2 = float32(max_dist * max_dist) with the product formed in double
  sums       math.fsum over the inliers of x, y, z, xx, yy, zz, xy, xz, yz (the matched TARGET point in double; every product of two
             floats is exact in double) and of d2 -- the correctly rounded sums
  abs_sums   math.fsum of the terms' absolute values: what the GPU test's bound m * 2^-53 * abs_sums * (1 + 2^-20) is made of
information(m, S) restates scl_registration_information.

CASES names every input the GPU tests hold to the checker; case(name) -> (src, tgts, transforms[m,4,4] float32, max_dist).
tests/test_registration_eval_cases.py shows with the checker alone that every one but LATTICE is off the inlier knife edge.  (The store
forms and the 20 x 60 chain are held to the host form and to properties, not to the checker: their clouds come out of the device's
voxel filter.)

  list        one source (every second point of a structured place, 1 cm of noise) against five candidates: the place under small
              and large motions, one of them empty; the transforms are the true motions behind small errors, so that the distances
              straddle max_dist = 0.05
  n1 n32 n33  the list's clouds cycled to 1, 32 and 33 candidates with distinct transforms (rounds of 32)
  src_N       N = 1, 2, 3, 255, 256, 257, 4097 source points (one workgroup of the reduction is 256, its partition changes at 64 x 256
              -- 4 097 sources are 17 workgroups) against the list
  overflow    two finite source points at 2.5e38 that a factor 1.5 in the transform's first row sends to infinity
  nan         rows of the source with a NaN coordinate
  maxd0       max_dist = 0: every point valid, none an inlier (no distance of the noisy source is exactly zero)
  all         max_dist = 1e30, whose square is infinite in float32: every valid point an inlier
  LATTICE     a 2 m lattice, the source its own points, the transform 0.5 m along x: every d2 is exactly 0.25 = maxd2 of max_dist 0.5
              (kept); the one case ON the edge"""
import functools
import math

import numpy as np

import oracle_icp_binding as oi
from scl_slam_amd.synth import rigid_transform, synth_structured_cloud

NOISE = 0.01
MAX_DIST = 0.05
LATTICE = "lattice"
SIZES = (1, 2, 3, 255, 256, 257, 4097)
CASES = ("list", "n1", "n32", "n33") + tuple(f"src_{n}" for n in SIZES) + ("overflow", "nan", "maxd0", "all", LATTICE)

_TRUE = (rigid_transform(0.01, -0.02, 0.05, 0.3, -0.2, 0.1),
         rigid_transform(0.01, -0.02, np.radians(91.3), 12.0, -31.0, 0.4),
         rigid_transform(-0.015, 0.01, np.radians(179.0), -27.0, 18.0, -0.3),
         None,                                                                       # the empty candidate
         rigid_transform(0.0, 0.0, np.radians(-33.0), 3.0, 4.0, 0.0))
_ERR = (rigid_transform(0.0, 0.0, 0.0, 0.03, -0.02, 0.01),
        rigid_transform(0.0004, -0.0003, np.radians(0.03), 0.02, -0.015, 0.005),
        rigid_transform(-0.0002, 0.0005, np.radians(-0.05), -0.02, 0.03, -0.004),
        rigid_transform(0.0, 0.0, 0.0, 0.0, 0.0, 0.0),
        rigid_transform(0.0, 0.0, np.radians(0.1), 0.05, 0.0, 0.0))                  # a poor registration: few inliers


def _moved(cloud, T):
    """the cloud's x, y, z moved by T in double, rounded once (how the inputs are MADE; the calls move clouds in float32)"""
    out = cloud.copy()
    out[:, :3] = (cloud[:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    return out


@functools.lru_cache(maxsize=None)
def place():
    return synth_structured_cloud(3000, seed=31)


@functools.lru_cache(maxsize=None)
def source():
    src = place()[::2].copy()
    src[:, :3] += (NOISE * np.random.RandomState(6).standard_normal((src.shape[0], 3))).astype(np.float32)
    return src


def long_source(n):
    """n points: the source repeated, every copy shifted by another 13 mm along x"""
    s = source()
    parts = [s.copy() for _ in range((n + len(s) - 1) // len(s))]
    for k, p in enumerate(parts):
        p[:, 0] += np.float32(0.013 * k)
    return np.ascontiguousarray(np.concatenate(parts)[:n])


@functools.lru_cache(maxsize=None)
def _list():
    tgts = [np.ascontiguousarray(_moved(place(), T)) if T is not None else place()[:0].copy() for T in _TRUE]
    Ts = np.stack([(E @ (T if T is not None else np.eye(4))).astype(np.float32) for E, T in zip(_ERR, _TRUE)])
    return tgts, Ts


def _cycled(n):
    tgts, Ts = _list()
    m = len(tgts)
    out_t = [tgts[c % m] for c in range(n)]
    out_T = np.stack([(rigid_transform(0, 0, np.radians(0.002 * c), 0.0007 * c, 0, 0) @ Ts[c % m].astype(np.float64)).astype(np.float32)
                      for c in range(n)])
    assert len({T.tobytes() for T in out_T}) == n
    return out_t, out_T


@functools.lru_cache(maxsize=None)
def case(name):
    tgts, Ts = _list()
    if name == "list":
        return source(), tgts, Ts, MAX_DIST
    if name in ("n1", "n32", "n33"):
        t, T = _cycled(int(name[1:]))
        return source(), t, T, MAX_DIST
    if name.startswith("src_"):
        return long_source(int(name[4:])), tgts, Ts, MAX_DIST
    if name == "overflow":
        src = source().copy()
        src[7, 0] = np.float32(2.5e38); src[900, 0] = np.float32(-2.5e38)
        T = Ts[:3].copy()
        T[:, 0, 0] *= np.float32(1.5)                                  # 2.5e38 x 1.5 cos(yaw) is beyond float32 for yaws near 0 and 180 degrees
        T[1, 0, 0] = np.float32(1.5)                                   # (candidate 1's cosine is near zero)
        return src, tgts[:3], T, MAX_DIST
    if name == "nan":
        src = source().copy()
        src[3, 0] = np.nan; src[400, 1] = np.nan; src[1499, 2] = np.nan; src[77, :3] = np.nan
        return src, tgts, Ts, MAX_DIST
    if name == "maxd0":
        return source(), tgts, Ts, 0.0
    if name == "all":
        return source(), tgts, Ts, 1e30
    if name == LATTICE:
        g = np.arange(10, dtype=np.float32) * np.float32(2.0)
        pts = np.zeros((1000, 8), np.float32)
        pts[:, :3] = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
        src = np.ascontiguousarray(pts[::2])
        T = np.stack([rigid_transform(0, 0, 0, 0.5, 0, 0), rigid_transform(0, 0, 0, -0.5, 0, 0), rigid_transform(0, 0, 0, 0, 0.5, 0)]).astype(np.float32)
        return src, [pts, pts, pts], T, 0.5
    raise KeyError(name)


def maxd2_of(max_dist):
    with np.errstate(over="ignore"):
        return np.float32(float(max_dist) * float(max_dist))


def pairs(src, tgt, T):
    """(nn index, float32 nn_dist2) of the source moved by T, from the checker"""
    src = np.ascontiguousarray(src, np.float32); tgt = np.ascontiguousarray(tgt, np.float32)
    if len(src) == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.float32)
    moved = oi.transform(src, T)
    if len(tgt) == 0:
        return np.full(len(src), -1, np.int32), np.full(len(src), np.finfo(np.float32).max, np.float32)
    return oi.nn(moved, tgt, use_grid=len(src) * len(tgt) > 50_000_000)   # (the brute-force walk: exact, and quick at these sizes)


def sums_of(tgt, idx, d2, max_dist):
    """(n_valid, n_inliers, sums[10], abs_sums[10]) of one candidate's pairs: the definition, with math.fsum"""
    valid = idx >= 0
    inl = valid & (d2 <= maxd2_of(max_dist))
    q = np.ascontiguousarray(tgt, np.float32)[idx[inl], :3].astype(np.float64)
    x, y, z = (q[:, 0], q[:, 1], q[:, 2]) if len(q) else (np.zeros(0),) * 3
    terms = [x, y, z, x * x, y * y, z * z, x * y, x * z, y * z, d2[inl].astype(np.float64)]
    sums = np.array([math.fsum(t.tolist()) for t in terms])
    abs_sums = np.array([math.fsum(np.abs(t).tolist()) for t in terms])
    return int(valid.sum()), int(inl.sum()), sums, abs_sums


def checker(src, tgt, T, max_dist):
    idx, d2 = pairs(src, tgt, T)
    return sums_of(tgt, idx, d2, max_dist)


@functools.lru_cache(maxsize=None)
def checked(name):
    """the checker's answer for every candidate of a named case, computed once"""
    src, tgts, Ts, max_dist = case(name)
    return [checker(src, t, T, max_dist) for t, T in zip(tgts, Ts)]


def information(m, S):
    """scl_registration_information restated: sum of G^T G for G = [-[q]x | I3], rotation first"""
    Sx, Sy, Sz, Sxx, Syy, Szz, Sxy, Sxz, Syz = (np.float64(v) for v in S[:9])
    m = np.float64(m)
    return np.array([[Syy + Szz, -Sxy, -Sxz, 0.0, -Sz, Sy],
                     [-Sxy, Sxx + Szz, -Syz, Sz, 0.0, -Sx],
                     [-Sxz, -Syz, Sxx + Syy, -Sy, Sx, 0.0],
                     [0.0, Sz, -Sy, m, 0.0, 0.0],
                     [-Sz, 0.0, Sx, 0.0, m, 0.0],
                     [Sy, -Sx, 0.0, 0.0, 0.0, m]], np.float64)


def jittered(cloud, seed):
    """a copy with a random half of the coordinates moved one ulp, up or down"""
    rs = np.random.RandomState(seed)
    out = np.ascontiguousarray(cloud, np.float32).copy()
    xyz = out[:, :3]
    move = rs.rand(*xyz.shape) < 0.5
    toward = np.where(rs.rand(*xyz.shape) < 0.5, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)
    out[:, :3] = np.where(move & np.isfinite(xyz), np.nextafter(xyz, toward), xyz)
    return out
