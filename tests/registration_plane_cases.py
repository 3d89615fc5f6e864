"""The CPU checker and the named inputs of the point-to-plane registration scoring (include/scl_engine.h "POINT-TO-PLANE REGISTRATION
SCORING"), on top of tests/registration_eval_cases.py.

checker(src, tgt, T, max_dist, normals) restates one candidate.  The pairs are registration_eval_cases.pairs' (the source moved by
T in float32 with icpo_transform, every moved point's nearest target point and float32 squared distance from icpo_nn); the normals
are an INPUT, (n_tgt, 3) float32 -- the CPU tests pass the checker's icpo_normals, the GPU tests the device's target_normals, so the
sums are held to the definition on exactly the normals the device used.  It answers a PlaneCheck:
  n_valid, n_inliers   as registration_eval_cases.sums_of counts them
  n_planar             the inliers whose normal is not (0, 0, 0)
  exact[28]            the plane sums as fractions.Fraction, formed without a single rounding: the upper triangle of sum J^T J for
                       J = (p x n, n) (21), sum J r for r = (q - p) . n (6), sum r r.  Every float32 is an integer multiple of 2^-149,
                       so the sums are formed over Python integers with the common power-of-two denominator kept aside and handed
                       to Fraction at the end -- the same rationals as Fraction arithmetic term by term (which
                       tests/test_registration_plane_cases.py shows), a hundred times sooner
  major[28]            float64: the same sums with every term replaced by its majorant, R = (|p_y n_z| + |p_z n_y|, ..., |n_x|, |n_y|,
                       |n_z|) for J and rbar = sum_k (|q_k| + |p_k|) |n_k| for r -- what the bound (n_planar + 10) * 2^-53 * major is made of
  d2_sum               math.fsum of (double)d2 over ALL inliers (the device's sums[28] is held bit for bit to the existing eval's
                       moments[9] instead)
information_plane(sums) restates scl_registration_information_plane.

case(name) -> (src, tgts, transforms[m,4,4] float32, max_dist, normal_radius).  The place is synth_structured_cloud(3000, seed=31,
extent=8.0): the 40 m place of the point-to-point cases is too sparse for normals (1 679 of its 3 000 points have fewer than three
neighbours within 1 m); of this one 3 points have none, which is wanted.  Every case but the lattice has its source taken off the
inlier knife edge (_off_edge).
  list         a source of every second point with 1 cm of noise against five candidates: the place under small and large motions,
                one of them empty; the transforms are the true motions behind small errors, max_dist = 0.05, radius 1
  n1 n32 n33    the list's clouds cycled to 1, 32 and 33 candidates with distinct transforms (rounds of 32)
  src_N         N = 1, 2, 3, 255, 256, 257, 4 097 source points against the list; 16 385 (a lane's second trip: 64 workgroups of 256
                cover 16 384) and 65 537 (the four-trip loop's second pass: 4 x 16 384) against one candidate each
  sparse        the place plus 40 isolated points that the source matches: n_planar < n_inliers
  tiny_radius   radius 1e-3: no point has a neighbour, every normal is zero, the plane sums are 0 and the sum of d2 is not
  huge_radius   radius 100, beyond the cloud: every point's ball is the whole cloud
  tgt1 tgt2     targets of 1 and 2 points (no normal)
  nan overflow maxd0 all   as in the point-to-point cases
  lattice       the 2 m lattice, every d2 exactly maxd2 (kept), radius 2.5 (a point and its six neighbours)
  corridor      a floor and two parallel walls along x, 3 000 points with 1 cm of noise: nothing constrains the motion along x"""
import functools
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np

import oracle_icp_binding as oi
import registration_eval_cases as rc
from scl_slam_amd.synth import rigid_transform, synth_structured_cloud

MAX_DIST = rc.MAX_DIST
RADIUS = 1.0
LATTICE = rc.LATTICE
SIZES = (1, 2, 3, 255, 256, 257, 4097)
SIZES_ONE = (16385, 65537)                                    # against one candidate each
CASES = (("list", "n1", "n32", "n33") + tuple(f"src_{n}" for n in SIZES + SIZES_ONE) +
         ("sparse", "tiny_radius", "huge_radius", "tgt1", "tgt2", "nan", "overflow", "maxd0", "all", LATTICE, "corridor"))

PlaneCheck = namedtuple("PlaneCheck", "n_valid n_inliers n_planar exact major d2_sum")
_SCALE = 149                                                  # every finite float32 times 2^149 is an integer


@functools.lru_cache(maxsize=None)
def place():
    return synth_structured_cloud(3000, seed=31, extent=8.0)


def _noisy_half(cloud, seed=6):
    src = cloud[::2].copy()
    src[:, :3] += (rc.NOISE * np.random.RandomState(seed).standard_normal((src.shape[0], 3))).astype(np.float32)
    return src


@functools.lru_cache(maxsize=None)
def source():
    return _noisy_half(place())


def long_source(n):
    """n points: the source repeated, every copy shifted by another 1.1 mm along x"""
    s = source()
    parts = [s.copy() for _ in range((n + len(s) - 1) // len(s))]
    for k, p in enumerate(parts):
        p[:, 0] += np.float32(0.0011 * k)
    return np.ascontiguousarray(np.concatenate(parts)[:n])


@functools.lru_cache(maxsize=None)
def _list():
    tgts = [np.ascontiguousarray(rc._moved(place(), T)) if T is not None else place()[:0].copy() for T in rc._TRUE]
    Ts = np.stack([(E @ (T if T is not None else np.eye(4))).astype(np.float32) for E, T in zip(rc._ERR, rc._TRUE)])
    return tgts, Ts


def _cycled(n):
    tgts, Ts = _list()
    m = len(tgts)
    out_T = np.stack([(rigid_transform(0, 0, np.radians(0.002 * c), 0.0007 * c, 0, 0) @ Ts[c % m].astype(np.float64)).astype(np.float32)
                      for c in range(n)])
    assert len({T.tobytes() for T in out_T}) == n
    return [tgts[c % m] for c in range(n)], out_T


@functools.lru_cache(maxsize=None)
def corridor():
    """20 m of floor (3 m wide) and two walls 2.5 m high along x, 1 cm of noise across each plane"""
    rs = np.random.RandomState(44)
    n = 3000
    pts = np.zeros((n, 8), np.float32)
    x = rs.uniform(-10.0, 10.0, n); noise = 0.01 * rs.standard_normal(n)
    k = n // 3
    u = rs.uniform(-1.5, 1.5, n); h = rs.uniform(0.0, 2.5, n)
    pts[:k, :3] = np.stack([x[:k], u[:k], noise[:k]], 1)
    pts[k:2 * k, :3] = np.stack([x[k:2 * k], -1.5 + noise[k:2 * k], h[k:2 * k]], 1)
    pts[2 * k:, :3] = np.stack([x[2 * k:], 1.5 + noise[2 * k:], h[2 * k:]], 1)
    return pts


@functools.lru_cache(maxsize=None)
def _sparse():
    """the place plus 40 points on their own, 3 m apart and 10 m above everything else; the source has them too"""
    extra = np.zeros((40, 8), np.float32)
    extra[:, 0] = 3.0 * (np.arange(40) % 8) - 10.5; extra[:, 1] = 3.0 * (np.arange(40) // 8) - 6.0; extra[:, 2] = 16.0
    tgt = np.ascontiguousarray(np.concatenate([place(), extra]))
    src = np.ascontiguousarray(np.concatenate([source(), extra + np.float32([0.004, -0.003, 0.002, 0, 0, 0, 0, 0])]))
    return src, tgt


def _off_edge(src, tgts, Ts, max_dist):
    """the source with every point whose nn_dist2 lies within 0.1 % of maxd2 for some candidate pushed 3 mm along each axis, until
    there is none: a place this dense has, among 1 300 inliers per candidate, a pair within a few ulps of the inlier rule for one
    candidate in ten, and no count of these cases is to hang on a rounding (tests/test_registration_plane_cases.py shows it)"""
    maxd2 = float(rc.maxd2_of(max_dist))
    if not (0.0 < maxd2 < np.inf):
        return src
    src = src.copy()
    for _ in range(20):
        bad = np.zeros(len(src), bool)
        for t, T in zip(tgts, Ts):
            idx, d2 = rc.pairs(src, t, T)
            bad |= (idx >= 0) & (np.abs(d2.astype(np.float64) - maxd2) < 1e-3 * maxd2)
        if not bad.any():
            return src
        src[bad, :3] += np.float32(0.003)
    raise AssertionError("no source off the edge found")


@functools.lru_cache(maxsize=None)
def case(name):
    src, tgts, Ts, max_dist, radius = _case(name)
    return (src if name == LATTICE else _off_edge(src, tgts, Ts, max_dist)), tgts, Ts, max_dist, radius


def _case(name):
    tgts, Ts = _list()
    if name == "list":
        return source(), tgts, Ts, MAX_DIST, RADIUS
    if name in ("n1", "n32", "n33"):
        t, T = _cycled(int(name[1:]))
        return source(), t, T, MAX_DIST, RADIUS
    if name.startswith("src_"):
        n = int(name[4:])
        return (long_source(n), tgts, Ts, MAX_DIST, RADIUS) if n in SIZES else (long_source(n), tgts[:1], Ts[:1], MAX_DIST, RADIUS)
    if name == "sparse":
        src, tgt = _sparse()
        return src, [tgt, tgts[1]], np.stack([rc._ERR[0].astype(np.float32), Ts[1]]), MAX_DIST, RADIUS
    if name == "tiny_radius":
        return source(), tgts[:2], Ts[:2], MAX_DIST, 1e-3
    if name == "huge_radius":
        return source(), tgts[:2], Ts[:2], MAX_DIST, 100.0
    if name in ("tgt1", "tgt2"):
        k = int(name[3:])
        return source(), [np.ascontiguousarray(tgts[0][:k]), np.ascontiguousarray(tgts[1][:k])], Ts[:2], MAX_DIST, RADIUS
    if name in ("overflow", "nan"):
        src = source().copy()
        if name == "nan":
            src[3, 0] = np.nan; src[400, 1] = np.nan; src[1499, 2] = np.nan; src[77, :3] = np.nan
            return src, tgts, Ts, MAX_DIST, RADIUS
        src[7, 0] = np.float32(2.5e38); src[900, 0] = np.float32(-2.5e38)
        T = Ts[:3].copy()
        T[:, 0, 0] *= np.float32(1.5)                                  # (as in the point-to-point case: beyond float32 after the move)
        T[1, 0, 0] = np.float32(1.5)
        return src, tgts[:3], T, MAX_DIST, RADIUS
    if name == "maxd0":
        return source(), tgts, Ts, 0.0, RADIUS
    if name == "all":
        return source(), tgts, Ts, 1e30, RADIUS
    if name == LATTICE:
        src, t, T, max_dist = rc.case(rc.LATTICE)
        return src, t, T, max_dist, 2.5
    if name == "corridor":
        c = corridor()
        T = np.stack([rigid_transform(0.0003, -0.0002, np.radians(0.02), 0.01, -0.006, 0.004),
                      rigid_transform(0.0, 0.0, 0.0, 0.02, 0.0, 0.0)]).astype(np.float32)
        return _noisy_half(c, seed=9), [c, c], T, MAX_DIST, RADIUS
    raise KeyError(name)


def distinct_targets(name):
    """the distinct non-empty target clouds of a case (the cycled cases repeat five)"""
    seen, out = set(), []
    for t in case(name)[1]:
        if id(t) not in seen and len(t):
            seen.add(id(t)); out.append(t)
    return out


def _ints(a):
    """a float32 array -> an object array of Python integers, value * 2^149 (exact: a power of two scales a double exactly)"""
    flat = (np.asarray(a, np.float32).astype(np.float64) * 2.0 ** _SCALE).ravel()
    return np.array([int(v) for v in flat], dtype=object).reshape(np.shape(a))


def plane_sums(p, q, n):
    """the 28 exact sums and their majorants over given pairs: p, q, n are (m,3) float32 (moved source, target, normal != 0)"""
    m = len(p)
    if m == 0:
        return [Fraction(0)] * 28, np.zeros(28)
    P, Q, N = _ints(p), _ints(q), _ints(n)
    rot = [P[:, 1] * N[:, 2] - P[:, 2] * N[:, 1], P[:, 2] * N[:, 0] - P[:, 0] * N[:, 2], P[:, 0] * N[:, 1] - P[:, 1] * N[:, 0]]   # x 2^-298
    one = 1 << _SCALE
    J = rot + [N[:, 0] * one, N[:, 1] * one, N[:, 2] * one]                                                                  # all x 2^-298
    r = (Q[:, 0] - P[:, 0]) * N[:, 0] + (Q[:, 1] - P[:, 1]) * N[:, 1] + (Q[:, 2] - P[:, 2]) * N[:, 2]                            # x 2^-298
    den = 1 << (4 * _SCALE)
    exact = [Fraction(int((J[a] * J[b]).sum()), den) for a in range(6) for b in range(a, 6)]
    exact += [Fraction(int((J[a] * r).sum()), den) for a in range(6)] + [Fraction(int((r * r).sum()), den)]
    pd, qd, nd = (np.abs(np.asarray(v, np.float32).astype(np.float64)) for v in (p, q, n))
    R = [pd[:, 1] * nd[:, 2] + pd[:, 2] * nd[:, 1], pd[:, 2] * nd[:, 0] + pd[:, 0] * nd[:, 2], pd[:, 0] * nd[:, 1] + pd[:, 1] * nd[:, 0],
         nd[:, 0], nd[:, 1], nd[:, 2]]
    rbar = ((qd + pd) * nd).sum(1)
    major = [float((R[a] * R[b]).sum()) for a in range(6) for b in range(a, 6)] + [float((R[a] * rbar).sum()) for a in range(6)]
    major.append(float((rbar * rbar).sum()))
    return exact, np.array(major)


def checker(src, tgt, T, max_dist, normals):
    idx, d2 = rc.pairs(src, tgt, T)
    valid = idx >= 0
    inl = valid & (d2 <= rc.maxd2_of(max_dist))
    d2_sum = math.fsum(d2[inl].astype(np.float64).tolist())
    if not inl.any():
        return PlaneCheck(int(valid.sum()), 0, 0, [Fraction(0)] * 28, np.zeros(28), d2_sum)
    normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    assert len(normals) == len(tgt)
    moved = oi.transform(np.ascontiguousarray(src, np.float32), T)[:, :3]
    j = idx[inl]
    n = normals[j]
    planar = (n != 0).any(1)
    exact, major = plane_sums(moved[inl][planar], np.ascontiguousarray(tgt, np.float32)[j, :3][planar], n[planar])
    return PlaneCheck(int(valid.sum()), int(inl.sum()), int(planar.sum()), exact, major, d2_sum)


def within_bound(got, chk):
    """per sum 0 .. 27: (|got - exact|, bound) as Fractions, bound = (n_planar + 10) * 2^-53 * major"""
    out = []
    for k in range(28):
        err = abs(Fraction(float(got[k])) - chk.exact[k])
        out.append((err, Fraction(chk.n_planar + 10, 1 << 53) * Fraction(float(chk.major[k]))))
    return out


def neighbour_d2(tgt, rows):
    """float64 squared distances from points `rows` of a cloud to all of its points"""
    x = np.ascontiguousarray(tgt, np.float32)[:, :3].astype(np.float64)
    d = x[None, :, :] - x[rows, None, :]
    return (d * d).sum(2), d


def cpu_normals(tgt, radius):
    """icpo_normals, except where its grid of radius-sized cells would not fit in memory: there the cloud must have no two points
    within the radius (checked), and every normal is zero"""
    tgt = np.ascontiguousarray(tgt, np.float32)
    if len(tgt) == 0:
        return np.zeros((0, 3), np.float32)
    ext = (tgt[:, :3].max(0).astype(np.float64) - tgt[:, :3].min(0)) / radius + 1
    if np.prod(ext) <= 5e7:
        return oi.normals(tgt, radius)
    for r0 in range(0, len(tgt), 256):
        d2, _ = neighbour_d2(tgt, np.arange(r0, min(r0 + 256, len(tgt))))
        assert ((d2 <= radius * radius).sum(1) == 1).all()
    return np.zeros((len(tgt), 3), np.float32)


_NORMALS = {}


def cpu_normals_once(tgt, radius):
    """cpu_normals, computed once per cloud object (the cases share their targets) and radius"""
    key = (id(tgt), radius)
    if key not in _NORMALS:
        _NORMALS[key] = (tgt, cpu_normals(tgt, radius))           # (the cloud is kept: its id stays its own)
    return _NORMALS[key][1]


@functools.lru_cache(maxsize=None)
def checked(name):
    """the checker's answer, on icpo_normals, for every candidate of a named case, computed once"""
    src, tgts, Ts, max_dist, radius = case(name)
    return [checker(src, t, T, max_dist, cpu_normals_once(t, radius)) for t, T in zip(tgts, Ts)]


def information_plane(sums):
    """scl_registration_information_plane restated: (the symmetric 6 x 6 of the triangle, sum J r)"""
    info = np.zeros((6, 6), np.float64)
    info[np.triu_indices(6)] = np.asarray(sums, np.float64)[:21]
    info.T[np.triu_indices(6)] = np.asarray(sums, np.float64)[:21]
    return info, np.asarray(sums, np.float64)[21:27].copy()
