"""tests/registration_plane_cases.py pinned without a GPU: the checker on answers written by hand and against plain Fraction
arithmetic, every named input but the lattice off the inlier knife edge, no pair of target points on the edge of a normal's ball,
the checker's own normals within the eigen-residual bound the GPU test holds the device's to, and the corridor degenerate along x."""
from fractions import Fraction

import numpy as np
import pytest

import registration_eval_cases as rc
import registration_plane_cases as pc
from scl_slam_amd.synth import rigid_transform

IDENT = np.eye(4, dtype=np.float32)
TRI = (0, 6, 11, 15, 18, 20)                                   # where the diagonal sits in the upper triangle, row by row


def test_three_points_on_a_known_plane():
    """sources at height 0.25 over the plane z = 0, normal (0, 0, 1): J = (y, -x, 0, 0, 0, 1), r = -0.25"""
    tgt = np.float32([[1, 0, 0], [0, 2, 0], [3, 4, 0]])
    src = tgt + np.float32([0, 0, 0.25])
    nrm = np.float32([[0, 0, 1]] * 3)
    c = pc.checker(src, tgt, IDENT, 1.0, nrm)
    assert (c.n_valid, c.n_inliers, c.n_planar) == (3, 3, 3) and c.d2_sum == 3 * 0.0625
    info, grad = pc.information_plane([float(v) for v in c.exact] + [c.d2_sum])
    want = np.zeros((6, 6))
    want[0, 0] = 0 + 4 + 16; want[1, 1] = 1 + 0 + 9; want[0, 1] = want[1, 0] = -(0 + 0 + 12)      # sum yy, sum xx, -sum xy
    want[0, 5] = want[5, 0] = 0 + 2 + 4; want[1, 5] = want[5, 1] = -(1 + 0 + 3); want[5, 5] = 3
    assert np.array_equal(info, want)
    assert grad.tolist() == [-0.25 * 6, 0.25 * 4, 0, 0, 0, -0.75] and c.exact[27] == Fraction(3, 16)
    # the majorants: |y|, |x|, 0, 0, 0, 1 and rbar = (|q_z| + |p_z|) |n_z| = 0.25
    assert c.major[0] == 20 and c.major[6] == 10 and c.major[1] == 12 and c.major[20] == 3 and c.major[27] == 3 * 0.0625
    assert c.major[21] == 0.25 * 6 and c.major[22] == 0.25 * 4 and c.major[26] == 0.75


def test_a_point_with_a_zero_normal_counts_as_an_inlier_only():
    tgt = np.float32([[1, 0, 0], [0, 2, 0], [3, 4, 0]])
    src = tgt + np.float32([0, 0, 0.25])
    nrm = np.float32([[0, 0, 1], [0, 0, 0], [0, 0, -1]])          # (the sign of a normal changes no sum)
    c = pc.checker(src, tgt, IDENT, 1.0, nrm)
    assert (c.n_valid, c.n_inliers, c.n_planar) == (3, 3, 2) and c.d2_sum == 3 * 0.0625
    assert [c.exact[k] for k in TRI] == [0 + 16, 1 + 9, 0, 0, 0, 2] and c.exact[27] == Fraction(2, 16)
    assert [float(v) for v in c.exact[21:27]] == [-0.25 * 4, 0.25 * 4, 0, 0, 0, -0.5]
    none = pc.checker(src, tgt, IDENT, 1.0, np.zeros((3, 3), np.float32))
    assert (none.n_inliers, none.n_planar) == (3, 0) and not any(none.exact) and not none.major.any() and none.d2_sum == 3 * 0.0625
    empty = pc.checker(src, tgt[:0], IDENT, 1.0, np.zeros((0, 3), np.float32))
    assert (empty.n_valid, empty.n_inliers, empty.n_planar, empty.d2_sum) == (0, 0, 0, 0.0)


def test_the_integer_sums_are_fraction_arithmetic():
    rs = np.random.RandomState(5)
    p = (rs.standard_normal((40, 3)) * 10.0 ** rs.randint(-3, 3, (40, 3))).astype(np.float32)
    q = (p + 0.01 * rs.standard_normal((40, 3))).astype(np.float32)
    n = rs.standard_normal((40, 3)); n = (n / np.linalg.norm(n, axis=1)[:, None]).astype(np.float32)
    exact, major = pc.plane_sums(p, q, n)
    want = [Fraction(0)] * 28
    for k in range(40):
        P, Q, N = ([Fraction(float(v)) for v in a[k]] for a in (p, q, n))
        J = [P[1] * N[2] - P[2] * N[1], P[2] * N[0] - P[0] * N[2], P[0] * N[1] - P[1] * N[0], N[0], N[1], N[2]]
        r = sum((Q[a] - P[a]) * N[a] for a in range(3))
        terms = [J[a] * J[b] for a in range(6) for b in range(a, 6)] + [J[a] * r for a in range(6)] + [r * r]
        want = [w + t for w, t in zip(want, terms)]
    assert exact == want
    assert all(abs(e) <= Fraction(float(m)) * (1 + Fraction(1, 2 ** 40)) for e, m in zip(exact, major))    # a majorant is one
    got = np.array([float(e) for e in exact])
    assert all(err <= bound for err, bound in pc.within_bound(got, pc.PlaneCheck(40, 40, 40, exact, major, 0.0)))
    off = got.copy(); off[3] += 1e-9 * major[3]
    assert not all(err <= bound for err, bound in pc.within_bound(off, pc.PlaneCheck(40, 40, 40, exact, major, 0.0)))


def test_information_plane_is_the_mirrored_triangle():
    S = np.arange(29, dtype=np.float64) + 1
    info, grad = pc.information_plane(S)
    assert np.array_equal(info, info.T) and info[0].tolist() == [1, 2, 3, 4, 5, 6] and info[1, 1:].tolist() == [7, 8, 9, 10, 11]
    assert np.diag(info).tolist() == [S[k] for k in TRI] and info[4, 5] == 20 and grad.tolist() == [22, 23, 24, 25, 26, 27]


def test_the_cases_cover_what_they_name():
    for name in pc.CASES:
        src, tgts, Ts, max_dist, radius = pc.case(name)
        assert len(tgts) == len(Ts) and Ts.dtype == np.float32 and np.isfinite(Ts[:, :3]).all() and radius > 0, name
    res = pc.checked("list")
    assert [r.n_valid for r in res] == [1500, 1500, 1500, 0, 1500]
    assert all(0 < r.n_planar <= r.n_inliers < 1500 for r in res[:3] + res[4:]) and res[3].n_inliers == 0
    assert [len(pc.case(n)[1]) for n in ("n1", "n32", "n33")] == [1, 32, 33]
    assert [len(pc.case(f"src_{n}")[0]) for n in pc.SIZES + pc.SIZES_ONE] == list(pc.SIZES + pc.SIZES_ONE)
    assert [len(pc.case(f"src_{n}")[1]) for n in pc.SIZES_ONE] == [1, 1]
    nrm = pc.cpu_normals_once(pc.place(), pc.RADIUS)
    assert int((~(nrm != 0).any(1)).sum()) == 3                                  # the place has three points without a normal
    sp = pc.checked("sparse")[0]
    assert sp.n_inliers - sp.n_planar >= 40                                      # the isolated points are matched and have no plane
    for r in pc.checked("tiny_radius"):
        assert r.n_inliers > 1000 and r.n_planar == 0 and not any(r.exact) and r.d2_sum > 0
    for r in pc.checked("huge_radius"):
        assert r.n_planar == r.n_inliers > 1000
    for name in ("tgt1", "tgt2"):
        assert all(r.n_valid == 1500 and r.n_inliers >= 1 and r.n_planar == 0 for r in pc.checked(name))
    assert [r.n_valid for r in pc.checked("nan")] == [1496, 1496, 1496, 0, 1496]
    assert all(r.n_valid == 1498 and r.n_planar > 0 for r in pc.checked("overflow"))
    assert all(r.n_inliers == 0 for r in pc.checked("maxd0"))
    assert all(r.n_valid == r.n_inliers for r in pc.checked("all")) and pc.checked("all")[0].n_planar == 1499
    for r in pc.checked(pc.LATTICE):
        assert (r.n_valid, r.n_inliers, r.n_planar, r.d2_sum) == (500, 500, 500, 125.0)


@pytest.mark.parametrize("name", [n for n in pc.CASES if n != pc.LATTICE])
def test_off_the_knife_edge(name):
    """copies with half of the coordinates of the source and of every target moved one ulp give the same counts"""
    src, tgts, Ts, max_dist, _ = pc.case(name)
    want = [(r.n_valid, r.n_inliers) for r in pc.checked(name)]
    made = {}
    got = []
    for t, T in zip(tgts, Ts):
        if id(t) not in made:
            made[id(t)] = rc.jittered(t, 100 + len(made))
        got.append(rc.checker(rc.jittered(src, 7), made[id(t)], T, max_dist)[:2])
    assert got == want


def test_the_lattice_is_on_the_edge():
    src, tgts, Ts, max_dist, _ = pc.case(pc.LATTICE)
    idx, d2 = rc.pairs(src, tgts[0], Ts[0])
    assert (d2 == rc.maxd2_of(max_dist)).all() and (idx >= 0).all()


@pytest.mark.parametrize("name", ["list", "sparse", "tiny_radius", "huge_radius", "tgt1", "tgt2", pc.LATTICE, "corridor"])
def test_no_pair_of_target_points_is_on_the_edge_of_a_ball(name):
    """|d^2 - r^2| >= 1e-9 r^2 for every pair of points of every target (the other cases use the list's targets and radius): which
    points a normal is made of does not hang on a rounding"""
    radius = pc.case(name)[4]
    r2 = radius * radius
    for t in pc.distinct_targets(name):
        closest = np.inf
        for r0 in range(0, len(t), 500):
            d2, _ = pc.neighbour_d2(t, np.arange(r0, min(r0 + 500, len(t))))
            closest = min(closest, float(np.abs(d2 - r2).min()))
        assert closest >= 1e-9 * r2, (name, closest / r2)


def eigen_residuals(tgt, radius, normals):
    """per point with a normal: (| |n| - 1 |, ||C n - l_min n|| / l_max) with C the float64 covariance of the points within the radius,
    by brute force; and the set of points with fewer than three of them"""
    tgt = np.ascontiguousarray(tgt, np.float32)
    nrm = np.asarray(normals, np.float32).astype(np.float64)
    few = np.zeros(len(tgt), bool); unit = np.zeros(len(tgt)); res = np.zeros(len(tgt))
    for r0 in range(0, len(tgt), 256):
        rows = np.arange(r0, min(r0 + 256, len(tgt)))
        d2, d = pc.neighbour_d2(tgt, rows)
        w = (d2 <= radius * radius).astype(np.float64)
        cnt = w.sum(1)
        few[rows] = cnt < 3
        mean = (w[:, :, None] * d).sum(1) / cnt[:, None]
        c = d - mean[:, None, :]
        C = np.einsum("ij,ija,ijb->iab", w, c, c) / cnt[:, None, None]
        lam = np.linalg.eigvalsh(C)
        n = nrm[rows]
        resid = np.einsum("iab,ib->ia", C, n) - lam[:, :1] * n
        res[rows] = np.linalg.norm(resid, axis=1) / np.maximum(lam[:, 2], 1e-300)
        unit[rows] = np.abs(np.linalg.norm(n, axis=1) - 1.0)
    return few, unit, res


@pytest.mark.parametrize("radius", [1.0, 0.5])
def test_the_checkers_normals_meet_the_eigen_residual_bound(radius):
    tgt = pc.place()
    nrm = pc.cpu_normals_once(tgt, radius)
    few, unit, res = eigen_residuals(tgt, radius, nrm)
    zero = ~(nrm != 0).any(1)
    assert np.array_equal(zero, few)
    print(f"radius {radius}: {int(few.sum())} without a normal, worst | |n| - 1 | {unit[~few].max() * 2 ** 23:.3f} x 2^-23, "
          f"worst residual {res[~few].max() * 2 ** 23:.3f} x 2^-23 l_max")
    assert (unit[~few] <= 2.0 ** -23).all() and (res[~few] <= 2.0 ** -23).all()


def test_the_corridor_does_not_constrain_the_motion_along_x():
    for r in pc.checked("corridor"):
        info, _ = pc.information_plane([float(v) for v in r.exact] + [r.d2_sum])
        lam, vec = np.linalg.eigh(info)
        assert 0 <= lam[0] < 1e-3 * lam[5] and abs(vec[3, 0]) > 0.99
        # the point-to-point matrix of the same pairs: m * I3 in its translation block, whatever the scene
        assert np.array_equal(rc.information(r.n_inliers, np.zeros(10))[3:, 3:], r.n_inliers * np.eye(3))
