"""tests/registration_eval_cases.py pinned without a GPU: the checker on answers written by hand, and every named input of the GPU
tests shown to be off the inlier knife edge (the one lattice case, which is meant to sit on it, excepted)."""
import numpy as np
import pytest

import registration_eval_cases as rc
from scl_slam_amd.synth import rigid_transform

THREE = np.float32([[1, 0, 0], [0, 2, 0], [0, 0, 3]])
IDENT = np.eye(4, dtype=np.float32)
SHIFT = rigid_transform(0, 0, 0, 0.5, 0, 0).astype(np.float32)


def test_three_points_under_the_identity():
    nv, m, S, A = rc.checker(THREE, THREE, IDENT, 1.0)
    assert (nv, m) == (3, 3)
    assert S.tolist() == [1, 2, 3, 1, 4, 9, 0, 0, 0, 0] and A.tolist() == S.tolist()
    info = rc.information(m, S)
    assert np.diag(info).tolist() == [13, 10, 5, 3, 3, 3]
    want = np.diag([13.0, 10, 5, 3, 3, 3])
    for (r, c), v in {(0, 4): -3, (0, 5): 2, (1, 3): 3, (1, 5): -1, (2, 3): -2, (2, 4): 1}.items():
        want[r, c] = want[c, r] = v
    assert np.array_equal(info, want) and np.array_equal(info, info.T)


def test_equality_is_kept_and_the_next_float_below_is_not():
    nv, m, S, _ = rc.checker(THREE, THREE, SHIFT, 0.5)
    assert (nv, m) == (3, 3) and S[9] == 0.75 and S[:3].tolist() == [1, 2, 3]       # the sums are the TARGET points'
    below = float(np.nextafter(np.float32(0.5), np.float32(0)))
    nv, m, S, _ = rc.checker(THREE, THREE, SHIFT, below)
    assert (nv, m) == (3, 0) and not S.any()
    assert rc.maxd2_of(0.5) == np.float32(0.25) and rc.maxd2_of(below) < np.float32(0.25) and np.isinf(rc.maxd2_of(1e30))


def test_a_nan_source_point_is_neither_valid_nor_an_inlier():
    src = np.vstack([THREE, [[np.nan, 0, 0]], [[0, 0, np.inf]]]).astype(np.float32)
    nv, m, S, _ = rc.checker(src, THREE, IDENT, 1e30)
    assert (nv, m) == (3, 3) and S.tolist() == [1, 2, 3, 1, 4, 9, 0, 0, 0, 0]
    assert rc.checker(THREE[:0], THREE, IDENT, 1.0)[:2] == (0, 0) and rc.checker(THREE, THREE[:0], IDENT, 1.0)[:2] == (0, 0)


def test_the_cases_cover_what_they_name():
    for name in rc.CASES:
        src, tgts, Ts, max_dist = rc.case(name)
        assert len(tgts) == len(Ts) and Ts.dtype == np.float32 and np.isfinite(Ts[:, :3]).all(), name
    res = rc.checked("list")
    assert [r[0] for r in res] == [1500, 1500, 1500, 0, 1500]
    assert all(0 < r[1] < 1500 for r in res[:3]) and res[3][1] == 0 and 0 <= res[4][1] < res[0][1]      # the distances straddle max_dist
    assert [len(rc.case(n)[1]) for n in ("n1", "n32", "n33")] == [1, 32, 33]
    assert [len(rc.case(f"src_{n}")[0]) for n in rc.SIZES] == list(rc.SIZES)
    src, tgts, Ts, _ = rc.case("overflow")
    assert np.isfinite(src[:, :3]).all()
    for (nv, _, _, _), T in zip(rc.checked("overflow"), Ts):
        moved = rc.oi.transform(src, T)
        assert int((~np.isfinite(moved[:, :3]).all(1)).sum()) == 2 and nv == 1498
    assert [r[0] for r in rc.checked("nan")] == [1496, 1496, 1496, 0, 1496]
    assert all(r[0] in (0, 1500) and r[1] == 0 for r in rc.checked("maxd0"))
    assert all(r[0] == r[1] for r in rc.checked("all")) and rc.checked("all")[0][1] == 1500
    for nv, m, S, _ in rc.checked(rc.LATTICE):                        # every distance exactly on the edge, and kept
        assert (nv, m) == (500, 500) and S[9] == 125.0


@pytest.mark.parametrize("name", [n for n in rc.CASES if n != rc.LATTICE])
def test_off_the_knife_edge(name):
    """copies with half of the coordinates of the source and of every target moved one ulp give the same counts"""
    src, tgts, Ts, max_dist = rc.case(name)
    want = [(r[0], r[1]) for r in rc.checked(name)]
    made = {}
    got = []
    for c, (t, T) in enumerate(zip(tgts, Ts)):
        if id(t) not in made:
            made[id(t)] = rc.jittered(t, 100 + len(made))
        got.append(rc.checker(rc.jittered(src, 7), made[id(t)], T, max_dist)[:2])
    assert got == want


def test_the_lattice_is_on_the_edge():
    src, tgts, Ts, max_dist = rc.case(rc.LATTICE)
    idx, d2 = rc.pairs(src, tgts[0], Ts[0])
    assert (d2 == rc.maxd2_of(max_dist)).all() and (idx >= 0).all()
    assert rc.checker(src, tgts[0], Ts[0], float(np.nextafter(np.float32(max_dist), np.float32(0))))[:2] == (500, 0)
