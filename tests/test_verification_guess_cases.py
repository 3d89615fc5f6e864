"""The guessed candidate list of tests/verification_guess_cases.py pinned on the CPU checker (oracle/icp_oracle.c): per candidate
one icpo_geometric_verification of the scan's finite rows moved by the candidate's guess (oi.transform, DM.h:247-249).  It shows
what the initial guess is for -- the yawed candidates fail as they are and verify once the scan is turned by their yaw -- and that
the list tells candidates and guesses apart, so that "guessed batch == single calls == checker" in
tests/test_gpu_verification_guess.py cannot hold by accident.  No GPU needed."""
import functools

import numpy as np
import pytest

import oracle_icp_binding as oi
import verification_guess_cases as gc

IDENT = np.eye(4, dtype=np.float32)
ALL = 2000 - gc.N_NONFINITE


@functools.lru_cache(maxsize=None)
def moved_sources():
    """the finite rows moved by every candidate's guess, once (the GPU tests share them through checker())"""
    src = gc.finite_source()
    return tuple(oi.transform(src, g) for g in gc.guesses())


@functools.lru_cache(maxsize=None)
def checker(iterations, threshold=gc.THRESHOLD, ratio=gc.RATIO, seed=gc.SEED):
    """[(T_fit, success, n_corr, n_inliers)] per candidate with its guess"""
    return [oi.geometric_verification(s, c, iterations, threshold, ratio, seed) for s, c in zip(moved_sources(), gc.clouds())]


@functools.lru_cache(maxsize=None)
def plain(iterations):
    """the same candidates without a guess"""
    src = gc.finite_source()
    return [oi.geometric_verification(src, c, iterations, gc.THRESHOLD, gc.RATIO, gc.SEED) for c in gc.clouds()]


def test_the_list_and_its_guesses():
    names = gc.names()
    assert names[:-1] == gc.bc.names() and names[-1] == "moved_6dof" and len(names) == 14
    G = gc.guesses()
    assert G.shape == (14, 4, 4) and G.dtype == np.float32 and np.isfinite(G).all()
    g = dict(zip(names, G))
    assert np.array_equal(g["matching"], IDENT) and np.array_equal(g["permuted"], IDENT)
    assert not np.array_equal(g["matching_again"], g["matching"])
    assert np.array_equal(gc.clouds()[names.index("matching_again")], gc.clouds()[names.index("matching")])
    for n, deg in (("yaw_3", 3.0), ("yaw_20", 20.0), ("yaw_90", 90.0), ("matching_again", 17.0)):
        c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
        assert np.allclose(g[n], [[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], atol=1e-7)
    m = g["moved_6dof"]                                               # roll, pitch and metres of translation: all six degrees
    assert abs(m[2, 1]) > 0.01 and abs(m[2, 0]) > 0.01 and abs(m[1, 0]) > 0.1 and (np.abs(m[:3, 3]) > 1.0).all()
    assert not np.array_equal(g["empty"][3], [0, 0, 0, 1])            # a last row the calls must not read
    assert len({x.tobytes() for x in G}) >= 10


@pytest.mark.parametrize("iterations", [9, 300])
def test_the_yawed_candidates_need_their_guess(iterations):
    res, raw = dict(zip(gc.names(), checker(iterations))), dict(zip(gc.names(), plain(iterations)))
    for n in gc.names():
        print(iterations, n, "plain", raw[n][1:], "guessed", res[n][1:])
    want = {300: {"yaw_3": 430, "yaw_20": 60, "yaw_90": 94}, 9: {"yaw_3": 84, "yaw_20": 23, "yaw_90": 27}}[iterations]
    for n, inl in want.items():
        assert raw[n][1:] == (False, ALL, inl)
        assert res[n][1:] == (True, ALL, ALL)
    assert raw["moved_6dof"][1] is False and res["moved_6dof"][1:] == (True, ALL, ALL)
    assert res["matching"][1:] == (True, ALL, ALL) and raw["matching_again"][1:] == (True, ALL, ALL)
    assert not res["matching_again"][1] and res["matching_again"][3] < ALL // 4


@pytest.mark.parametrize("iterations", gc.ITERATIONS)
def test_the_list_tells_candidates_apart(iterations):
    res = dict(zip(gc.names(), checker(iterations)))
    for n, r in res.items():
        print(iterations, n, r[1:])
    assert res["matching"][1] and not res["matching_again"][1]
    assert res["empty"][1:] == (False, 0, 0) and np.array_equal(res["empty"][0], IDENT)
    for n, r in res.items():
        if n != "empty":
            assert r[2] == ALL
        if r[3] < 3:
            assert np.array_equal(r[0], IDENT)
    if iterations > 1:
        assert len({r[3] for r in res.values()}) >= 4                 # a batch that mixes up candidates or guesses cannot pass
    else:                                                             # one hypothesis: what the checker shows
        assert len({r[3] for r in res.values()}) >= 3
        assert [res[n][1] for n in ("yaw_3", "yaw_20", "yaw_90", "moved_6dof")] == [True] * 4


def test_the_fit_after_a_right_guess_is_small():
    """a guessed candidate's T_fit is the residual motion, near the identity; the whole motion is T_fit @ G"""
    res = dict(zip(gc.names(), checker(300)))
    for n in ("yaw_3", "yaw_20", "yaw_90", "moved_6dof"):
        assert np.abs(res[n][0] - IDENT).max() < 0.1, n
