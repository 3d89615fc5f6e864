"""The checkers of tests/pcm_cases.py pinned by answers written by hand, the families' properties the GPU tests rely on, and the
tolerance TAU measured and pinned (no GPU)."""
import numpy as np
import pytest

import pcm_cases as pc

IDENT = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])


def _two_loops(z0, z1, cov0, cov1, odom_var=None, idx_a=(0, 2), idx_b=(0, 1)):
    poses = np.tile(IDENT, (3, 1))
    return pc.Case(poses, poses, np.int32(idx_a), np.int32(idx_b), np.array([z0, z1], np.float64),
                   np.array([cov0, cov1], np.float64).reshape(2, 36), odom_var, pc.THRESHOLD, None, None)


def _both(case):
    return pc.d2_exact(case)[0, 1], pc.d2_numpy(case)[0, 1]


def test_a_translation_offset_with_three_steps_of_odometry():
    delta, sigma, v = 0.3, 0.05, 4e-4
    z1 = IDENT.copy(); z1[0] = delta
    c = _two_loops(IDENT, z1, sigma ** 2 * np.eye(6), sigma ** 2 * np.eye(6), odom_var=[v] * 6)      # |0 - 2| + |0 - 1| = 3 steps
    want = delta ** 2 / (2 * sigma ** 2 + 3 * v)
    for got in _both(c):
        assert got == pytest.approx(want, rel=1e-14)
    assert np.array_equal(pc.d2_exact(c), pc.d2_exact(c).T) and pc.d2_exact(c)[0, 0] == 0.0


def test_a_pure_yaw():
    theta, sigma = 0.2, 0.03
    z1 = np.concatenate([[0, 0, 0], pc.rotvec_to_quat([0, 0, theta])])
    for got in _both(_two_loops(IDENT, z1, sigma ** 2 * np.eye(6), sigma ** 2 * np.eye(6))):
        assert got == pytest.approx(theta ** 2 / (2 * sigma ** 2), rel=1e-13)


def test_q_and_minus_q_and_an_unnormalised_q_give_the_same_value():
    rs = np.random.RandomState(5)
    z0 = np.concatenate([rs.standard_normal(3), pc.rotvec_to_quat([0.3, -0.2, 0.5])])
    z1 = np.concatenate([rs.standard_normal(3), pc.rotvec_to_quat([-0.1, 0.4, 2.9])])
    cov = pc.random_cov(rs)
    base = _both(_two_loops(z0, z1, cov, cov))
    for f0, f1 in ((-1.0, 1.0), (1.0, -1.0), (-1.0, -1.0), (2.0, 0.5)):
        a, b = z0.copy(), z1.copy(); a[3:] *= f0; b[3:] *= f1
        got = _both(_two_loops(a, b, cov, cov))
        assert got[0] == pytest.approx(base[0], rel=1e-13) and got[1] == pytest.approx(base[1], rel=1e-11)


def test_a_zero_covariance_gives_infinity_and_no_edge():
    z1 = IDENT.copy(); z1[1] = 0.1
    c = _two_loops(IDENT, z1, np.zeros((6, 6)), np.zeros((6, 6)))
    assert _both(c) == (np.inf, np.inf)
    assert not pc.graph(pc.d2_numpy(c), 1e300).any()
    assert not pc.graph(np.array([[0.0, np.nan], [np.nan, 0.0]]), 1e300).any()
    assert pc.graph(np.array([[0.0, 2.0], [2.0, 0.0]]), 2.0).sum() == 2                           # equality is kept


def test_only_the_upper_triangle_of_a_covariance_is_read():
    z1 = IDENT.copy(); z1[0] = 0.2
    cov = 0.01 * np.eye(6); cov[0, 4] = cov[4, 0] = 0.002
    junk = cov.copy(); junk[np.tril_indices(6, -1)] = 123.0
    assert _both(_two_loops(IDENT, z1, cov, cov)) == _both(_two_loops(IDENT, z1, junk, junk))


@pytest.mark.parametrize("name", sorted(pc.HAND_GRAPHS))
def test_greedy_clique_on_the_graphs_with_written_answers(name):
    n, edges, members, seed = pc.HAND_GRAPHS[name]
    a = pc.graph_from_edges(n, edges)
    assert pc.greedy_clique(a) == (members, seed) and pc.is_clique(a, members)
    if n <= 24:
        assert len(members) <= pc.max_clique_brute(a)
    if name == "greedy_misses":
        assert pc.max_clique_brute(a) == pc.GREEDY_MISSES_EXACT > len(members)
    if name == "equal":
        assert pc.max_clique_brute(a) == 3


def test_greedy_clique_of_no_vertex_and_brute_force_on_a_complete_graph():
    assert pc.greedy_clique(np.zeros((0, 0), bool)) == ((), -1)
    k = ~np.eye(7, dtype=bool)
    assert pc.max_clique_brute(k) == 7 and pc.greedy_clique(k) == (tuple(range(7)), 0)


def test_the_fast_greedy_is_the_greedy():
    for name, (n, edges, members, seed) in pc.HAND_GRAPHS.items():
        assert pc.greedy_clique_fast(pc.graph_from_edges(n, edges)) == (members, seed), name
    assert pc.greedy_clique_fast(np.zeros((0, 0), bool)) == ((), -1)
    rs = np.random.RandomState(21)
    for n, density in [(n, d) for n in (1, 2, 9, 33, 64, 65, 90) for d in (0.0, 0.1, 0.5, 0.9, 1.0)] + [(150, 0.5), (150, 0.95)]:
        a = np.triu(rs.rand(n, n) < density, 1); a = a | a.T
        assert pc.greedy_clique_fast(a) == pc.greedy_clique(a), (n, density)
    c, exact = pc.case_and_d2("mixed", 40)
    g = pc.graph(exact, c.threshold)
    assert pc.greedy_clique_fast(g) == pc.greedy_clique(g)


def test_inliers_drawn_from_their_covariance_have_a_mean_d2_of_six():
    """the covariance model is the right one: d2 of two inliers is chi-square with 6 degrees of freedom (no odometry term)"""
    c, _ = pc.make_case(1.0, 110, seed=77, odom_var=None)
    inl = np.flatnonzero(c.inlier)
    I, J = np.triu_indices(len(inl), 1)
    assert len(I) >= 2000
    d2 = pc.d2_numpy_pairs(c, inl[I[:2000]], inl[J[:2000]])
    print("mean d2 over 2000 inlier pairs:", d2.mean())
    assert 5.5 <= d2.mean() <= 6.5


@pytest.mark.parametrize("family", sorted(pc.FAMILIES))
def test_the_families_are_off_the_knife_edge_and_tau_is_pinned(family):
    worst = 0.0
    for n in pc.SMALL_N:
        c, exact = pc.case_and_d2(family, n)
        assert c.gap >= pc.KNIFE_EDGE
        got = pc.d2_numpy(c)
        assert np.array_equal(np.isinf(got), np.isinf(exact))
        fin = np.isfinite(exact)
        worst = max(worst, float(np.max(np.abs(got - exact)[fin] / np.maximum(1.0, exact[fin]))))
        assert np.array_equal(pc.graph(got, c.threshold), pc.graph(exact, c.threshold))
    print(family, "largest deviation of d2_numpy from d2_exact:", worst, "TAU / 16:", pc.TAU[family] / 16)
    assert worst <= pc.TAU[family] / 16                      # the restatement stays within what TAU was made of
    assert worst >= pc.TAU[family] / 64                      # ... and TAU is not wider than that measurement justifies
    assert pc.TAU[family] <= pc.KNIFE_EDGE * 1e-2            # two decades below the gap: the device's graph is the checker's


def test_planted_inliers_are_the_clique_of_the_checkers_graph():
    for n in pc.SMALL_N:
        c, exact = pc.case_and_d2("planted", n)
        g = pc.graph(exact, c.threshold)
        inl = tuple(np.flatnonzero(c.inlier).tolist())
        assert pc.is_clique(g, inl) and pc.greedy_clique(g)[0] == inl
    c, exact = pc.case_and_d2("mixed", 40)
    g = pc.graph(exact, c.threshold)
    inl = np.flatnonzero(c.inlier)
    assert not pc.is_clique(g, inl)                          # correctly modelled noise: not every pair of inliers passes at 0.75


def test_the_large_mixed_graph_is_off_the_knife_edge():
    c, d2 = pc.case_and_d2("mixed", 1000)
    assert c.gap >= pc.KNIFE_EDGE and len(c.idx_a) == 1000
