"""The checker of the marginal covariances (tests/pgo_marginal_cases.py) held to itself, without a GPU: the numpy restatement against
the 40-digit one on the small cases (TAU_MARG and TAU_REL measured again and compared with the pin), against the answers derived by
hand on exact chains of 3 and 4 poses with the matrices written out, every joint covariance positive definite, rel(i, i) zero."""
import numpy as np
import pytest

import pcm_cases as pc
import pgo_cases as pg
import pgo_marginal_cases as mc


def test_the_pins_are_what_the_restatement_measures():
    worst_m = worst_r = 0.0
    for name in mc.SMALL_CASES:
        dm, dr = mc.restatement_deviations(name)
        print(f"{name}: blocks {dm:.3e} rel {dr:.3e}")
        worst_m, worst_r = max(worst_m, dm), max(worst_r, dr)
    print(f"largest: blocks {worst_m:.3e} (pinned {mc.MEASURED_MARG:.0e}) rel {worst_r:.3e} (pinned {mc.MEASURED_REL:.0e})")
    # the pin is the measurement rounded up to one digit: never below it, never more than the rounding above it
    assert worst_m <= mc.MEASURED_MARG <= 4 * worst_m
    assert worst_r <= mc.MEASURED_REL <= 4 * worst_r
    assert mc.TAU_MARG == 16 * mc.MEASURED_MARG and mc.TAU_REL == 16 * mc.MEASURED_REL


@pytest.mark.parametrize("n", [3, 4])
def test_known_answers_on_exact_chains_written_out(n):
    g = mc.exact_chain(n)
    lin = pg.linearize_numpy(g)
    assert lin.chi2.max() < 1e-24                           # the measurements are exact: every D(E) = I up to that
    S, X = mc.sigma_numpy(lin), pc._normalised(g.poses)
    cov = pc._sym(g.f_cov)
    # Sigma[0, 0] = p_cov
    want = np.diag([1e-6] * 3 + [1e-4] * 3)
    assert (mc.known_prior_block(g) == want).all()
    assert mc.dev_block(mc.block(S, 0, 0), want, S, 0, 0) <= mc.TAU_MARG
    # rel(k, k + 1) = f_cov[k]
    for k in range(n - 1):
        d = mc.dev_rel(mc.rel_numpy(S, X, k, k + 1), cov[k])
        print(f"chain{n} rel({k}, {k + 1}): {d:.3e}")
        assert d <= mc.TAU_REL
    # rel(0, 2) = Ad(z_1^-1) f_cov[0] Ad(z_1^-1)^T + f_cov[1], Ad(R, t) = [[R, 0], [[t]x R, R]] written out
    z = pc.inverse(pc._normalised(g.f_z[1:2]))[0]
    R, t = pc.qmat(z[3:]), z[:3]
    K = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])
    A = np.block([[R, np.zeros((3, 3))], [K @ R, R]])
    want = A @ cov[0] @ A.T + cov[1]
    assert np.allclose(want, mc.known_rel_02(g), rtol=1e-14, atol=0)
    assert mc.dev_rel(mc.rel_numpy(S, X, 0, 2), want) <= mc.TAU_REL
    # and the second pose's marginal is the prior carried along the first step plus that step's own covariance
    z0 = pc.inverse(pc._normalised(g.f_z[0:1]))
    A0 = pc.adjoint(z0)[0]
    want11 = A0 @ np.diag([1e-6] * 3 + [1e-4] * 3) @ A0.T + cov[0]
    assert mc.dev_block(mc.block(S, 1, 1), want11, S, 1, 1) <= mc.TAU_MARG


def test_every_joint_covariance_of_the_restatement_is_positive_definite():
    for name in mc.SMALL_CASES:
        S, X = mc.small_numpy(name)
        n = len(X)
        for i in range(n):
            for j in range(i + 1, n):
                idx = np.r_[6 * i:6 * i + 6, 6 * j:6 * j + 6]
                J = S[np.ix_(idx, idx)]
                d = np.sqrt(np.diag(J))
                assert np.linalg.eigvalsh(J / np.outer(d, d)).min() > 0, (name, i, j)
                assert np.linalg.eigvalsh(mc.rel_numpy(S, X, i, j)).min() > 0, (name, i, j)


def test_rel_of_a_pose_with_itself_is_zero():
    for name in mc.SMALL_CASES:
        S, X = mc.small_numpy(name)
        _, rel_e = mc.small_exact(name)
        for i in range(len(X)):
            assert (mc.rel_numpy(S, X, i, i) == 0).all() and (rel_e[i, i] == 0).all()


def test_the_cut_of_the_two_robot_graph():
    g = mc.two_robots_cut()
    assert len(g.poses) == 16 and len(g.f_i) == 15 and pg.components_ok(16, g.f_i, g.f_j, g.p_idx)
    assert (3, 11) in set(zip(g.f_i.tolist(), g.f_j.tolist()))
