"""The checkers of the pose-graph solve (tests/pgo_cases.py) pinned by answers written by hand, without a GPU: what the GPU tests
compare against must itself be right."""
import mpmath
import numpy as np
import pytest

import pcm_cases as pc
import pgo_cases as pg

I6 = np.eye(6).reshape(1, 36)


def test_one_prior_and_one_factor_have_the_minimiser_x0_z_at_cost_zero():
    x0 = pg.pose([1.0, 2.0, -0.5], [0.2, -0.1, 0.9]); z = pg.pose([0.7, -0.3, 0.1], [-0.4, 0.3, 0.2])
    start = np.array([pg.perturb(x0, [0.1, -0.2, 0.1, 0.3, 0.2, -0.4]), pg.pose([3.0, 3.0, 3.0], [0.5, 0.5, -0.5])])
    g = pg.graph(start, [0], [1], z[None], 0.01 * I6, [0], x0[None], 0.01 * I6)
    want = pg.canonical(np.array([x0, pc.compose(x0, z)]))
    X, info = pg.lm_numpy(g, pg.TIGHT)
    assert pg.pose_deviation(X, want) <= 1e-14 and info["final_cost"] <= 1e-26
    Xe, ie = pg.lm_exact(g, pg.EXACT)
    assert pg.pose_deviation(Xe, want) <= 1e-15 and ie["final_cost"] <= 1e-60


def test_two_translation_factors_that_disagree_give_the_mean():
    """two factors of information 1 / s2 between an anchored origin and pose 1, measuring translations a and b and no rotation: the
    minimiser is (a + b) / 2 and the cost 2 * 1/2 * |a - b|^2 / 4 / s2"""
    a, b, s2 = np.array([1.0, 0.0, 0.5]), np.array([1.4, -0.2, 0.3]), 0.04
    ident = pg.pose([0, 0, 0], [0, 0, 0])
    g = pg.graph([ident, pg.pose([5.0, 5.0, 5.0], [0, 0, 0])], [0, 0], [1, 1], [pg.pose(a, [0, 0, 0]), pg.pose(b, [0, 0, 0])], np.tile(s2 * I6, (2, 1)),
                 [0], ident[None], 1e-6 * I6)
    want_cost = ((a - b) ** 2).sum() / 4 / s2
    # the damped step leaves lambda of the distance to the minimiser behind, and the float64 loop stops once the COST no longer moves by
    # 1e-14 of itself -- a distance of 1e-7 of the first one would do that; the 40-digit loop runs to the minimiser
    for (X, info), tol in ((pg.lm_numpy(g, pg.TIGHT), 1e-9), (pg.lm_exact(g, pg.EXACT), 1e-15)):
        assert np.abs(X[1, :3] - (a + b) / 2).max() <= tol and np.abs(X[1, 3:] - [0, 0, 0, 1]).max() <= tol
        assert abs(info["final_cost"] - want_cost) <= 1e-14 * want_cost


def _m_perturbed(P, xi):
    return pg._m_retract([P], [[mpmath.mpf(v) for v in xi]])[0]


def test_jacobians_against_central_differences_at_40_digits():
    """A_i, A_j of _m_factor are L^-1 J; J against (r(X Exp(h e_a)) - r(X Exp(-h e_a))) / 2h with h = 1e-12 at 40 digits: the truncation is
    h^2 = 1e-24.  The retraction R Exp(w), t + R v agrees with Exp on SE(3) to first order, which is all a derivative at 0 sees.  The
    third factor has a residual rotation of 3 rad, the fourth of 0.01 (the series)"""
    rs = np.random.RandomState(5)
    with mpmath.workdps(40):
        for trial, ang in enumerate((0.3, 1.5, 3.0, 0.01)):
            xi, xj = pg.pose(rs.normal(0, 3, 3), rs.normal(0, 1, 3)), pg.pose(rs.normal(0, 3, 3), rs.normal(0, 1, 3))
            axis = rs.standard_normal(3); axis /= np.linalg.norm(axis)
            z = pc.compose(pg.between(xi, xj), np.concatenate([rs.normal(0, 0.2, 3), pc.rotvec_to_quat(ang * axis)]))
            cov = pg.odom_cov(rs)
            S = [[mpmath.mpf(float(v)) for v in row] for row in cov]
            L = mpmath.matrix(pg.m_cholesky(S))
            for prior in (False, True):
                Xi, Xj, Z = (None if prior else pg._m_pose(xi)), pg._m_pose(xj), pg._m_pose(xj if prior else z)
                if prior:
                    Z = _m_perturbed(Z, [0.05 * ang, 0.02, -0.03, 0.1, 0.2, -0.1])
                y, Ai, Aj = pg._m_factor(Xi, Xj, Z, S)
                h = mpmath.mpf(10) ** -12
                for side, A in ((0, Ai), (1, Aj)):
                    if A is None:
                        continue
                    J = L * mpmath.matrix(A)
                    for a in range(6):
                        e = [h if k == a else 0 for k in range(6)]; m = [-v for v in e]
                        plus = pg.m_residual(_m_perturbed(Xi, e) if side == 0 else Xi, _m_perturbed(Xj, e) if side == 1 else Xj, Z)
                        minus = pg.m_residual(_m_perturbed(Xi, m) if side == 0 else Xi, _m_perturbed(Xj, m) if side == 1 else Xj, Z)
                        for k in range(6):
                            assert abs((plus[k] - minus[k]) / (2 * h) - J[k, a]) <= mpmath.mpf(10) ** -18, (trial, prior, side, a, k)


def test_the_series_of_c_meets_the_closed_form_on_both_sides_of_the_switch():
    with mpmath.workdps(40):
        for theta in (mpmath.mpf("0.0499999"), mpmath.mpf("0.0500001"), mpmath.mpf("1e-3"), mpmath.mpf("1e-9")):
            w, nv = mpmath.cos(theta / 2), mpmath.sin(theta / 2)
            closed = pg.m_c_of(theta, w, nv, series_below=0)
            textbook = 1 / theta ** 2 - (1 + mpmath.cos(theta)) / (2 * theta * mpmath.sin(theta))
            assert abs(closed - textbook) <= mpmath.mpf(10) ** -30 / theta ** 2          # the half-angle form IS the contract's c
            assert abs(pg.m_c_of(theta, w, nv) - closed) <= mpmath.mpf(10) ** -18        # the series' next term: theta^8 / 47900160 < 1e-18
        assert pg.m_c_of(mpmath.mpf(0), mpmath.mpf(1), mpmath.mpf(0)) == mpmath.mpf(1) / 12
    th = np.array([0.0499999, 0.0500001, 0.3])
    assert np.allclose(pg._c_of(th, np.cos(th / 2), np.sin(th / 2)), 1 / 12 + th ** 2 / 720 + th ** 4 / 30240 + th ** 6 / 1209600, rtol=1e-9, atol=0)


def test_a_rotation_just_short_of_a_half_turn_takes_the_sign_rule():
    """E a rotation of pi - 1e-9 about z whose quaternion has w < 0: the residual is that of -q, an angle of pi - 1e-9 about +z"""
    ang = np.pi - 1e-9
    q = -np.array([0.0, 0.0, np.sin(ang / 2), np.cos(ang / 2)])
    x = np.concatenate([[0.0, 0.0, 0.0], q])
    ident = pg.pose([0, 0, 0], [0, 0, 0])
    g = pg.graph(x[None], [], [], np.zeros((0, 7)), np.zeros((0, 36)), [0], ident[None], I6)
    for lin in (pg.linearize_numpy(g), pg.linearize_exact(g)):
        assert abs(lin.chi2[0] - ang ** 2) <= 1e-14 * ang ** 2
        assert abs(lin.grad[0, 2] - ang) <= 1e-12 and abs(lin.diag[0, 2, 2] - 1.0) <= 1e-12   # Jr^-1 e_z = e_z


def test_the_restatement_stays_within_a_sixteenth_of_tau_lin():
    for name in pg.LIN_CASES:
        nu = pg.linearize_numpy(pg.lin_case(name))
        d = pg.lin_deviations(nu, pg.lin_exact(name), nu)
        print(name, d)
        assert max(d.values()) <= pg.TAU_LIN_CASE[name] / 16, (name, d)
    assert pg.TAU_LIN == max(pg.TAU_LIN_CASE[n] for n in ("chain5", "one", "two"))


def test_the_scipy_loop_stays_within_a_sixteenth_of_tau_x_of_the_minimiser():
    Xe, ie = pg.ring16_exact()
    X, info = pg.lm_numpy(pg.ring16(), pg.TIGHT)
    dev = pg.pose_deviation(X, Xe)
    print("ring16: deviation", dev, "condition", pg.ring16_condition(), "iterations", info["iterations"], ie["iterations"])
    assert dev <= pg.TAU_X / 16
    lin = pg.linearize_numpy(pg.ring16(), Xe)
    assert (np.abs(ie["lin"].grad) <= 1e-3 * pg.TAU_LIN * lin.grad_m).all()                # lm_exact ran to the minimiser


def test_the_checkers_own_answers_meet_the_gradient_criterion_of_the_optimiser_tests():
    """pgo_cases.py OPT_NOISE: a case on which the contract's loop, run by the checker, leaves a gradient above TAU_LIN decides nothing"""
    for name, g in (("ring16", pg.ring16()), ("two robots", pg.two_robot_graph())):
        X, info = pg.lm_numpy(g, pg.TIGHT)
        lin = info["lin"]
        worst = float((np.abs(lin.grad) / lin.grad_m).max())
        print(name, "gradient / majorant at lm_numpy's answer:", worst, "final cost", info["final_cost"], "iterations", info["iterations"])
        assert worst <= pg.TAU_LIN / 4 and info["stop_reason"] in (pg.STOP_COST, pg.STOP_STEP)


def test_the_rejected_case_rejects_its_first_step_and_still_converges():
    g, params = pg.rejected_case()
    X, info = pg.lm_numpy(g, params)
    lam, ok, cost = info["trace"][0]
    assert not ok and cost > 1.2 * info["initial_cost"]                                   # decided far above rounding
    assert info["rejected"] >= 5 and info["accepted"] >= 3 and info["stop_reason"] in (pg.STOP_COST, pg.STOP_STEP)
    lin = info["lin"]
    assert (np.abs(lin.grad) <= pg.TAU_LIN * lin.grad_m).all()


def test_union_find():
    assert pg.components_ok(4, [0, 1, 2], [1, 2, 3], [2])                                 # one component
    assert not pg.components_ok(4, [0, 2], [1, 3], [0])                                   # two, one prior
    assert pg.components_ok(4, [0, 2], [1, 3], [0, 3])
    assert not pg.components_ok(3, [0], [1], [2])                                         # the prior sits on an isolated pose
    assert pg.components_ok(3, [0], [1], [2, 1]) and pg.components_ok(1, [], [], [0]) and not pg.components_ok(1, [], [], [])
    assert pg.incidence(3, [2, 0, 2], [0, 1, 0], [1]) == ([0, 3, 5, 7], [1, 2, 5, 3, 7, 0, 4])
