"""The checker of the condensed direct step (tests/pgo_condensed_cases.py) without a GPU: held to answers written out by hand on
chains of 3 and 4 poses, to scipy's sparse direct solve on pgo_cases.hessian, and its own backward error measured over every step case
-- the measurement TAU_STEP is 16 times of."""
import numpy as np
import pytest

import pgo_cases as pg
import pgo_condensed_cases as cc


@pytest.mark.parametrize("n", (3, 4))
def test_hand_written_chains(n):
    g, junctions, segments, S_of = cc.hand_case(n)
    lin = pg.linearize_numpy(g)
    assert cc.classify(n, g.f_i, g.f_j, g.p_idx) == (junctions, segments)
    for lam in cc.LAMBDAS:
        J, segs, S, rhs, back = cc.condensed_system(lin, lam)
        want = S_of(lin, lam)
        assert (J, segs) == (junctions, segments) and S.shape == (12, 12)
        # both are sums of a few products of the same blocks: within rounding of the largest of them
        scale = np.abs(pg.hessian(lin, lam).toarray()).max()
        assert np.abs(S - want).max() <= 1e-10 * scale and np.abs(S - S.T).max() <= 1e-10 * scale


def test_the_level_order_of_short_paths():
    assert cc.path_levels(2) == []
    assert cc.path_levels(3) == [[(1, 0, 2)]]
    assert cc.path_levels(4) == [[(1, 0, 2)], [(2, 0, 3)]]
    assert cc.path_levels(5) == [[(1, 0, 2), (3, 2, 4)], [(2, 0, 4)]]
    assert cc.path_levels(6) == [[(1, 0, 2), (3, 2, 4)], [(2, 0, 4)], [(4, 0, 5)]]
    assert len(cc.path_levels(4097)) == 12 and len(cc.path_levels(100000)) == 17
    for m in (7, 64, 65, 66, 257):                                              # every node between the ends goes exactly once
        gone = [node for level in cc.path_levels(m) for node, _, _ in level]
        assert sorted(gone) == list(range(1, m - 1))


def test_the_rule_on_the_named_graphs():
    for name, want in cc.COUNTS.items():
        g = cc.step_case(name)
        J, segs = cc.classify(len(g.poses), g.f_i, g.f_j, g.p_idx)
        got = (len(J), len(segs), max([b - a + 1 for a, b in segs], default=0))
        assert all(w is None or w == v for w, v in zip(want, got)), (name, got, want)
    for L in cc.SEGMENT_LENGTHS:
        g = cc.step_case(f"segment{L}")
        assert cc.classify(L + 2, g.f_i, g.f_j, g.p_idx) == ([0, L + 1], [(1, L)])
    g = cc.many_junctions()
    assert len(cc.classify(len(g.poses), g.f_i, g.f_j, g.p_idx)[0]) == cc.MAX_JUNCTIONS + 1


def test_backward_error_of_the_checker_is_what_tau_step_was_measured_from():
    worst = 0.0
    for name in cc.STEP_CASES:
        lin = cc.step_lin(name)
        for lam in cc.LAMBDAS:
            d = cc.solve_condensed(lin, lam)
            be = cc.backward_error(lin, lam, d)
            print(f"{name:14s} lambda {lam:g}: backward error {be:.3g}")
            worst = max(worst, be)
    print("largest", worst, "MEASURED", cc.MEASURED, "TAU_STEP", cc.TAU_STEP)
    assert worst <= cc.MEASURED == cc.TAU_STEP / 16


@pytest.mark.parametrize("name", [n for n in cc.STEP_CASES if n not in ("chain4097", "drifting4097")])
def test_against_scipys_direct_solve(name):
    """at lambda = 10 the damped matrix is well conditioned (block-diagonally dominant), so two backward stable solves agree closely"""
    lin = cc.step_lin(name)
    d = cc.solve_condensed(lin, 10.0).ravel()
    want = pg.spla.spsolve(pg.hessian(lin, 10.0).tocsc(), -lin.grad.ravel())
    assert np.abs(d - want).max() <= 1e-9 * np.abs(want).max()


def test_the_scipy_loop_stops_on_the_cost_on_the_optimiser_tests_graphs():
    """what test_gpu_pgo_condensed.py asks of the device on drifting_graph(1000), first of the checker: the stop and the cost"""
    _, info = pg.lm_numpy(pg.drifting_graph(1000), pg.DEFAULTS)
    print(info["iterations"], info["final_cost"])
    assert info["stop_reason"] == pg.STOP_COST and info["iterations"] < pg.DEFAULTS["max_iterations"]
    assert abs(info["final_cost"] - 96.4933) <= 1e-4
    _, own = cc.lm_condensed(pg.drifting_graph(1000), pg.DEFAULTS)
    assert own["stop_reason"] == pg.STOP_COST and abs(own["final_cost"] - info["final_cost"]) <= 1e-8 * info["final_cost"]
    for g, params in ((pg.ring16(), pg.TIGHT), pg.rejected_case()):
        _, a = pg.lm_numpy(g, params)
        _, b = cc.lm_condensed(g, params)
        assert (a["iterations"], a["accepted"], a["rejected"]) == (b["iterations"], b["accepted"], b["rejected"])
