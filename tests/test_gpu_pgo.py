"""The pose-graph solve on the GPU (include/scl_engine.h "POSE-GRAPH SOLVE") against the checkers of tests/pgo_cases.py: the
linearisation within TAU_LIN of the 40-digit definition relative to each sum's majorant, the operator within TAU_LIN of the scipy matrix
times x, the optimiser within TAU_X of the 40-digit minimiser (small graphs) or of the scipy loop (larger ones, scaled by the condition
estimates), the gradient at its answer within TAU_LIN of zero; state, errors, two shards."""
from ctypes import POINTER, byref, c_double, c_int

import numpy as np
import pytest

import icp_guess_cases as gc
import pcm_cases as pc
import pgo_cases as pg
from scl_slam_amd import PgoParams, PgoResult, ScanContextEngine, SclError

pytestmark = pytest.mark.gpu
INVALID_ARG = -1
# the optimiser tests: both stop tolerances 1e-14 and CG 1e-12, so that what remains is rounding and not the stopping rule; CG may take as
# many iterations as a chain of a few thousand poses needs
TIGHT = dict(pg.TIGHT, cg_max_iterations=4000)


@pytest.fixture(scope="module")
def eng():
    e = ScanContextEngine(initial_capacity=16)
    yield e
    e.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _lin(e, g):
    cost, grad, diag, chi2 = e.pgo_linearize(*g)
    return pg.Lin(cost=cost, grad=grad, diag=diag, chi2=chi2)


def _opt(e, g, params=None):
    return e.pgo_optimize(*g, params=PgoParams.defaults(**(TIGHT if params is None else params)))


def _gradient_is_zero(g, X, exact):
    """the gradient at X, by the 40-digit checker where the size allows and in float64 otherwise, within TAU_LIN of zero relative to its
    majorant"""
    nu = pg.linearize_numpy(g, X)
    grad = pg.linearize_exact(g, X).grad if exact else nu.grad
    worst = float((np.abs(grad) / nu.grad_m).max())
    print("gradient at the answer / majorant:", worst, "(TAU_LIN", pg.TAU_LIN, ")")
    return worst <= pg.TAU_LIN


# ---- linearise -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", pg.LIN_CASES)
def test_linearisation_against_the_40_digit_checker(eng, name):
    g = pg.lin_case(name)
    got, exact, maj = _lin(eng, g), pg.lin_exact(name), pg.linearize_numpy(g)
    d = pg.lin_deviations(got, exact, maj)
    print(name, "deviations / majorant:", d, "TAU_LIN", pg.TAU_LIN_CASE[name])
    assert max(d.values()) <= pg.TAU_LIN_CASE[name]
    assert np.array_equal(got.diag, np.swapaxes(got.diag, 1, 2))
    cost_only = eng._lib.scl_pgo_linearize                                       # each output alone gives the same bits
    c = c_double(0.0)
    keep, args, n, m = eng._pgo_inputs(*g)
    assert cost_only(eng._h, *args, byref(c), None, None, None) == 0 and c.value == got.cost
    chi2 = np.zeros(m)
    assert cost_only(eng._h, *args, None, None, None, chi2.ctypes.data_as(POINTER(c_double))) == 0 and np.array_equal(_bits(chi2), _bits(got.chi2))


# ---- the operator ----------------------------------------------------------------------------------------------------------------------

def _operator_case(eng, g, lam, columns):
    lin = pg.linearize_numpy(g)
    H, Hm = pg.hessian(lin, lam).tocsc(), pg.hessian_majorant(lin, lam).tocsc()
    n = len(g.poses)
    worst = 0.0
    for col in columns:
        x = np.zeros(6 * n); x[col] = 1.0
        y = eng.pgo_hessian_apply(*g, lam, x).ravel()
        want, maj = H[:, col].toarray().ravel(), Hm[:, col].toarray().ravel()
        assert not y[maj == 0].any()                                              # outside the block row's pattern: exact zeros
        nz = maj > 0
        worst = max(worst, float((np.abs(y[nz] - want[nz]) / maj[nz]).max()))
    rs = np.random.RandomState(n)
    x = rs.standard_normal(6 * n)
    y = eng.pgo_hessian_apply(*g, lam, x).ravel()
    worst = max(worst, float((np.abs(y - H @ x) / (Hm @ np.abs(x))).max()))
    return worst


@pytest.mark.parametrize("lam", (0.0, 10.0))
@pytest.mark.parametrize("n,degree", ((1, 1), (2, 2), (63, 63), (64, 64), (65, 65), (255, 4), (256, 63), (257, 300)))
def test_operator_against_the_scipy_matrix(eng, n, degree, lam):
    """pose 0 has `degree` incident factors: 63 is the last degree one thread sums, 64 the first a wave takes, 300 a long row"""
    g = pg.hub_graph(n, degree)
    ptr, _ = pg.incidence(n, g.f_i, g.f_j, g.p_idx)
    assert ptr[1] - ptr[0] == degree
    rs = np.random.RandomState(n + degree)
    # a unit vector in every block column (all six of the hub's and of the last pose's), and a dozen more
    columns = range(6 * n) if n <= 2 else sorted(set(range(6)) | set(range(6 * n - 6, 6 * n)) | {6 * p + p % 6 for p in range(n)} |
                                                 set(rs.randint(0, 6 * n, 12).tolist()))
    worst = _operator_case(eng, g, lam, columns)
    print("operator deviation / majorant:", worst)
    assert worst <= pg.TAU_LIN


# ---- optimise --------------------------------------------------------------------------------------------------------------------------

def test_ring_of_16_against_the_40_digit_minimiser(eng):
    g = pg.ring16()
    want, _ = pg.ring16_exact()
    X, res, chi2 = _opt(eng, g)
    dev = pg.pose_deviation(X, want)
    print("ring16: deviation", dev, "TAU_X", pg.TAU_X, {k: getattr(res, k) for k, _ in PgoResult._fields_})
    assert dev <= pg.TAU_X
    assert np.abs(np.linalg.norm(X[:, 3:], axis=1) - 1).max() <= 4e-16 and (X[:, 6] >= 0).all()
    assert res.accepted + res.rejected == res.iterations and res.stop_reason in (1, 2, 3, 4) and res.final_cost <= res.initial_cost
    assert abs(0.5 * chi2.sum() - res.final_cost) <= 1e-14 * res.final_cost and len(chi2) == len(g.f_i) + 1
    assert _gradient_is_zero(g, X, exact=True)
    lin = _lin(eng, g._replace(poses=X))                                          # the result's figures are those of a linearisation there
    assert abs(lin.cost - res.final_cost) <= pg.TAU_LIN * pg.linearize_numpy(g, X).cost_m * 2
    assert abs(np.abs(lin.grad).max() - res.gradient_max) <= pg.TAU_LIN * pg.linearize_numpy(g, X).grad_m.max() * 2


def _against_the_scipy_loop(eng, g, exact_gradient):
    want, info = pg.lm_numpy(g, pg.TIGHT)
    X, res, _ = _opt(eng, g)
    cond = pg.condition(info["lin"])
    bound = pg.TAU_X * max(1.0, cond / pg.ring16_condition())
    dev = pg.pose_deviation(X, want)
    print("deviation", dev, "bound", bound, "condition", cond, {k: getattr(res, k) for k, _ in PgoResult._fields_}, "checker iterations", info["iterations"])
    assert dev <= bound
    assert _gradient_is_zero(g, X, exact_gradient)
    return X, res


def test_two_robots_of_32_poses_against_the_scipy_loop(eng):
    _against_the_scipy_loop(eng, pg.two_robot_graph(), exact_gradient=False)


def test_4097_poses_against_the_scipy_loop(eng):
    """The criterion is on the device's answer (3.1e-14 of the majorant when this was written).  The checker's own loop ends at 6.7e-12
    on this graph (pgo_cases.py, OPT_NOISE); nothing is asked of that."""
    _against_the_scipy_loop(eng, pg.anchored_graph(4097), exact_gradient=False)


def test_default_parameters_on_a_long_chain_under_one_prior(eng):
    """The regime the optimiser tests above stay out of: 1 000 poses of drifting odometry with loops at 3 %, ONE prior, noise as the
    covariances say, and the defaults -- 500 CG iterations per solve, which block Jacobi exhausts on such a chain, so LM takes inexact
    steps.  It still has to arrive where the direct solve does.  Both loops stop on an accepted step that lowers the cost by no more
    than 1e-10 of itself; if the steps before it shrank the distance to the minimum cost by as little as 1 % each, what is left is at
    most 1e-10 * 0.99 / 0.01 = 1e-8 of the cost, for either loop."""
    g = pg.drifting_graph(1000)
    want, info = pg.lm_numpy(g, pg.DEFAULTS)
    X, res, _ = eng.pgo_optimize(*g)
    print({k: getattr(res, k) for k, _ in PgoResult._fields_}, "checker:", info["final_cost"], info["iterations"])
    assert info["stop_reason"] == pg.STOP_COST and res.stop_reason == PgoResult.STOP_COST
    assert res.cg_iterations == 500 * res.iterations                              # every solve ran into the cap
    assert abs(res.final_cost - info["final_cost"]) <= 2e-8 * info["final_cost"]
    assert res.iterations > info["iterations"]                                    # inexact steps: more of them


def test_planted_257_poses_return_to_the_truth(eng):
    g, truth = pg.planted_graph()
    X, res, _ = _opt(eng, g)
    cond = pg.condition(pg.linearize_numpy(g, truth))
    bound = pg.TAU_X * max(1.0, cond / pg.ring16_condition())
    dev = pg.pose_deviation(X, truth)
    print("planted: deviation from the truth", dev, "bound", bound, {k: getattr(res, k) for k, _ in PgoResult._fields_})
    assert dev <= bound and res.final_cost <= 1e-20 * res.initial_cost


def test_the_rejected_step_case(eng):
    g, params = pg.rejected_case()
    want, info = pg.lm_numpy(g, params)
    assert not info["trace"][0][1]
    X, res, _ = _opt(eng, g, dict(params, cg_max_iterations=4000))
    print({k: getattr(res, k) for k, _ in PgoResult._fields_}, "checker:", info["final_cost"], info["iterations"], info["rejected"])
    assert res.rejected >= 1
    # both costs are evaluations, each within TAU_LIN of its majorant, at two points near a minimum, where the cost is flat
    assert abs(res.final_cost - info["final_cost"]) <= 2 * pg.TAU_LIN * info["lin"].cost_m
    assert _gradient_is_zero(g, X, exact=True)


def test_one_iteration_is_one_step(eng):
    g = pg.ring16()
    X, res, _ = _opt(eng, g, dict(TIGHT, max_iterations=1))
    assert (res.iterations, res.accepted, res.rejected, res.stop_reason) == (1, 1, 0, PgoResult.STOP_ITERATIONS)
    lin = pg.linearize_numpy(g)
    step = pg.spla.spsolve(pg.hessian(lin, TIGHT["lambda_initial"]).tocsc(), -lin.grad.ravel()).reshape(-1, 6)
    # PCG stops at a relative residual of cg_tolerance, which leaves at most cond(H) * cg_tolerance of the step as its error
    bound = max(pg.TAU_X, pg.ring16_condition() * TIGHT["cg_tolerance"] * float(np.abs(step).max()))
    assert pg.pose_deviation(X, pg.retract(pc._normalised(g.poses), step)) <= bound
    assert res.final_lambda == TIGHT["lambda_initial"] / TIGHT["lambda_factor"] and res.cg_iterations >= 1


def test_poses_out_may_alias_poses(eng):
    g = pg.two_robot_graph()
    X, res, chi2 = _opt(eng, g)
    keep, args, n, m = eng._pgo_inputs(*g)
    buf = keep[0].copy()
    args = (buf.ctypes.data_as(POINTER(c_double)),) + args[1:]
    r2 = PgoResult()
    prm = PgoParams.defaults(**TIGHT)
    assert eng._lib.scl_pgo_optimize(eng._h, *args, byref(prm), buf.ctypes.data_as(POINTER(c_double)), byref(r2), None) == 0
    assert np.array_equal(_bits(buf), _bits(X)) and bytes(r2) == bytes(res)


# ---- state -----------------------------------------------------------------------------------------------------------------------------

def test_the_same_bits_twice_and_after_a_larger_call():
    e = ScanContextEngine(initial_capacity=16)
    try:
        small, hub, big = pg.two_robot_graph(), pg.hub_graph(257, 300), pg.anchored_graph(4097)
        prm = dict(TIGHT, max_iterations=4)

        def run(g):
            X, res, chi2 = _opt(e, g, prm)
            cost, grad, diag, c2 = e.pgo_linearize(*g)
            y = e.pgo_hessian_apply(*g, 0.5, np.ones(6 * len(g.poses)))
            return [_bits(v).copy() for v in (X, chi2, grad, diag, c2, y)] + [bytes(res), cost]
        a_small, a_hub = run(small), run(hub)
        run(big)                                                                  # grows every buffer
        for first, g in ((a_small, small), (a_hub, hub)):
            for x, y in zip(first, run(g)):
                assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y
    finally:
        e.close()


def test_pcm_and_icp_around_a_solve_answer_as_on_a_twin_that_never_ran_it():
    isrc, itgts, G = gc.source(), gc.targets()[:3], gc.guesses()[:3]
    c = pc.case("mixed", 129)
    g = pg.two_robot_graph()
    e, twin = ScanContextEngine(), ScanContextEngine()
    try:
        pp = e.icp_default_params(); pp.max_iterations = 10

        def same(a, b):
            return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) for x, y in zip(a, b))
        pcm = lambda en: en.pcm_select(c.poses_a, c.poses_b, c.idx_a, c.idx_b, c.z, c.cov, c.threshold, odom_var=c.odom_var)
        first = _opt(e, g)
        for _ in range(2):
            assert same(e.icp_align_batch_guess(isrc, itgts, G, pp)[:5], twin.icp_align_batch_guess(isrc, itgts, G, pp)[:5])
            again = _opt(e, g)
            assert same((again[0], again[2]), (first[0], first[2])) and bytes(again[1]) == bytes(first[1])
            a, b = pcm(e), pcm(twin)
            assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])
    finally:
        e.close(); twin.close()


def test_timing_is_reported_under_the_profile_switch(eng):
    g = pg.ring16()
    eng.profile_enable(1)
    try:
        _opt(eng, g)
        lin_ms, solve_ms = eng.pgo_last_timing()
        assert lin_ms > 0.0 and solve_ms > 0.0
        eng.pgo_linearize(*g)
        lin_ms, solve_ms = eng.pgo_last_timing()
        assert lin_ms > 0.0 and solve_ms == 0.0
    finally:
        eng.profile_enable(0)
    _opt(eng, g)                                                                  # an untimed call leaves the last timed call's figures
    assert eng.pgo_last_timing() == (lin_ms, solve_ms)


# ---- errors ----------------------------------------------------------------------------------------------------------------------------

def _raw(e, g, n_poses=None, n_factors=None, n_priors=None, null=(), params=None, lam=0.0, x=None, handle="engine"):
    """the three calls on raw pointers: (their statuses, whether every output kept its sentinel)"""
    lib = e._lib
    dp = lambda a: None if a is None else a.ctypes.data_as(POINTER(c_double))
    ip = lambda a: None if a is None else a.ctypes.data_as(POINTER(c_int))
    hold = {k: np.ascontiguousarray(getattr(g, k), np.int32 if k in ("f_i", "f_j", "p_idx") else np.float64) for k in g._fields}
    arg = {k: None if k in null else (ip(v) if v.dtype == np.int32 else dp(v)) for k, v in hold.items()}
    n, m = len(g.poses), len(g.f_i) + len(g.p_idx)
    common = (e._h if handle == "engine" else None, arg["poses"], n if n_poses is None else n_poses, arg["f_i"], arg["f_j"], arg["f_z"], arg["f_cov"],
              len(g.f_i) if n_factors is None else n_factors, arg["p_idx"], arg["p_z"], arg["p_cov"], len(g.p_idx) if n_priors is None else n_priors)
    cost = c_double(7.0); grad = np.full(6 * n, 7.0); diag = np.full(36 * n, 7.0); chi2 = np.full(m, 7.0); y = np.full(6 * n, 7.0); out = np.full(7 * n, 7.0)
    res = PgoResult(); res.iterations = 7; res.final_cost = 7.0
    xx = np.ones(6 * n) if x is None else np.ascontiguousarray(x, np.float64)
    prm = None if params is None else byref(PgoParams.defaults(**params))
    rcs = (lib.scl_pgo_linearize(*common, None if "cost" in null else byref(cost), None if "gradient" in null else dp(grad),
                                 None if "diag" in null else dp(diag), None if "chi2" in null else dp(chi2)),
           lib.scl_pgo_hessian_apply(*common, lam, None if "x" in null else dp(xx), None if "y" in null else dp(y)),
           lib.scl_pgo_optimize(*common, prm, None if "poses_out" in null else dp(out), None if "result" in null else byref(res), dp(chi2)))
    untouched = (cost.value == 7.0 and res.iterations == 7 and res.final_cost == 7.0 and
                 all((v == 7.0).all() for v in (grad, diag, chi2, y, out)))
    return rcs, untouched


def test_errors_write_nothing(eng):
    g = pg.lin_case("chain5")
    assert _raw(eng, g)[0] == (0, 0, 0)
    F = len(g.f_i)

    def put(field, row, col, value):
        a = np.array(getattr(g, field)).copy()
        a.reshape(len(a), -1)[row, col] = value
        return g._replace(**{field: a})

    def scaled_q(field, row, s):
        a = np.array(getattr(g, field), np.float64).copy()
        a[row, 3:] *= s
        return g._replace(**{field: a})
    rank5 = np.diag([1.0, 1, 1, 1, 1, 0]).ravel()
    J = np.random.RandomState(2).standard_normal((5, 6))
    every = [                                                                     # refused by all three calls
        dict(n_poses=-1), dict(n_factors=-1), dict(n_priors=-1), dict(n_poses=0), dict(n_poses=1048577), dict(n_factors=4194305),
        dict(n_priors=len(g.poses) + 1), dict(null=("poses",)), dict(null=("f_i",)), dict(null=("f_j",)), dict(null=("f_z",)), dict(null=("f_cov",)),
        dict(null=("p_idx",)), dict(null=("p_z",)), dict(null=("p_cov",)),
        dict(g=put("f_i", 2, 0, len(g.poses))), dict(g=put("f_j", 0, 0, -1)), dict(g=put("p_idx", 0, 0, len(g.poses))), dict(n_poses=4),
        dict(g=put("f_i", 1, 0, int(g.f_j[1]))),                                  # f_i == f_j
        dict(g=put("poses", 3, 1, np.nan)), dict(g=put("f_z", F - 1, 6, np.inf)), dict(g=put("p_z", 0, 0, np.nan)),
        dict(g=put("f_cov", 0, 1, np.nan)), dict(g=put("p_cov", 0, 35, np.inf)),
        dict(g=scaled_q("poses", 1, 0.49)), dict(g=scaled_q("f_z", 0, 2.01)), dict(g=scaled_q("p_z", 0, 0.49)),
        dict(g=g._replace(f_cov=np.vstack([rank5[None], g.f_cov[1:]]))), dict(g=g._replace(p_cov=(J.T @ J).reshape(1, 36))),
        dict(g=g._replace(f_cov=np.vstack([g.f_cov[:-1], -g.f_cov[-1:]]))),
        dict(n_priors=0),                                                         # no prior: the one component has none
        dict(g=g._replace(f_i=g.f_i[2:], f_j=g.f_j[2:], f_z=g.f_z[2:], f_cov=g.f_cov[2:])),   # poses 0 - 1 - 2 cut into components, one prior
        dict(handle=None),
    ]
    for kw in every:
        kw = dict(kw)
        rcs, untouched = _raw(eng, kw.pop("g", g), **kw)
        assert rcs == (INVALID_ARG,) * 3 and untouched, kw
    with pytest.raises(SclError, match="component without a prior"):
        eng.pgo_optimize(*g._replace(p_idx=np.zeros(0, np.int32), p_z=np.zeros((0, 7)), p_cov=np.zeros((0, 36))))
    # refused by the call they belong to
    assert _raw(eng, g, null=("cost", "gradient", "diag", "chi2"))[0][0] == INVALID_ARG
    for kw in (dict(null=("x",)), dict(null=("y",)), dict(lam=-1e-300), dict(lam=np.nan), dict(lam=np.inf), dict(x=np.full(30, np.nan))):
        rcs, _ = _raw(eng, g, **kw)
        assert rcs[1] == INVALID_ARG and rcs[0] == 0, kw
    for kw in (dict(null=("poses_out",)), dict(null=("result",))):
        assert _raw(eng, g, **kw)[0][2] == INVALID_ARG
    for field in ("max_iterations", "lambda_initial", "lambda_factor", "lambda_max", "relative_cost_tolerance", "step_tolerance", "cg_tolerance",
                  "cg_max_iterations"):
        values = (0, -1) if "iterations" in field else (0.0, -1.0, np.nan, np.inf)
        for v in values + ((1.0,) if field == "lambda_factor" else ()):
            n, m = len(g.poses), F + 1
            out = np.full(7 * n, 7.0); res = PgoResult(); res.iterations = 7
            keep, args, _, _ = eng._pgo_inputs(*g)
            rc = eng._lib.scl_pgo_optimize(eng._h, *args, byref(PgoParams.defaults(**{field: v})), out.ctypes.data_as(POINTER(c_double)), byref(res), None)
            assert rc == INVALID_ARG and (out == 7.0).all() and res.iterations == 7, (field, v)


# ---- two shards ------------------------------------------------------------------------------------------------------------------------

def test_sharded_engine_equals_plain(eng):
    g = pg.two_robot_graph()
    sh = ScanContextEngine(initial_capacity=16, devices=[0, 0], exchange=1)
    try:
        a, b = _opt(eng, g), _opt(sh, g)
        assert np.array_equal(_bits(a[0]), _bits(b[0])) and bytes(a[1]) == bytes(b[1]) and np.array_equal(_bits(a[2]), _bits(b[2]))
        la, lb = eng.pgo_linearize(*g), sh.pgo_linearize(*g)
        assert la[0] == lb[0] and all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(la[1:], lb[1:]))
        x = np.arange(6.0 * len(g.poses))
        assert np.array_equal(_bits(eng.pgo_hessian_apply(*g, 2.0, x)), _bits(sh.pgo_hessian_apply(*g, 2.0, x)))
        with pytest.raises(SclError, match="out of range"):
            sh.pgo_optimize(*g._replace(p_idx=np.int32([999])))
        sh.profile_enable(1)
        _opt(sh, g)
        assert min(sh.pgo_last_timing()) > 0.0
        sh.profile_enable(0)
    finally:
        sh.close()
