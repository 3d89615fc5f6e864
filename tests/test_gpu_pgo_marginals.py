"""The many-column solve and the marginal covariances on the GPU (include/scl_engine.h "POSE-GRAPH SOLVE, MANY RIGHT-HAND SIDES AND
MARGINAL COVARIANCES") against tests/pgo_marginal_cases.py and tests/pgo_condensed_cases.py: every column within TAU_STEP as a backward
error and consistent with scl_pgo_hessian_apply; a column's bits independent of its neighbours, its position, the call's size and the
column groups; the marginals bit for bit the rows of the unit columns, within TAU_MARG / TAU_REL of the 40-digit checker and of the
numpy restatement, and equal to the answers derived by hand on exact chains; the chain from the search to the solve extended by the
marginals; errors that write nothing; isolation from the other solves; two shards.

The group border.  Columns run in groups of 256 MB / (8 (6 n_poses + 18 n_nodes)) columns, from 16 on a multiple of 16.  chain4097 (4097
poses, one segment of 4097 path nodes) has 786 624 bytes per column: 341, so 336 columns per group.  GROUP_COLUMNS = 340 columns reach a
second group of 4 -- a partial tile, and fewer than the minimum of 6."""
import functools
from ctypes import POINTER, byref, c_double, c_int

import numpy as np
import pytest

import icp_guess_cases as gc
import pcm_cases as pc
import pgo_cases as pg
import pgo_condensed_cases as cc
import pgo_marginal_cases as mc
from scl_slam_amd import PgoParams, PgoResult, ScanContextEngine, SclError
from scl_slam_amd.synth import rigid_transform, synth_scan

pytestmark = pytest.mark.gpu
INVALID_ARG = -1
SOLVE_CASES = ("segment1", "segment2", "segment63", "segment64", "segment65", "segment257", "mid_prior", "adjacent", "duplicate", "reversed",
               "hub257", "drifting4097")
N_RHS = (1, 15, 16, 17, 33)
GROUP_COLUMNS, GROUP = 340, 336


@pytest.fixture(scope="module")
def eng():
    e = ScanContextEngine(initial_capacity=16)
    yield e
    e.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _system(name, lam):
    lin = cc.step_lin(name)
    return pg.hessian(lin, lam), pg.hessian_majorant(lin, lam)


@functools.lru_cache(maxsize=None)
def _columns(name, count=33):
    """`count` right-hand sides (count, n, 6) of the named graph: -g of the checker, a unit column, a column of ones, then random dense
    columns of mixed scale; read-only"""
    lin = cc.step_lin(name)
    rs = np.random.RandomState(len(name) + 31 * lin.n)
    b = rs.standard_normal((count, lin.n, 6)) * 10.0 ** rs.uniform(-3, 3, (count, 1, 1))
    b[0] = -lin.grad
    if count > 2:
        b[1] = 0.0; b[1, lin.n // 2, 4] = 1.0
        b[2] = 1.0
    b.setflags(write=False)
    return b


def _backward_errors(name, lam, b, x):
    """per column: max over rows of |H x - b| / (|H| |x| + |b|), the measure of cc.backward_error with the column as right-hand side"""
    H, Hm = _system(name, lam)
    B, X = b.reshape(len(b), -1).T, x.reshape(len(x), -1).T
    return (np.abs(H @ X - B) / (Hm @ np.abs(X) + np.abs(B))).max(0)


# ---- the many-column solve -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lam", cc.LAMBDAS)
@pytest.mark.parametrize("name", SOLVE_CASES)
def test_every_column_within_tau_step_and_consistent_with_the_operator(eng, name, lam):
    g, b = cc.step_case(name), _columns(name)
    Hm = _system(name, lam)[1]
    full = eng.pgo_solve_condensed_many(*g, lam, b)
    assert full.shape == b.shape and np.isfinite(full).all()
    for n_rhs in N_RHS:
        x = full if n_rhs == len(b) else eng.pgo_solve_condensed_many(*g, lam, b[:n_rhs])
        be = _backward_errors(name, lam, b[:n_rhs], x)
        print(f"{name} lambda {lam:g} n_rhs {n_rhs}: largest backward error {be.max():.3g} (column {int(be.argmax())}), TAU_STEP {cc.TAU_STEP:.3g}")
        assert x.shape == (n_rhs, len(g.poses), 6) and (be <= cc.TAU_STEP).all()
        assert _same(x, full[:n_rhs])                        # the core rule, once more
    own = []
    for c in range(len(b)):                                 # the device's own operator on every column
        y = eng.pgo_hessian_apply(*g, lam, full[c]).ravel()
        own.append(float((np.abs(y - b[c].ravel()) / (Hm @ np.abs(full[c].ravel()) + np.abs(b[c].ravel()))).max()))
    print(f"{name} lambda {lam:g}: against the device's operator {max(own):.3g}")
    assert max(own) <= cc.TAU_STEP
    # the -g column against the single step: its accuracy, not its bits.  The column is the checker's -g, the step's the device's own, so
    # the step is held as a solution of the column's system
    d = eng.pgo_solve_condensed(*g, lam)
    grad = eng.pgo_linearize(*g)[1]
    own_col = eng.pgo_solve_condensed_many(*g, lam, -grad[None])[0]
    be = _backward_errors(name, lam, -grad[None], d[None])[0]
    print(f"{name} lambda {lam:g}: the single step as a solution of the -g column {be:.3g}; bit equal to the column solved here: {_same(own_col, d)}; "
          f"largest difference {np.abs(own_col - d).max():.3g} of {np.abs(d).max():.3g}")
    assert be <= cc.TAU_STEP and _backward_errors(name, lam, -grad[None], own_col[None])[0] <= cc.TAU_STEP


@pytest.mark.parametrize("name", ["adjacent", "segment65", "hub257", "drifting4097"])
def test_a_column_does_not_depend_on_its_neighbours_or_its_position(eng, name):
    g, b = cc.step_case(name), _columns(name)
    full = eng.pgo_solve_condensed_many(*g, 1e-5, b)
    for c in (0, 1, 15, 16, 32):
        alone = eng.pgo_solve_condensed_many(*g, 1e-5, b[c:c + 1])
        first = eng.pgo_solve_condensed_many(*g, 1e-5, np.concatenate([b[c:c + 1], b[:16][::-1]]))     # as column 0 of 17, other neighbours
        assert _same(alone[0], full[c]) and _same(first[0], full[c]), (name, c)
        assert _same(first[1:], full[:16][::-1])


def test_a_column_does_not_depend_on_the_column_groups(eng):
    """GROUP_COLUMNS columns on chain4097: two groups (see the module's docstring); columns on both sides of the border solved alone, and
    the second group's columns as the head of a call"""
    g = cc.step_case("chain4097")
    n = len(g.poses)
    assert eng.pgo_count_junctions(n, g.f_i, g.f_j, g.p_idx) == (2, 1, 4095)
    assert (256 << 20) // (8 * (6 * n + 18 * n)) // 16 * 16 == GROUP < GROUP_COLUMNS
    rs = np.random.RandomState(4097)
    b = rs.standard_normal((GROUP_COLUMNS, n, 6))
    full = eng.pgo_solve_condensed_many(*g, 1e-5, b)
    for c in (0, GROUP - 1, GROUP, GROUP_COLUMNS - 1):
        assert _same(eng.pgo_solve_condensed_many(*g, 1e-5, b[c:c + 1])[0], full[c]), c
    assert _same(eng.pgo_solve_condensed_many(*g, 1e-5, b[GROUP - 2:]), full[GROUP - 2:])
    H, Hm = pg.hessian(cc.step_lin("chain4097"), 1e-5), pg.hessian_majorant(cc.step_lin("chain4097"), 1e-5)
    for c in (GROUP - 1, GROUP, GROUP_COLUMNS - 1):
        be = float((np.abs(H @ full[c].ravel() - b[c].ravel()) / (Hm @ np.abs(full[c].ravel()) + np.abs(b[c].ravel()))).max())
        assert be <= cc.TAU_STEP, (c, be)


def test_the_same_bits_twice_after_a_larger_call_and_in_place():
    e = ScanContextEngine(initial_capacity=16)
    try:
        small, big = cc.step_case("adjacent"), cc.step_case("drifting4097")
        b = _columns("adjacent")
        q = np.int32([0, 3, 4, 9, 11])
        first = e.pgo_solve_condensed_many(*small, 1e-5, b)
        m_first = e.pgo_marginals(*small, q, q[::-1].copy())
        assert _same(first, e.pgo_solve_condensed_many(*small, 1e-5, b))
        e.pgo_solve_condensed_many(*big, 1e-5, _columns("drifting4097"))                        # grows every buffer
        e.pgo_marginals(*big, np.arange(0, 4096, 16), np.arange(0, 4096, 16))
        assert _same(first, e.pgo_solve_condensed_many(*small, 1e-5, b))
        m_again = e.pgo_marginals(*small, q, q[::-1].copy())
        assert _same(m_first[0], m_again[0]) and _same(m_first[1], m_again[1])
        # x aliasing rhs
        keep, args, n, m = e._pgo_inputs(*small)
        buf = np.array(b)
        p = buf.ctypes.data_as(POINTER(c_double))
        assert e._lib.scl_pgo_solve_condensed_many(e._h, *args, 1e-5, p, len(buf), p) == 0
        assert _same(buf, first)
    finally:
        e.close()


# ---- the marginals -------------------------------------------------------------------------------------------------------------------------

def _unit_columns(n, poses):
    b = np.zeros((6 * len(poses), n, 6))
    for u, p in enumerate(poses):
        for a in range(6):
            b[6 * u + a, p, a] = 1.0
    return b


def test_blocks_are_the_rows_of_the_unit_columns_bit_for_bit(eng):
    g = pg.two_robot_graph()
    rs = np.random.RandomState(8)
    qi, qj = rs.randint(0, 64, 40).astype(np.int32), rs.randint(0, 64, 40).astype(np.int32)
    qi[:4] = qj[:4]                                         # diagonal blocks among them
    sel = sorted(set(qi.tolist()) | set(qj.tolist()))
    pos = {p: u for u, p in enumerate(sel)}
    x = eng.pgo_solve_condensed_many(*g, 0.0, _unit_columns(64, sel))
    blocks, rel = eng.pgo_marginals(*g, qi, qj)
    for k, (i, j) in enumerate(zip(qi.tolist(), qj.tolist())):
        want = x[6 * pos[j]:6 * pos[j] + 6, i, :].T         # rows of pose i in the columns of pose j
        if i == j:
            want = np.triu(want) + np.triu(want, 1).T
            assert _same(blocks[k], blocks[k].T) and (rel[k] == 0).all() and not np.signbit(rel[k]).any()
        assert _same(blocks[k], want), (k, i, j)
        assert _same(rel[k], rel[k].T)


def _all_pairs(n):
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    return i.ravel().astype(np.int32), j.ravel().astype(np.int32)


@pytest.mark.parametrize("name", mc.SMALL_CASES)
def test_marginals_against_the_40_digit_checker(eng, name):
    g = mc.small_case(name)
    Se, rel_e = mc.small_exact(name)
    qi, qj = _all_pairs(len(g.poses))
    blocks, rel = eng.pgo_marginals(*g, qi, qj)
    dm = max(mc.dev_block(blocks[k], mc.block(Se, i, j), Se, i, j) for k, (i, j) in enumerate(zip(qi, qj)))
    dr = max(mc.dev_rel(rel[k], rel_e[i, j]) for k, (i, j) in enumerate(zip(qi, qj)) if i != j)
    print(f"{name}: blocks {dm:.3e} (TAU_MARG {mc.TAU_MARG:.1e}), rel {dr:.3e} (TAU_REL {mc.TAU_REL:.1e})")
    assert dm <= mc.TAU_MARG and dr <= mc.TAU_REL
    for k, (i, j) in enumerate(zip(qi, qj)):
        if i == j:
            assert _same(blocks[k], blocks[k].T) and (rel[k] == 0).all()
    if name == "two_robots_cut":
        # junction - junction (0, 3), interior - interior in one segment (1, 2) and across segments (1, 5), (5, 12), both orders, the
        # same pose in many queries; one query; only blocks; only rel; a list and a superset of it
        pairs = [(0, 3), (3, 0), (1, 2), (2, 1), (1, 5), (5, 1), (5, 12), (12, 5), (1, 1), (1, 15), (1, 0)]
        si, sj = np.int32([p[0] for p in pairs]), np.int32([p[1] for p in pairs])
        sb, sr = eng.pgo_marginals(*g, si, sj)
        for k, (i, j) in enumerate(pairs):
            assert mc.dev_block(sb[k], mc.block(Se, i, j), Se, i, j) <= mc.TAU_MARG
            assert _same(sb[k], blocks[16 * i + j]) and _same(sr[k], rel[16 * i + j])       # the superset gives the shared queries' bits
        one_b, one_r = eng.pgo_marginals(*g, [5], [12])
        assert _same(one_b[0], blocks[16 * 5 + 12]) and _same(one_r[0], rel[16 * 5 + 12])
        only_b = eng.pgo_marginals(*g, si, sj, want_rel=False)
        only_r = eng.pgo_marginals(*g, si, sj, want_blocks=False)
        assert only_b[1] is None and only_r[0] is None and _same(only_b[0], sb) and _same(only_r[1], sr)


@pytest.mark.parametrize("name", ["anchored257", "hub257"])
def test_marginals_against_the_numpy_restatement_with_256_distinct_poses(eng, name):
    """blocks within TAU_MARG_NUMPY_257 (the factor 64 and its reason: tests/pgo_marginal_cases.py; measured on an MI355X against the
    numpy restatement: anchored257 2.9e-13, hub257 6.2e-13, TAU_MARG 3.2e-13), rel within TAU_REL"""
    g = pg.anchored_graph(257) if name == "anchored257" else cc.step_case("hub257")
    n = len(g.poses)
    S, X = mc.sigma_numpy(pg.linearize_numpy(g)), pc._normalised(g.poses)
    rs = np.random.RandomState(257)
    sel = np.sort(rs.permutation(n)[:256]).astype(np.int32)
    qi = np.concatenate([sel, sel[rs.randint(0, 256, 768)]]).astype(np.int32)
    qj = np.concatenate([sel, sel[rs.randint(0, 256, 768)]]).astype(np.int32)
    blocks, rel = eng.pgo_marginals(*g, qi, qj)
    dm = max(mc.dev_block(blocks[k], mc.block(S, i, j), S, i, j) for k, (i, j) in enumerate(zip(qi, qj)))
    dr = max(mc.dev_rel(rel[k], mc.rel_numpy(S, X, i, j)) for k, (i, j) in enumerate(zip(qi, qj)) if i != j)
    print(f"{name}: blocks {dm:.3e} (TAU_MARG_NUMPY_257 {mc.TAU_MARG_NUMPY_257:.1e}, TAU_MARG {mc.TAU_MARG:.1e}), rel {dr:.3e} (TAU_REL {mc.TAU_REL:.1e})")
    assert dm <= mc.TAU_MARG_NUMPY_257 and dr <= mc.TAU_REL
    assert all(_same(blocks[k], blocks[k].T) for k in range(256))


@pytest.mark.parametrize("n", [4, 12, 65])
def test_known_answers_on_exact_chains(eng, n):
    """Sigma[0, 0] = p_cov, rel(k, k + 1) = f_cov[k], rel(0, 2) = Ad(z_1^-1) f_cov[0] Ad(z_1^-1)^T + f_cov[1] (derived in
    tests/pgo_marginal_cases.py).  Every query's bound is mc.known_answer_bound: TAU, or 16 x the numpy restatement's own deviation from
    the hand-derived answer on that query where that is larger (chain65 only).  Measured on an MI355X, chain65: Sigma[0, 0] 7.0e-15,
    rel(0, 2) 4.5e-13 (the restatement: 1.8e-13)."""
    g = mc.exact_chain(n)
    S, X = mc.sigma_numpy(pg.linearize_numpy(g)), pc._normalised(g.poses)
    qi = np.concatenate([[0, 0], np.arange(n - 1)]).astype(np.int32)
    qj = np.concatenate([[0, 2], np.arange(1, n)]).astype(np.int32)
    blocks, rel = eng.pgo_marginals(*g, qi, qj)
    d0 = mc.dev_block(blocks[0], mc.known_prior_block(g), S, 0, 0)
    r0 = mc.dev_block(mc.block(S, 0, 0), mc.known_prior_block(g), S, 0, 0)
    d2, r2 = mc.dev_rel(rel[1], mc.known_rel_02(g)), mc.dev_rel(mc.rel_numpy(S, X, 0, 2), mc.known_rel_02(g))
    print(f"chain{n}: Sigma[0, 0] {d0:.3e} (restatement {r0:.3e}), rel(0, 2) {d2:.3e} (restatement {r2:.3e})")
    assert d0 <= mc.known_answer_bound(mc.TAU_MARG, r0) and d2 <= mc.known_answer_bound(mc.TAU_REL, r2)
    for k in range(n - 1):
        want = mc.known_rel_step(g, k)
        d, r = mc.dev_rel(rel[2 + k], want), mc.dev_rel(mc.rel_numpy(S, X, k, k + 1), want)
        if k in (0, n // 2, n - 2):
            print(f"chain{n}: rel({k}, {k + 1}) {d:.3e} (restatement {r:.3e}), bound {mc.known_answer_bound(mc.TAU_REL, r):.3e}")
        assert d <= mc.known_answer_bound(mc.TAU_REL, r), (n, k, d, r)


# ---- the chain from the search to the solve, extended by the marginals -----------------------------------------------------------------------

K, SECTORS, WRONG = 5, (7, 3, 11, 0, 5), 2


def _pose7(M):
    """x, y, z, qx, qy, qz, qw of a 4 x 4 rigid motion"""
    R = np.asarray(M, np.float64)[:3, :3]
    Kq = np.array([[R[0, 0] - R[1, 1] - R[2, 2], 0, 0, 0], [R[0, 1] + R[1, 0], R[1, 1] - R[0, 0] - R[2, 2], 0, 0],
                   [R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], R[2, 2] - R[0, 0] - R[1, 1], 0],
                   [R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], R[0, 0] + R[1, 1] + R[2, 2]]]) / 3.0
    w, v = np.linalg.eigh(Kq, UPLO="L")
    q = v[:, np.argmax(w)]
    return np.concatenate([np.asarray(M, np.float64)[:3, 3], q if q[3] >= 0 else -q])


def test_the_chain_from_search_to_the_marginals():
    """tests/test_gpu_pgo_chain.py's five places restated: poses 0 .. 4 robot 1's (drifting odometry), 5 .. 9 robot 0's (a prior on its
    first keyframe, exact odometry); PCM rejects the wrong loop at place WRONG.  After scl_pgo_optimize_condensed over the members, the
    marginal of robot 1's keyframe at that place -- held by its two neighbours' odometry only -- has a larger largest eigenvalue than
    either neighbour's, and rel between the two robots' first keyframes is positive definite."""
    W = rigid_transform(0.01, -0.02, 0.7, 40.0, -25.0, 0.5)
    odom_var = [1e-6] * 3 + [1e-4] * 3
    e = ScanContextEngine(num_ring=20, num_sector=60)
    try:
        clouds = [synth_scan(20000, seed=7 + 10 * k) for k in range(K)]
        poses_pre = [np.float32([14.0 + 9 * k, -6.5 + 4 * k, 0.4 - 0.1 * k, 0.02, -0.015, 1.1 + 0.3 * k]) for k in range(K)]
        for k in range(K):
            e.make_and_save(clouds[k], 0, k)
            e.keyframe_put(0, k, clouds[k])
        poses_a, poses_b, zs, covs, truth_a, truth_b = [], [], [], [], [], []
        for k in range(K):
            Rz = rigid_transform(0.0, 0.0, np.radians(6.0 * SECTORS[k]), 0, 0, 0)
            M_pre = gc.pose_matrix(poses_pre[k])
            pose_cur = np.float32(e.matrix_to_pose(np.linalg.inv(W) @ M_pre @ np.linalg.inv(Rz)))
            M_cur = gc.pose_matrix(pose_cur)
            turned = clouds[k].copy()
            turned[:, :3] = (clouds[k][:, :3].astype(np.float64) @ Rz[:3, :3].T).astype(np.float32)
            received = turned.copy()
            xyz = turned[:, :3].astype(np.float64) @ M_cur[:3, :3].T + M_cur[:3, 3]
            received[:, :3] = (xyz + gc.NOISE * np.random.RandomState(90 + k).standard_normal(xyz.shape)).astype(np.float32)
            e.make_and_save(turned, 1, k)
            ids, shifts, dists, found = e.sc_search_inter([K + k], 2, robot_pre=0)
            assert found[0] >= 1 and e.get_index(int(ids[0, 0])) == (0, k) and shifts[0, 0] == SECTORS[k]
            G = e.loop_guess_from_shift(int(shifts[0, 0]), 60, pose_cur, poses_pre[k])[None]
            args = (received, gc.E2E_LEAF, 0, [k], 0, M_pre.astype(np.float32).reshape(1, 1, 4, 4), gc.E2E_LEAF)
            icp = e.icp_align_batch_from_store_guess(*args, G)
            ev = e.registration_eval_batch_from_store(*args, icp[0], 0.5)
            s2 = ev.moments[0, 9] / max(1, int(ev.n_inliers[0]) - 6)
            zs.append(e.loop_pose_between(icp[0][0], pose_cur, poses_pre[k])[0]); covs.append(ScanContextEngine.loop_covariance(ev.information(0), s2))
            poses_a.append(_pose7(M_cur)); poses_b.append(_pose7(M_pre))
            truth_b.append(_pose7(M_pre)); truth_a.append(_pose7(M_pre @ np.linalg.inv(Rz)))
        truth = np.array(truth_a + truth_b)
        idx = np.arange(K, dtype=np.int32)
        z = np.array(zs)
        z[WRONG] = pc.compose(z[WRONG], np.concatenate([[3.0, 0.0, 0.0], pc.rotvec_to_quat([0.0, 0.0, 0.5])]))
        cov = np.array(covs).reshape(K, 36)
        mem, seed, deg = e.pcm_select(np.array(poses_a), np.array(poses_b), idx, idx, z, cov, pc.THRESHOLD, odom_var=odom_var)
        assert mem.tolist() == [k for k in range(K) if k != WRONG]
        bias = np.array([0.0, 0.0, 0.01, 0.05, 0.0, 0.0])
        odo_cov_a = np.diag([1e-4] * 3 + [2.5e-3] * 3).ravel(); tight = (1e-8 * np.eye(6)).ravel()
        f_i, f_j, f_z, f_cov = [], [], [], []
        for k in range(K - 1):
            f_i += [k, K + k]; f_j += [k + 1, K + k + 1]
            f_z += [pg.perturb(pg.between(truth[k], truth[k + 1]), bias), pg.between(truth[K + k], truth[K + k + 1])]
            f_cov += [odo_cov_a, tight]
        start = [pg.perturb(truth[0], bias)]
        for k in range(K - 1):
            nxt = pc.compose(start[-1], f_z[2 * k]); nxt[3:] /= np.linalg.norm(nxt[3:])
            start.append(nxt)
        start = np.array(start + [truth[K + k] for k in range(K)])
        g = pg.graph(start, f_i + [int(idx[m]) for m in mem], f_j + [K + int(idx[m]) for m in mem],
                     np.vstack([np.array(f_z)] + [z[m][None] for m in mem]), np.vstack([np.array(f_cov)] + [cov[m][None] for m in mem]),
                     [K], truth[K][None], tight[None])
        X, res, chi2, failed = e.pgo_optimize_condensed(*g, params=PgoParams.defaults(relative_cost_tolerance=1e-14, step_tolerance=1e-14))
        assert res.final_cost < res.initial_cost and failed == 0
        q = np.int32([WRONG - 1, WRONG, WRONG + 1, 0])
        blocks, rel = e.pgo_marginals(*g._replace(poses=X), q, np.int32([WRONG - 1, WRONG, WRONG + 1, K]))
        top = [float(np.linalg.eigvalsh(blocks[k]).max()) for k in range(3)]
        print("largest eigenvalues of the marginals at places", WRONG - 1, WRONG, WRONG + 1, ":", top, "\nrel(0, K) eigenvalues:", np.linalg.eigvalsh(rel[3]))
        assert top[1] > top[0] and top[1] > top[2]
        assert np.linalg.eigvalsh(rel[3]).min() > 0
    finally:
        e.close()


# ---- errors, isolation, shards ---------------------------------------------------------------------------------------------------------------

def _raw(e, g, n_poses=None, n_factors=None, n_priors=None, null=(), lam=1e-5, handle="engine", rhs=None, n_rhs=2, q=((0, 1), (2, 2)), n_queries=None):
    """the two calls on raw pointers: (their statuses, whether every output kept its sentinel)"""
    lib = e._lib
    dp = lambda a: None if a is None else a.ctypes.data_as(POINTER(c_double))
    ip = lambda a: None if a is None else a.ctypes.data_as(POINTER(c_int))
    hold = {k: np.ascontiguousarray(getattr(g, k), np.int32 if k in ("f_i", "f_j", "p_idx") else np.float64) for k in g._fields}
    arg = {k: None if k in null else (ip(v) if v.dtype == np.int32 else dp(v)) for k, v in hold.items()}
    n = len(g.poses)
    common = (e._h if handle == "engine" else None, arg["poses"], n if n_poses is None else n_poses, arg["f_i"], arg["f_j"], arg["f_z"], arg["f_cov"],
              len(g.f_i) if n_factors is None else n_factors, arg["p_idx"], arg["p_z"], arg["p_cov"], len(g.p_idx) if n_priors is None else n_priors)
    b = np.ones((2, n, 6)) if rhs is None else np.ascontiguousarray(rhs, np.float64)
    x = np.full(b.size, 7.0)
    qi, qj = np.int32([p[0] for p in q]), np.int32([p[1] for p in q])
    nq = len(qi) if n_queries is None else n_queries
    blocks = np.full(36 * max(len(qi), 1), 7.0); rel = np.full(36 * max(len(qi), 1), 7.0)
    rcs = (lib.scl_pgo_solve_condensed_many(*common, lam, None if "rhs" in null else dp(b), n_rhs, None if "x" in null else dp(x)),
           lib.scl_pgo_marginals(*common, None if "q_i" in null else ip(qi), None if "q_j" in null else ip(qj), nq,
                                 None if "blocks" in null else dp(blocks), None if "rel" in null else dp(rel)))
    return rcs, all((v == 7.0).all() for v in (x, blocks, rel))


def test_errors_write_nothing(eng):
    g = pg.lin_case("chain5")
    n, F = len(g.poses), len(g.f_i)
    assert _raw(eng, g)[0] == (0, 0)

    def put(field, row, col, value):
        a = np.array(getattr(g, field)).copy()
        a.reshape(len(a), -1)[row, col] = value
        return g._replace(**{field: a})

    def scaled_q(field, row, s):
        a = np.array(getattr(g, field), np.float64).copy()
        a[row, 3:] *= s
        return g._replace(**{field: a})
    rank5 = np.diag([1.0, 1, 1, 1, 1, 0]).ravel()
    hub = cc.step_case("hub257")
    both = [                                                                      # everything scl_pgo_solve_condensed refuses
        dict(g=cc.many_junctions()),
        dict(n_poses=-1), dict(n_factors=-1), dict(n_priors=-1), dict(n_poses=0), dict(n_poses=1048577), dict(n_factors=4194305),
        dict(n_priors=n + 1), dict(null=("poses",)), dict(null=("f_i",)), dict(null=("f_j",)), dict(null=("f_z",)), dict(null=("f_cov",)),
        dict(null=("p_idx",)), dict(null=("p_z",)), dict(null=("p_cov",)),
        dict(g=put("f_i", 2, 0, n)), dict(g=put("f_j", 0, 0, -1)), dict(g=put("p_idx", 0, 0, n)), dict(n_poses=4),
        dict(g=put("f_i", 1, 0, int(g.f_j[1]))),
        dict(g=put("poses", 3, 1, np.nan)), dict(g=put("f_z", F - 1, 6, np.inf)), dict(g=put("p_z", 0, 0, np.nan)),
        dict(g=put("f_cov", 0, 1, np.nan)), dict(g=put("p_cov", 0, 35, np.inf)),
        dict(g=scaled_q("poses", 1, 0.49)), dict(g=scaled_q("f_z", 0, 2.01)), dict(g=scaled_q("p_z", 0, 0.49)),
        dict(g=g._replace(f_cov=np.vstack([rank5[None], g.f_cov[1:]]))),
        dict(n_priors=0),
        dict(g=g._replace(f_i=g.f_i[2:], f_j=g.f_j[2:], f_z=g.f_z[2:], f_cov=g.f_cov[2:])),
        dict(handle=None),
    ]
    for kw in both:
        kw = dict(kw)
        rcs, untouched = _raw(eng, kw.pop("g", g), **kw)
        assert rcs == (INVALID_ARG,) * 2 and untouched, kw
    bad = np.ones((2, n, 6)); bad[1, n - 1, 5] = np.nan
    inf = np.ones((2, n, 6)); inf[0, 0, 0] = -np.inf
    for kw in (dict(n_rhs=0), dict(n_rhs=-1), dict(n_rhs=1537), dict(null=("rhs",)), dict(null=("x",)), dict(rhs=bad), dict(rhs=inf),
               dict(lam=-1e-300), dict(lam=np.nan), dict(lam=np.inf)):
        rcs, untouched = _raw(eng, g, **kw)
        assert rcs == (INVALID_ARG, 0) and untouched is False, kw        # the marginals ran and wrote
        x_kept = _raw(eng, g, null=("blocks", "rel") + tuple(kw.get("null", ())), **{k: v for k, v in kw.items() if k != "null"})
        assert x_kept == ((INVALID_ARG, INVALID_ARG), True), kw          # with both refused nothing is written
    for kw in (dict(n_queries=0), dict(n_queries=-1), dict(n_queries=4097), dict(null=("q_i",)), dict(null=("q_j",)), dict(null=("blocks", "rel")),
               dict(q=((0, n),)), dict(q=((-1, 0),)), dict(q=((0, 1), (n, 0))), dict(q=((0, 0), (1, -5)))):
        rcs, untouched = _raw(eng, g, n_rhs=0, **kw)
        assert rcs == (INVALID_ARG,) * 2 and untouched, kw
    # 257 distinct poses; 256 of them pass
    all257 = tuple((k, k) for k in range(257))
    assert _raw(eng, hub, n_rhs=0, q=all257) == ((INVALID_ARG,) * 2, True)
    assert _raw(eng, hub, n_rhs=0, q=all257[:128] + tuple((k, 383 - k) for k in range(128, 256)))[0] == (INVALID_ARG, 0)
    with pytest.raises(SclError, match="256 distinct"):
        eng.pgo_marginals(*hub, np.arange(257), np.arange(257))
    with pytest.raises(SclError, match="1024 junctions"):
        eng.pgo_marginals(*cc.many_junctions(), [0], [1])
    with pytest.raises(SclError, match="n_rhs"):
        eng.pgo_solve_condensed_many(*g, 1e-5, np.ones((1537, n, 6)))


def test_the_other_solves_around_the_calls_answer_as_on_a_twin_that_never_made_them():
    g, other = pg.two_robot_graph(), cc.step_case("segment257")
    e, twin = ScanContextEngine(initial_capacity=16), ScanContextEngine(initial_capacity=16)
    try:
        def solves(en):
            a = en.pgo_optimize(*g, params=PgoParams.defaults(**dict(pg.TIGHT, cg_max_iterations=4000)))
            b = en.pgo_optimize_condensed(*g, params=PgoParams.defaults(**dict(pg.TIGHT, max_iterations=3)))
            d = en.pgo_solve_condensed(*g, 1e-5)
            return [_bits(a[0]).copy(), bytes(a[1]), _bits(a[2]).copy(), _bits(b[0]).copy(), bytes(b[1]), _bits(b[2]).copy(), b[3], _bits(d).copy()]

        def same(a, b):
            return all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))
        before = solves(e)
        assert same(before, solves(twin))
        e.pgo_solve_condensed_many(*other, 1e-5, _columns("segment257"))
        e.pgo_marginals(*other, [0, 100, 258], [258, 100, 7])
        e.pgo_marginals(*g, [0, 40], [63, 3])
        assert same(before, solves(e))
    finally:
        e.close(); twin.close()


def test_sharded_engine_equals_plain(eng):
    g = pg.two_robot_graph()
    b = _columns("adjacent")[:5, :1].repeat(64, 1) * np.arange(1, 65)[None, :, None]
    q = np.int32([0, 3, 35, 63, 12])
    sh = ScanContextEngine(initial_capacity=16, devices=[0, 0], exchange=1)
    try:
        assert _same(eng.pgo_solve_condensed_many(*g, 1e-5, b), sh.pgo_solve_condensed_many(*g, 1e-5, b))
        one, two = eng.pgo_marginals(*g, q, q[::-1].copy()), sh.pgo_marginals(*g, q, q[::-1].copy())
        assert _same(one[0], two[0]) and _same(one[1], two[1])
        with pytest.raises(SclError, match="256 distinct"):
            sh.pgo_marginals(*cc.step_case("hub257"), np.arange(257), np.arange(257))
    finally:
        sh.close()


def test_timing_is_reported_under_the_profile_switch(eng):
    g = cc.step_case("segment65")
    eng.profile_enable(1)
    try:
        eng.pgo_solve_condensed_many(*g, 1e-5, _columns("segment65"))
        lin_ms, solve_ms = eng.pgo_last_timing()
        parts = eng.pgo_condensed_last_timing()
        assert lin_ms > 0.0 and solve_ms > 0.0 and all(p > 0.0 for p in parts) and sum(parts) <= solve_ms * (1 + 1e-6)
        eng.pgo_marginals(*g, [0, 30], [66, 31])
        assert min(eng.pgo_last_timing()) > 0.0 and all(p > 0.0 for p in eng.pgo_condensed_last_timing())
    finally:
        eng.profile_enable(0)
