"""The checker and the named inputs of the marginal covariances of the pose-graph solve (include/scl_engine.h "POSE-GRAPH SOLVE, MANY
RIGHT-HAND SIDES AND MARGINAL COVARIANCES"), on top of tests/pgo_cases.py and tests/pgo_condensed_cases.py.

  sigma_numpy(lin)            Sigma = inv(hessian(lin, 0)) by LAPACK's Cholesky and one triangular solve (6 n x 6 n, dense)
  rel_numpy(Sigma, X, i, j)   rel = Sigma_jj - A Sigma_ij - (A Sigma_ij)^T + A Sigma_ii A^T, A = Ad((X_i^-1 X_j)^-1), float64
  exact(g)                    the same two at 40 digits (mpmath) from the unrounded linearisation, for graphs of <= 16 poses:
                              (Sigma rounded to float64, rel(i, j) -> 6 x 6 rounded to float64)
  dev_block / dev_rel         the deviation measures below

The deviation measure.  dev = max_ab |got_ab - want_ab| / sqrt(S_aa S_bb): for a block Sigma[i, j] S_aa is the diagonal entry a of pose
i's own marginal block and S_bb entry b of pose j's -- correlation-scaled, so that rotations (1e-4 rad^2) and translations (m^2) weigh
alike.  For rel the same against rel's own diagonal.

TAU_MARG, TAU_REL.  16 x the largest dev of the numpy restatement against the 40-digit one over SMALL_CASES (every block and every rel of
every ordered pair of poses), measured on the CPU and pinned here with the measured value beside it; 16 is the project's factor for
another order of the same operations, as TAU_STEP has it.  test_pgo_marginal_cases.py measures again and holds the pin to it."""
import functools

import mpmath
import numpy as np
import scipy.linalg as sla

import pcm_cases as pc
import pgo_cases as pg
import pgo_condensed_cases as cc

# measured on the CPU (test_pgo_marginal_cases.py prints each), (blocks, rel): ring16 7.40e-15, 1.16e-14; hand3 1.91e-15, 1.91e-15; hand4
# 4.45e-15, 4.51e-15; two_robots_cut 1.14e-14, 1.53e-14.  The largest of each, rounded up to one digit:
MEASURED_MARG = 2e-14
MEASURED_REL = 2e-14
TAU_MARG = 16 * MEASURED_MARG
TAU_REL = 16 * MEASURED_REL
# The factor, raised for the blocks of the two 257-pose graphs that are held to the NUMPY restatement (anchored_graph(257), hub257).  The
# pin was measured where cond(H) <= 3e5; these have 1.4e7 and 1.0e10, and an inverse's error grows with it.  There the float64 reference is
# itself 2.6e-13 and 2.2e-13 (13 and 11 x MEASURED_MARG) off two steps of Newton-Schulz refinement of it in extended precision, measured on
# the CPU -- most of TAU_MARG gone before the device is looked at.  The device measured 2.9e-13 and 6.2e-13 against it on an MI355X:
# within a further factor 16 of the bound, which by the rule of this file's issue is recorded (PGO marginals) and
# answered by a larger factor with the reason stated, not by silence: 64 = 16 for another order of the operations x 4 for a reference
# that is no better than the device.  rel on the same graphs stays at TAU_REL.
TAU_MARG_NUMPY_257 = 64 * MEASURED_MARG


def known_answer_bound(tau, restatement_dev):
    """The bound of a known answer on an exact chain: TAU, or 16 x the numpy restatement's own deviation from the hand-derived answer on
    that very query where that is larger -- TAU's definition applied to the case at hand.  The pins were measured on graphs of <= 16
    poses (cond(H) <= 3e5).  On the 65-pose chain cond(H) is 6e7, and rel between two late poses is a difference of terms far larger
    than itself: there the restatement is 9.5e-13 off f_cov (rel(63, 64)) and 1.8e-13 off the answer for rel(0, 2), against 3e-15 on the
    4-pose chain.  Formed from the CPU restatement and the hand-derived answer, never from the device's output."""
    return max(tau, 16.0 * restatement_dev)


# ---- float64 ---------------------------------------------------------------------------------------------------------------------------

def sigma_numpy(lin):
    H = pg.hessian(lin, 0.0).toarray()
    Li = sla.solve_triangular(np.linalg.cholesky(H), np.eye(H.shape[0]), lower=True)
    return Li.T @ Li


def block(Sigma, i, j):
    return Sigma[6 * i:6 * i + 6, 6 * j:6 * j + 6]


def adjoint_inverse_between(X, i, j):
    """Ad(h^-1) for h = X_i^-1 X_j, h^-1 formed as the linearisation forms it: X_j^-1 X_i with the translations' difference first"""
    return pc.adjoint(pg._rel(X[j:j + 1], X[i:i + 1]))[0]


def rel_numpy(Sigma, X, i, j):
    if i == j:
        return np.zeros((6, 6))
    A = adjoint_inverse_between(X, i, j)
    M = A @ block(Sigma, i, j)
    return block(Sigma, j, j) - M - M.T + A @ block(Sigma, i, i) @ A.T


def dev_block(got, want, Sigma, i, j):
    s = np.sqrt(np.outer(np.diag(block(Sigma, i, i)), np.diag(block(Sigma, j, j))))
    return float((np.abs(np.asarray(got) - want) / s).max())


def dev_rel(got, want):
    d = np.diag(want)
    return float((np.abs(np.asarray(got) - want) / np.sqrt(np.outer(d, d))).max())


# ---- mpmath, 40 digits -----------------------------------------------------------------------------------------------------------------

def _m_hessian(lin):
    N = 6 * lin.n
    H = mpmath.zeros(N, N)
    for i, j, y, Ai, Aj in lin.facs:
        for (p, A), (q, B) in [((j, Aj), (j, Aj))] + ([] if Ai is None else [((i, Ai), (i, Ai)), ((i, Ai), (j, Aj)), ((j, Aj), (i, Ai))]):
            for a in range(6):
                for b in range(6):
                    H[6 * p + a, 6 * q + b] += sum(A[m][a] * B[m][b] for m in range(6))
    return H


def exact(g, poses=None):
    """(Sigma[6 n, 6 n], rel[n, n, 6, 6]) at 40 digits, rounded to float64"""
    rows = g.poses if poses is None else poses
    n = len(rows)
    assert n <= pg.EXACT_POSES
    with mpmath.workdps(40):
        X = [pg._m_pose(row) for row in rows]
        S = mpmath.inverse(_m_hessian(pg._m_linearize(g, X)))
        zero = mpmath.mpf(0)
        blk = lambda i, j: [[S[6 * i + a, 6 * j + b] for b in range(6)] for a in range(6)]
        T = lambda M: [[M[b][a] for b in range(6)] for a in range(6)]
        rel = np.zeros((n, n, 6, 6))
        for i in range(n):
            for j in range(n):
                if i == j:
                    continue
                q, t = pg._m_rel(X[j], X[i])
                R = pc._mq_mat(q)
                K = [[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]
                B = pc._m_mul(K, R)
                A = [R[a] + [zero] * 3 for a in range(3)] + [B[a] + R[a] for a in range(3)]
                M = pc._m_mul(A, blk(i, j))
                N = pc._m_mul(pc._m_mul(A, blk(i, i)), T(A))
                Sjj = blk(j, j)
                rel[i, j] = [[float(Sjj[a][b] - M[a][b] - M[b][a] + N[a][b]) for b in range(6)] for a in range(6)]
        Sigma = np.array([[float(S[a, b]) for b in range(6 * n)] for a in range(6 * n)])
    return Sigma, rel


# ---- the inputs --------------------------------------------------------------------------------------------------------------------------

def two_robots_cut():
    """the first 8 poses of each robot of pg.two_robot_graph (16 poses) with the factors among them: two chains and the loop 3 - 35"""
    g = pg.two_robot_graph()
    keep = np.r_[0:8, 32:40]
    new = {int(p): k for k, p in enumerate(keep)}
    sel = [k for k in range(len(g.f_i)) if int(g.f_i[k]) in new and int(g.f_j[k]) in new]
    return pg.graph(g.poses[keep], [new[int(g.f_i[k])] for k in sel], [new[int(g.f_j[k])] for k in sel], g.f_z[sel], g.f_cov[sel],
                    g.p_idx, g.p_z, g.p_cov)


def exact_chain(n, seed=None):
    """a loop-free chain of n poses under one prior at pose 0 whose measurements are the true relative poses, at the chained odometry:
    every residual is zero up to the rounding of the chaining, so every D(E) = I"""
    rs = np.random.RandomState(9700 + n if seed is None else seed)
    return pg.chain_graph(rs, pg.trajectory(rs, n), exact=True)


_SMALL = {
    "ring16": pg.ring16,
    "hand3": lambda: cc.hand_case(3)[0],
    "hand4": lambda: cc.hand_case(4)[0],
    "two_robots_cut": two_robots_cut,
}
SMALL_CASES = tuple(_SMALL)


@functools.lru_cache(maxsize=None)
def small_case(name):
    """the named graph; treat as read-only"""
    return _SMALL[name]()


@functools.lru_cache(maxsize=None)
def small_exact(name):
    return exact(small_case(name))


@functools.lru_cache(maxsize=None)
def small_numpy(name):
    """(Sigma, X normalised) of the numpy restatement"""
    g = small_case(name)
    return sigma_numpy(pg.linearize_numpy(g)), pc._normalised(g.poses)


def restatement_deviations(name):
    """(the largest dev_block, the largest dev_rel) of the numpy restatement against the 40-digit one over all ordered pairs"""
    Se, rel_e = small_exact(name)
    Sn, X = small_numpy(name)
    n = len(X)
    dm = max(dev_block(block(Sn, i, j), block(Se, i, j), Se, i, j) for i in range(n) for j in range(n))
    dr = max(dev_rel(rel_numpy(Sn, X, i, j), rel_e[i, j]) for i in range(n) for j in range(n) if i != j)
    return dm, dr


# ---- known answers, derived by hand --------------------------------------------------------------------------------------------------------
# On a loop-free chain with exact measurements (zero residuals: every D(E) = I) under one prior at pose p:
#   * Sigma[p, p] = p_cov.  The prior's pose is a cut vertex: everything else hangs off it with no information of its own about where the
#     chain lies, so marginalising it out leaves the prior's information alone.
#   * rel(k, k + 1) = f_cov[k].  With xi_rel = xi_{k+1} - Ad(z^-1) xi_k the factor k says xi_rel ~ N(0, f_cov[k]), and on a tree nothing
#     else constrains it.
#   * rel(0, 2) = Ad(z_1^-1) f_cov[0] Ad(z_1^-1)^T + f_cov[1]: h_02 = h_01 h_12, the right perturbation of the product is
#     Ad(h_12^-1) xi_01 + xi_12 with the two independent, and h_12 = z_1.

def known_prior_block(g):
    return pc._sym(g.p_cov)[0]


def known_rel_step(g, k):
    return pc._sym(g.f_cov)[k]


def known_rel_02(g):
    z1 = pc._normalised(g.f_z[1:2])
    A = pc.adjoint(pc.inverse(z1))[0]
    cov = pc._sym(g.f_cov)
    return A @ cov[0] @ A.T + cov[1]
