"""The checker and the named inputs of the condensed direct step of the pose-graph solve (include/scl_engine.h "POSE-GRAPH SOLVE,
CONDENSED DIRECT STEP"), on top of tests/pgo_cases.py.

  classify(n, f_i, f_j, p_idx)    (junctions, segments): the contract's interior / junction rule, segments as (a, b)
  path_levels(m)                  the order in which a path of m nodes is reduced: per level a list of (node, left, right)
  condensed_system(lin, lam)      (junctions, segments, S, rhs, back): every segment eliminated by block cyclic reduction, S over the
                                  junctions assembled densely; back(delta_J) walks the levels back and returns delta (n, 6)
  solve_condensed(lin, lam)       delta (n, 6): the step, S factored by np.linalg.cholesky
  backward_error(lin, lam, d)     max over rows of |(H + lam diag H) d + g| / (|H + lam diag H| |d| + |g|), the absolute matrix being
                                  pgo_cases.hessian_majorant

It restates the contract in numpy: dense 6 x 6 inverses by np.linalg.solve where the device uses a Cholesky factor, numpy's products
(another order inside every 6 x 6 product), LAPACK's Cholesky for S and two substitutions with its factor (a general solve with that
factor pivots, and then loses the row scaling a prior of 1e6 next to odometry of 1e2 needs: 1e-12 instead of 1e-15).

TAU_STEP.  A backward error does not grow with cond(H), so one number serves every size.  MEASURED is the largest backward error of
solve_condensed over STEP_CASES x LAMBDAS (test_pgo_condensed_cases.py prints each and pins the largest at MEASURED = TAU_STEP / 16);
TAU_STEP = 16 x MEASURED, the project's factor for another order inside the 6 x 6 products."""
import functools

import numpy as np
import scipy.linalg as sla

import pcm_cases as pc
import pgo_cases as pg

LAMBDAS = (1e-5, 10.0)
# measured: the largest is hub257 at lambda 1e-5 (a dense system of 1542 unknowns, no segment), 4.04e-15; drifting4097 7.3e-16, the
# chains 1-5e-16; rounded up to one digit
MEASURED = 5e-15
TAU_STEP = 16 * MEASURED
MAX_JUNCTIONS = 1024


def classify(n, f_i, f_j, p_idx):
    rows = [[] for _ in range(n)]
    for k, (a, b) in enumerate(zip(f_i, f_j)):
        rows[int(a)].append(int(b)); rows[int(b)].append(int(a))
    prior = set(int(p) for p in p_idx)
    interior = [k not in prior and sorted(rows[k]) == [k - 1, k + 1] for k in range(n)]
    junctions = [k for k in range(n) if not interior[k]]
    segments, k = [], 0
    while k < n:
        if interior[k]:
            b = k
            while interior[b + 1]:
                b += 1
            segments.append((k, b)); k = b + 1
        else:
            k += 1
    return junctions, segments


def path_levels(m):
    alive, levels = list(range(m)), []
    while len(alive) > 2:
        level, nxt = [], []
        for p, node in enumerate(alive):
            if p % 2 == 1 and p + 1 < len(alive):
                level.append((node, alive[p - 1], alive[p + 1]))
            else:
                nxt.append(node)
        levels.append(level); alive = nxt
    return levels


def _blocks(lin, lam):
    """(D[n,6,6] damped, the list over between factors of (i, j, W = A_i^T A_j))"""
    D = lin.diag.copy()
    idx = np.arange(6)
    D[:, idx, idx] += lam * D[:, idx, idx]
    W = np.einsum("kma,kmb->kab", lin.Ai[:lin.F], lin.Aj[:lin.F])
    return D, [(int(lin.fi[k]), int(lin.fj[k]), W[k]) for k in range(lin.F)]


def condensed_system(lin, lam):
    n = lin.n
    D, facs = _blocks(lin, lam)
    junctions, segments = classify(n, lin.fi[:lin.F], lin.fj[:lin.F], lin.fj[lin.F:])
    jof = {p: j for j, p in enumerate(junctions)}
    nJ = len(junctions)
    S = np.zeros((6 * nJ, 6 * nJ)); rhs = np.zeros(6 * nJ)
    for j, p in enumerate(junctions):
        S[6 * j:6 * j + 6, 6 * j:6 * j + 6] = D[p]; rhs[6 * j:6 * j + 6] = -lin.grad[p]
    coupling = {}                                           # (p, p + 1) -> the block H(p, p + 1) of an odometry step next to an interior pose
    for i, j, W in facs:
        if i in jof and j in jof:
            a, b = jof[i], jof[j]
            S[6 * a:6 * a + 6, 6 * b:6 * b + 6] += W; S[6 * b:6 * b + 6, 6 * a:6 * a + 6] += W.T
        else:
            coupling[(min(i, j), max(i, j))] = W if i < j else W.T
    store = []
    for a, b in segments:
        m = b - a + 3
        pose = lambda t: a - 1 + t
        Dn = [np.zeros((6, 6))] + [D[pose(t)].copy() for t in range(1, m - 1)] + [np.zeros((6, 6))]
        bn = [np.zeros(6)] + [-lin.grad[pose(t)].copy() for t in range(1, m - 1)] + [np.zeros(6)]
        U = [coupling[(pose(t), pose(t) + 1)].copy() for t in range(m - 1)] + [None]
        levels = path_levels(m)
        kept = []
        for level in levels:
            left, right = {}, {}
            for node, l, r in level:
                A, B = U[l], U[node]
                X = np.linalg.solve(Dn[node], np.concatenate([A.T, B, bn[node][:, None]], 1))        # D^-1 [A^T, B, b]
                right[l] = (-A @ X[:, :6], -A @ X[:, 12])
                left[r] = (-B.T @ X[:, 6:12], -B.T @ X[:, 12])
                U[l] = -A @ X[:, 6:12]
                kept.append((node, l, r, X))
            for t in sorted(set(left) | set(right)):        # a survivor takes its left contribution, then its right
                for side in (left, right):
                    if t in side:
                        Dn[t] = Dn[t] + side[t][0]; bn[t] = bn[t] + side[t][1]
        ja, jb = jof[a - 1], jof[b + 1]
        S[6 * ja:6 * ja + 6, 6 * ja:6 * ja + 6] += Dn[0]; S[6 * jb:6 * jb + 6, 6 * jb:6 * jb + 6] += Dn[m - 1]
        S[6 * ja:6 * ja + 6, 6 * jb:6 * jb + 6] += U[0]; S[6 * jb:6 * jb + 6, 6 * ja:6 * ja + 6] += U[0].T
        rhs[6 * ja:6 * ja + 6] += bn[0]; rhs[6 * jb:6 * jb + 6] += bn[m - 1]
        store.append((a, m, kept))

    def back(dJ):
        delta = np.zeros((n, 6))
        delta[junctions] = dJ.reshape(-1, 6)
        for a, m, kept in store:
            x = {0: delta[a - 1], m - 1: delta[a - 2 + m]}
            for node, l, r, X in reversed(kept):
                x[node] = X[:, 12] - X[:, :6] @ x[l] - X[:, 6:12] @ x[r]
                delta[a - 1 + node] = x[node]
        return delta
    return junctions, segments, S, rhs, back


def solve_condensed(lin, lam):
    _, _, S, rhs, back = condensed_system(lin, lam)
    L = np.linalg.cholesky(S)
    return back(sla.solve_triangular(L.T, sla.solve_triangular(L, rhs, lower=True), lower=False))


def backward_error(lin, lam, delta):
    H, Hm = pg.hessian(lin, lam), pg.hessian_majorant(lin, lam)
    d, g = np.asarray(delta, np.float64).ravel(), lin.grad.ravel()
    return float((np.abs(H @ d + g) / (Hm @ np.abs(d) + np.abs(g))).max())


def lm_condensed(g, params=None):
    """pgo_cases.lm_numpy with solve_condensed in place of scipy's sparse solve"""
    def solve(lin, lam):
        d = solve_condensed(lin, lam)
        return d, float(np.abs(d).max())
    X, info = pg._lm(pc._normalised(g.poses), params, lambda X: pg.linearize_numpy(g, X), solve, pg.retract,
                     lambda a, b: a < b, lambda a, b: a <= b, lambda a, b: a - b)
    return pg.canonical(X), info


# ---- the inputs --------------------------------------------------------------------------------------------------------------------------

def plain_chain(n, seed=None, loops=()):
    """n poses of drifting odometry under one prior at pose 0 (no loops: poses 0 and n - 1 are the junctions, n - 2 interior poses).
    Started from the truth behind a perturbation, not from the chained odometry: there every residual of a loop-free chain is zero, the
    gradient is rounding and a backward error relative to |g| says nothing"""
    rs = np.random.RandomState(9000 + n if seed is None else seed)
    return pg.chain_graph(rs, pg.trajectory(rs, n), loops=list(loops), start_noise=0.02)


def reversed_chain(n=12):
    """every odometry factor the other way round: f_i = k + 1, f_j = k, the measurement inverted"""
    g = plain_chain(n, seed=9100)
    return g._replace(f_i=g.f_j.copy(), f_j=g.f_i.copy(), f_z=np.array([pc.inverse(z[None])[0] for z in g.f_z]))


def duplicate_chain(n=12, at=5):
    """odometry factor `at` twice: poses at and at + 1 become junctions"""
    g = plain_chain(n, seed=9200)
    rs = np.random.RandomState(9201)
    return g._replace(f_i=np.append(g.f_i, g.f_i[at]).astype(np.int32), f_j=np.append(g.f_j, g.f_j[at]).astype(np.int32),
                      f_z=np.vstack([g.f_z, g.f_z[at:at + 1]]), f_cov=np.vstack([g.f_cov, pg.odom_cov(rs).reshape(1, 36)]))


def mid_prior_chain(n=12, at=6):
    g = plain_chain(n, seed=9300)
    cov = np.diag([1e-3] * 3 + [1e-2] * 3).reshape(1, 36)
    return g._replace(p_idx=np.int32([0, at]), p_z=np.vstack([g.p_z, g.poses[at:at + 1]]), p_cov=np.vstack([g.p_cov, cov]))


def adjacent_junctions_chain(n=12):
    """loops 3 - 8 and 4 - 9: junctions 3, 4 and 8, 9 lie next to each other with no segment between them"""
    return plain_chain(n, seed=9400, loops=[(3, 8), (9, 4)])


def many_junctions(n=MAX_JUNCTIONS + 1):
    """a chain of n poses each under a prior: n junctions, no segment"""
    g = plain_chain(n, seed=9500)
    cov = np.diag([1e-3] * 3 + [1e-2] * 3).reshape(1, 36)
    return g._replace(p_idx=np.arange(n, dtype=np.int32), p_z=g.poses.copy(), p_cov=np.tile(cov, (n, 1)))


SEGMENT_LENGTHS = (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 255, 256, 257)
_BUILD = {
    "one": lambda: pg.lin_case("one"),
    "two_poses": lambda: plain_chain(2),
    "reversed": reversed_chain,
    "duplicate": duplicate_chain,
    "mid_prior": mid_prior_chain,
    "adjacent": adjacent_junctions_chain,
    "two_robots": pg.two_robot_graph,
    "hub257": lambda: pg.hub_graph(257, 300),
    "planted": lambda: pg.planted_graph()[0],
    "chain4097": lambda: plain_chain(4097),
    "drifting4097": lambda: pg.drifting_graph(4097),
}
_BUILD.update({f"segment{L}": (lambda L=L: plain_chain(L + 2)) for L in SEGMENT_LENGTHS})
STEP_CASES = tuple(_BUILD)
# what the contract's rule makes of each: (junctions, segments, longest segment)
COUNTS = {"one": (1, 0, 0), "two_poses": (2, 0, 0), "reversed": (2, 1, 10), "duplicate": (4, 2, 4), "mid_prior": (3, 2, 5), "adjacent": (6, 3, 3),
          "two_robots": (11, 8, 12), "hub257": (257, 0, 0), "chain4097": (2, 1, 4095), "drifting4097": (240, None, None)}


@functools.lru_cache(maxsize=None)
def step_case(name):
    """the named graph; treat as read-only"""
    return _BUILD[name]()


@functools.lru_cache(maxsize=None)
def step_lin(name):
    return pg.linearize_numpy(step_case(name))


# ---- written out by hand ---------------------------------------------------------------------------------------------------------------

def hand_case(n):
    """a chain of 3 or 4 poses under one prior: (graph, junctions, segments, S(lin, lam) written out).  Pose 0 and the last pose are the
    junctions; S is the Schur complement on them, with the inverse of the interior written as such"""
    g = plain_chain(n, seed=9600 + n)

    def S_of(lin, lam):
        D, facs = _blocks(lin, lam)
        U = {(i, j): W for i, j, W in facs}                 # f_i < f_j here: W is the block (i, j)
        inv = np.linalg.inv
        if n == 3:
            Di = inv(D[1])
            return np.block([[D[0] - U[0, 1] @ Di @ U[0, 1].T, -U[0, 1] @ Di @ U[1, 2]],
                             [-U[1, 2].T @ Di @ U[0, 1].T, D[2] - U[1, 2].T @ Di @ U[1, 2]]])
        Mi = inv(np.block([[D[1], U[1, 2]], [U[1, 2].T, D[2]]]))
        C = np.block([[U[0, 1], np.zeros((6, 6))], [np.zeros((6, 6)), U[2, 3].T]])     # rows: poses 0 and 3; columns: poses 1 and 2
        return np.block([[D[0], np.zeros((6, 6))], [np.zeros((6, 6)), D[3]]]) - C @ Mi @ C.T
    return g, [0, n - 1], [(1, n - 2)], S_of
