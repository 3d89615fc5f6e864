"""The checkers and the named inputs of the pairwise consistency of loop closures (include/scl_engine.h "PAIRWISE CONSISTENCY OF LOOP
CLOSURES").

  d2_exact(case)        the definition in mpmath at 40 digits on the float64 inputs: the n x n matrix rounded to float64, +inf where a
                        pivot of the factorisation is not > 0
  d2_numpy(case)        a vectorised float64 restatement over all pairs (dense 6 x 6 adjoints, another order of every product than the
                        device's); d2_numpy_pairs(case, I, J) for chosen pairs
  graph(d2, threshold)  the n x n bool adjacency: d2 <= threshold off the diagonal
  greedy_clique(adj)    the contract's greedy maximum clique on Python integers as bit sets: (members ascending, seed)
  greedy_clique_fast(adj)  the same answer with the counts kept from step to step in numpy (test_pcm_cases.py holds it to greedy_clique):
                        what the large graphs are checked with
  max_clique_brute(adj) the exact maximum clique's size, n <= 24

case(family, n) -> Case, seeded.  Two trajectories of 1 m steps with a true transform between their world frames; every loop sits
between two random keyframes.  60 % of the loops (at least two) are inliers: the true relative pose behind a right perturbation drawn
from the loop's own covariance at `scale`; the others are gross outliers (3 m and 0.5 rad off, then the same noise).
  planted   scale 0.6   every pair of inliers is consistent at THRESHOLD (test_pcm_cases.py asserts it of the checker), so the clique
                        is the planted set
  mixed     scale 1.0   correctly modelled noise: a good part of the inlier pairs is not consistent at THRESHOLD
  far       scale 1.0   both trajectories 2 km from their origins -- used for the numeric tolerance
Every family is re-drawn, loop by loop, until no pair's d2 -- d2_exact for n <= EXACT_MAX, d2_numpy above -- lies within relative
KNIFE_EDGE of THRESHOLD; Case.gap is the relative distance of the closest pair that remained.  No pair is ever excluded from a comparison.

TAU[family]: the relative tolerance |d2 - d2_exact| <= TAU * max(1, d2_exact) the GPU tests hold the device to.  It is 16 x the largest
deviation of d2_numpy from d2_exact over the family's cases of n = 2, 3, 40, measured, written down below and pinned by
test_pcm_cases.py (which asserts that the restatement still stays within TAU / 16).  The factor 16 covers what separates the device
from numpy -- another atan2 / sqrt of a few ulp and another order inside the 6 x 6 products --, each of the order of the restatement's
own rounding."""
import functools
from collections import namedtuple

import mpmath
import numpy as np

THRESHOLD = 7.8408           # chi-square, 6 degrees of freedom, 0.75
KNIFE_EDGE = 1e-6
EXACT_MAX = 64
FAMILIES = {"planted": 0.6, "mixed": 1.0, "far": 1.0}
SMALL_N = (2, 3, 40)
ODOM_VAR = (1e-9, 1e-9, 1e-9, 1e-7, 1e-7, 1e-7)
# largest deviations measured over n = 2, 3, 40: planted 4.46e-12, mixed 3.09e-12, far 1.76e-11; times 16 (7.14e-11, 4.94e-11, 2.81e-10),
# rounded up to one digit
TAU = {"planted": 8e-11, "mixed": 5e-11, "far": 3e-10}

Case = namedtuple("Case", "poses_a poses_b idx_a idx_b z cov odom_var threshold inlier gap")


# ---- float64, vectorised ------------------------------------------------------------------------------------------------------------

def qmul(a, b):
    ax, ay, az, aw = np.moveaxis(a, -1, 0); bx, by, bz, bw = np.moveaxis(b, -1, 0)
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], -1)


def qconj(a):
    return a * np.array([-1.0, -1.0, -1.0, 1.0])


def qmat(q):
    x, y, z, w = np.moveaxis(q, -1, 0)
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                  2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)
    return R.reshape(q.shape[:-1] + (3, 3))


def rotvec_to_quat(r):
    r = np.asarray(r, np.float64)
    th = np.linalg.norm(r, axis=-1, keepdims=True)
    k = np.where(th > 1e-12, np.sin(th / 2) / np.where(th > 1e-12, th, 1.0), 0.5)
    return np.concatenate([k * r, np.cos(th / 2)], -1)


def compose(p1, p2):
    """(n,7) poses x, y, z, qx, qy, qz, qw (unit quaternions): p1 p2"""
    q = qmul(p1[..., 3:], p2[..., 3:])
    t = p1[..., :3] + np.einsum("...ij,...j->...i", qmat(p1[..., 3:]), p2[..., :3])
    return np.concatenate([t, q], -1)


def inverse(p):
    qi = qconj(p[..., 3:])
    return np.concatenate([-np.einsum("...ij,...j->...i", qmat(qi), p[..., :3]), qi], -1)


def _normalised(p):
    p = np.array(p, np.float64)
    p[..., 3:] /= np.sqrt((p[..., 3:] ** 2).sum(-1, keepdims=True))
    return p


def _skew(t):
    o = np.zeros(t.shape[:-1] + (3, 3))
    o[..., 0, 1], o[..., 0, 2], o[..., 1, 0], o[..., 1, 2], o[..., 2, 0], o[..., 2, 1] = -t[..., 2], t[..., 1], t[..., 2], -t[..., 0], -t[..., 1], t[..., 0]
    return o


def adjoint(p):
    R = qmat(p[..., 3:])
    A = np.zeros(p.shape[:-1] + (6, 6))
    A[..., :3, :3] = R; A[..., 3:, 3:] = R
    A[..., 3:, :3] = _skew(p[..., :3]) @ R
    return A


def _sym(cov):
    c = np.asarray(cov, np.float64).reshape(-1, 6, 6)
    u = np.triu(c)
    return u + np.swapaxes(np.triu(c, 1), -1, -2)                              # only the upper triangle is read


def d2_numpy_pairs(case, I, J):
    """d2 of the pairs (I[k], J[k]), I[k] < J[k]"""
    I = np.asarray(I); J = np.asarray(J)
    pa, pb, z = _normalised(case.poses_a), _normalised(case.poses_b), _normalised(case.z)
    S = _sym(case.cov)
    ai, aj, bi, bj = case.idx_a[I], case.idx_a[J], case.idx_b[I], case.idx_b[J]

    def rel(p, f, t):                                                          # (X_f)^-1 X_t
        qf = qconj(p[f, 3:])
        return np.concatenate([np.einsum("...ij,...j->...i", qmat(qf), p[t, :3] - p[f, :3]), qmul(qf, p[t, 3:])], -1)
    TA, TB, TBi = rel(pa, ai, aj), rel(pb, bj, bi), rel(pb, bi, bj)
    E = compose(compose(compose(TA, z[J]), TB), inverse(z[I]))
    M = compose(z[I], TBi)
    q = E[:, 3:] * np.where(E[:, 6:7] < 0, -1.0, 1.0)
    nv = np.sqrt((q[:, :3] ** 2).sum(-1))
    k = np.where(nv == 0, 2.0, 2.0 * np.arctan2(nv, q[:, 3]) / np.where(nv == 0, 1.0, nv))
    r = np.concatenate([k[:, None] * q[:, :3], E[:, :3]], -1)
    Ai, Am = adjoint(z[I]), adjoint(M)
    steps = np.abs(ai.astype(np.float64) - aj) + np.abs(bi.astype(np.float64) - bj)
    odom = np.zeros(6) if case.odom_var is None else np.asarray(case.odom_var, np.float64)
    Sig = Ai @ S[I] @ np.swapaxes(Ai, -1, -2) + Am @ S[J] @ np.swapaxes(Am, -1, -2)
    Sig[:, range(6), range(6)] += odom[None, :] * steps[:, None]
    # Cholesky from the upper triangle, column by column; a pivot that is not > 0: +inf
    m = len(I)
    L = np.zeros((m, 6, 6)); ok = np.ones(m, bool); y = np.zeros((m, 6))
    with np.errstate(invalid="ignore", divide="ignore"):
        for c in range(6):
            s = Sig[:, c, c] - (L[:, c, :c] ** 2).sum(-1)
            ok &= s > 0
            L[:, c, c] = np.sqrt(s)
            for rr in range(c + 1, 6):
                L[:, rr, c] = (Sig[:, c, rr] - (L[:, rr, :c] * L[:, c, :c]).sum(-1)) / L[:, c, c]
        for a in range(6):
            y[:, a] = (r[:, a] - (L[:, a, :a] * y[:, :a]).sum(-1)) / L[:, a, a]
    return np.where(ok, (y ** 2).sum(-1), np.inf)


def d2_numpy(case, chunk=200000):
    n = len(case.idx_a)
    I, J = np.triu_indices(n, 1)
    out = np.zeros((n, n))
    for s in range(0, len(I), chunk):
        v = d2_numpy_pairs(case, I[s:s + chunk], J[s:s + chunk])
        out[I[s:s + chunk], J[s:s + chunk]] = v
        out[J[s:s + chunk], I[s:s + chunk]] = v
    return out


def graph(d2, threshold):
    with np.errstate(invalid="ignore"):
        g = np.asarray(d2) <= threshold
    np.fill_diagonal(g, False)
    return g


# ---- mpmath, 40 digits ---------------------------------------------------------------------------------------------------------------

def _mq_mul(a, b):
    return [a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0],
            a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]]


def _mq_mat(q):
    x, y, z, w = q
    return [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
            [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
            [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]


def _m_pose(row):
    """(R, t, q) of a float64 pose row, the quaternion normalised at 40 digits"""
    v = [mpmath.mpf(float(x)) for x in row]
    s = mpmath.sqrt(v[3] ** 2 + v[4] ** 2 + v[5] ** 2 + v[6] ** 2)
    q = [c / s for c in v[3:]]
    return _mq_mat(q), v[:3], q


def _m_mul(A, B):
    return [[sum(A[i][k] * B[k][j] for k in range(len(B))) for j in range(len(B[0]))] for i in range(len(A))]


def _m_T(A):
    return [list(r) for r in zip(*A)]


def _m_compose(p1, p2):
    R1, t1, q1 = p1; R2, t2, q2 = p2
    return _m_mul(R1, R2), [t1[i] + sum(R1[i][k] * t2[k] for k in range(3)) for i in range(3)], _mq_mul(q1, q2)


def _m_inverse(p):
    R, t, q = p
    Rt = _m_T(R)
    return Rt, [-sum(Rt[i][k] * t[k] for k in range(3)) for i in range(3)], [-q[0], -q[1], -q[2], q[3]]


def _m_adjoint(p):
    R, t, _ = p
    K = [[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]
    B = _m_mul(K, R)
    z3 = [mpmath.mpf(0)] * 3
    return [R[i] + z3 for i in range(3)] + [B[i] + R[i] for i in range(3)]


def _m_pair(pa, pb, zs, Ss, SA, odom, ai, aj, bi, bj, i, j):
    TA = _m_compose(_m_inverse(pa[ai]), pa[aj])
    TB = _m_compose(_m_inverse(pb[bj]), pb[bi])
    E = _m_compose(_m_compose(_m_compose(TA, zs[j]), TB), _m_inverse(zs[i]))
    M = _m_compose(zs[i], _m_inverse(TB))
    q = E[2] if E[2][3] >= 0 else [-c for c in E[2]]
    nv = mpmath.sqrt(q[0] ** 2 + q[1] ** 2 + q[2] ** 2)
    k = mpmath.mpf(2) if nv == 0 else 2 * mpmath.atan2(nv, q[3]) / nv
    r = [k * q[0], k * q[1], k * q[2]] + list(E[1])
    Am = _m_adjoint(M)
    SM = _m_mul(_m_mul(Am, Ss[j]), _m_T(Am))
    steps = abs(ai - aj) + abs(bi - bj)
    Sig = [[SA[i][a][b] + SM[a][b] + (odom[a] * steps if a == b else 0) for b in range(6)] for a in range(6)]
    L = [[mpmath.mpf(0)] * 6 for _ in range(6)]
    for c in range(6):
        s = Sig[c][c] - sum(L[c][k2] ** 2 for k2 in range(c))
        if not s > 0:
            return float("inf")
        L[c][c] = mpmath.sqrt(s)
        for rr in range(c + 1, 6):
            L[rr][c] = (Sig[c][rr] - sum(L[rr][k2] * L[c][k2] for k2 in range(c))) / L[c][c]
    y = []
    for a in range(6):
        y.append((r[a] - sum(L[a][k2] * y[k2] for k2 in range(a))) / L[a][a])
    return float(sum(v * v for v in y))


def d2_exact(case, only=None):
    """the n x n matrix of the definition at 40 digits; only: the loops whose rows and columns are wanted (the rest stays 0)"""
    n = len(case.idx_a)
    out = np.zeros((n, n))
    with mpmath.workdps(40):
        pa = {k: _m_pose(case.poses_a[k]) for k in set(case.idx_a.tolist())}
        pb = {k: _m_pose(case.poses_b[k]) for k in set(case.idx_b.tolist())}
        zs = [_m_pose(row) for row in case.z]
        sym = _sym(case.cov)
        Ss = [[[mpmath.mpf(float(v)) for v in row] for row in S] for S in sym]
        SA = []
        for i in range(n):
            A = _m_adjoint(zs[i])
            SA.append(_m_mul(_m_mul(A, Ss[i]), _m_T(A)))
        odom = [mpmath.mpf(0)] * 6 if case.odom_var is None else [mpmath.mpf(float(v)) for v in case.odom_var]
        for i in range(n):
            for j in range(i + 1, n):
                if only is not None and i not in only and j not in only:
                    continue
                out[i, j] = out[j, i] = _m_pair(pa, pb, zs, Ss, SA, odom, int(case.idx_a[i]), int(case.idx_a[j]),
                                                int(case.idx_b[i]), int(case.idx_b[j]), i, j)
    return out


# ---- the clique -------------------------------------------------------------------------------------------------------------------------

def _rows(adj):
    a = np.asarray(adj, bool)
    return [int.from_bytes(np.packbits(row, bitorder="little").tobytes(), "little") for row in a]


def greedy_clique(adj):
    """(members ascending, seed) of the contract; ((), -1) for no vertex"""
    rows = _rows(adj)
    best, seed = (), -1
    for s in range(len(rows)):
        C, P = [s], rows[s]
        while P:
            top, u, m = -1, -1, P
            while m:
                v = (m & -m).bit_length() - 1
                m &= m - 1
                c = bin(rows[v] & P).count("1")
                if c > top:
                    top, u = c, v
            C.append(u)
            P &= rows[u]
        if len(C) > len(best):
            best, seed = tuple(sorted(C)), s
    return best, seed


def greedy_clique_fast(adj):
    """greedy_clique's answer for large graphs: cnt[v] = |adj[v] & P| starts as the seed's row of adj @ adj and loses |adj[v] & R| for the
    set R a step removes (or is counted anew over P', whichever is smaller); a seed whose degree + 1 does not exceed the best so far is
    passed over -- seeds come in ascending order and a tie keeps the lower one, so it could not have replaced the answer"""
    ab = np.ascontiguousarray(np.asarray(adj, bool))
    n = len(ab)
    if n == 0:
        return (), -1
    a = ab.astype(np.uint8)
    f = ab.astype(np.float32)
    common = (f @ f).astype(np.int64)                                          # exact: every entry is an integer below 2^24
    deg = ab.sum(1)
    best, seed = (), -1
    for s in range(n):
        if deg[s] + 1 <= len(best):
            continue
        P = ab[s].copy(); cnt = common[s].copy(); C = [s]
        idx = np.flatnonzero(P)
        while idx.size:
            u = int(idx[np.argmax(cnt[idx])])                                  # the first of the largest: the lowest index
            C.append(u)
            keep = ab[u, idx]
            R, idx = idx[~keep], idx[keep]
            P = P & ab[u]
            if R.size <= idx.size:
                cnt -= a[R].sum(0, dtype=np.int64)
            else:
                cnt = a[idx].sum(0, dtype=np.int64)
        if len(C) > len(best):
            best, seed = tuple(sorted(C)), s
    return best, seed


def max_clique_brute(adj):
    rows = _rows(adj)
    assert len(rows) <= 24

    def grow(size, P):
        top = size
        while P:
            v = (P & -P).bit_length() - 1
            P &= P - 1
            top = max(top, grow(size + 1, P & rows[v]))
        return top
    return grow(0, (1 << len(rows)) - 1)


def is_clique(adj, members):
    a = np.asarray(adj, bool)
    m = list(members)
    return all(a[i, j] for i in m for j in m if i != j)


# name -> (n, edges, members, seed): the answers written by hand from the contract (greedy_misses: found by search, its exact maximum is 6)
HAND_GRAPHS = {
    # seed 0 has P = {1, 3}, both with no neighbour in P: the tie goes to 1
    "tie": (4, [(0, 1), (1, 2), (2, 3), (0, 3)], (0, 1), 0),
    # two triangles: the one seed 0 finds is as large as the one seed 1 finds, and keeps the answer
    "equal": (6, [(1, 3), (1, 5), (3, 5), (0, 2), (0, 4), (2, 4)], (0, 2, 4), 0),
    "greedy_misses": (16, [(0, 2), (0, 3), (0, 4), (0, 5), (0, 6), (0, 7), (0, 8), (0, 11), (0, 12), (0, 14), (0, 15), (1, 3), (1, 5), (1, 6),
                           (1, 7), (1, 8), (1, 9), (1, 11), (1, 12), (1, 13), (1, 14), (1, 15), (2, 3), (2, 4), (2, 5), (2, 6), (2, 7), (2, 8),
                           (2, 10), (2, 13), (2, 14), (2, 15), (3, 7), (3, 9), (3, 10), (3, 11), (3, 12), (3, 13), (3, 14), (3, 15), (4, 5),
                           (4, 6), (4, 7), (4, 10), (4, 13), (4, 14), (5, 6), (5, 8), (5, 10), (5, 11), (5, 12), (5, 14), (5, 15), (6, 8),
                           (6, 10), (6, 11), (6, 13), (6, 15), (7, 8), (7, 9), (7, 11), (7, 12), (7, 13), (7, 14), (8, 9), (8, 10), (9, 11),
                           (9, 13), (9, 15), (10, 11), (10, 13), (10, 14), (10, 15), (11, 12), (11, 14), (12, 13), (12, 15), (13, 14),
                           (13, 15), (14, 15)], (0, 2, 4, 5, 6), 0),
    "empty": (5, [], (0,), 0),
    "across_63_64": (70, [(i, j) for i in range(62, 67) for j in range(i + 1, 67)], (62, 63, 64, 65, 66), 62),
}
GREEDY_MISSES_EXACT = 6


def graph_from_edges(n, edges):
    a = np.zeros((n, n), bool)
    for i, j in edges:
        a[i, j] = a[j, i] = True
    return a


# ---- the inputs --------------------------------------------------------------------------------------------------------------------------

def random_walk(rs, n, origin):
    """n poses, steps of about 1 m along the heading, which wanders"""
    poses = np.zeros((n, 7)); cur = np.concatenate([origin, rotvec_to_quat(rs.uniform(-0.2, 0.2, 3))])
    for k in range(n):
        poses[k] = cur
        step = np.concatenate([[rs.uniform(0.8, 1.2), 0.0, 0.0], rotvec_to_quat(rs.normal(0, [0.02, 0.02, 0.08]))])
        cur = compose(cur, step)
        cur[3:] /= np.linalg.norm(cur[3:])
    return poses


def random_cov(rs):
    sig = np.concatenate([rs.uniform(0.004, 0.008, 3), rs.uniform(0.03, 0.08, 3)])
    s = rs.choice([-1.0, 1.0], 6)
    return np.diag(sig) @ (0.7 * np.eye(6) + 0.3 * np.outer(s, s)) @ np.diag(sig)    # correlations of +-0.3


def draw_loop(rs, pa, pb, T_ab, inlier, scale, n_a, n_b):
    """(idx_a, idx_b, z[7], cov[6,6]) of one loop"""
    a, b = int(rs.randint(n_a)), int(rs.randint(n_b))
    cov = random_cov(rs)
    true = compose(compose(inverse(pa[a]), T_ab), pb[b])
    xi = scale * (np.linalg.cholesky(cov) @ rs.standard_normal(6))
    z = true
    if not inlier:
        d = rs.standard_normal(3); d *= 3.0 / np.linalg.norm(d)
        w = rs.standard_normal(3); w *= 0.5 / np.linalg.norm(w)
        z = compose(z, np.concatenate([d, rotvec_to_quat(w)]))
    z = compose(z, np.concatenate([xi[3:], rotvec_to_quat(xi[:3])]))
    z[3:] /= np.linalg.norm(z[3:])
    return a, b, z, cov


def _near(d2, threshold):
    with np.errstate(invalid="ignore"):
        return np.abs(d2 - threshold) <= KNIFE_EDGE * threshold


def make_case(scale, n, seed, origin_a=(0.0, 0.0, 0.0), origin_b=(30.0, -20.0, 1.0), n_kf=200, same=False, odom_var=ODOM_VAR):
    rs = np.random.RandomState(seed)
    pa = random_walk(rs, n_kf, np.asarray(origin_a, np.float64))
    pb = pa if same else random_walk(rs, n_kf, np.asarray(origin_b, np.float64))
    T_ab = np.concatenate([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0]]) if same else \
        np.concatenate([rs.uniform(-20, 20, 3), rotvec_to_quat(rs.uniform(-0.5, 0.5, 3))])
    n_in = min(n, max(2, int(round(0.6 * n))))
    inlier = np.zeros(n, bool); inlier[rs.permutation(n)[:n_in]] = True
    loops = [draw_loop(rs, pa, pb, T_ab, inlier[i], scale, n_kf, n_kf) for i in range(n)]

    def build():
        return Case(pa, pb, np.array([l[0] for l in loops], np.int32), np.array([l[1] for l in loops], np.int32),
                    np.array([l[2] for l in loops]).reshape(n, 7), np.array([l[3] for l in loops]).reshape(n, 36),
                    None if odom_var is None else np.asarray(odom_var, np.float64), THRESHOLD, inlier, None)
    c = build()
    exact = n <= EXACT_MAX
    d2 = d2_exact(c) if exact else d2_numpy(c)
    for _ in range(1000):
        bad = np.argwhere(np.triu(_near(d2, THRESHOLD), 1))
        if len(bad) == 0:
            break
        redo = sorted(set(int(p[1]) for p in bad))                              # the later loop of every pair on the edge
        for j in redo:
            loops[j] = draw_loop(rs, pa, pb, T_ab, inlier[j], scale, n_kf, n_kf)
        c = build()
        if exact:
            part = d2_exact(c, only=set(redo))
            for j in redo:
                d2[j, :] = part[j, :]; d2[:, j] = part[:, j]
        else:
            for j in redo:
                o = np.array([k for k in range(n) if k != j])
                v = d2_numpy_pairs(c, np.minimum(o, j), np.maximum(o, j))
                d2[j, o] = v; d2[o, j] = v
    else:
        raise AssertionError("the knife edge could not be left")
    off = ~np.eye(n, dtype=bool)
    fin = np.isfinite(d2) & off
    gap = float(np.min(np.abs(d2[fin] - THRESHOLD) / THRESHOLD)) if fin.any() else float("inf")
    return c._replace(gap=gap), d2


@functools.lru_cache(maxsize=None)
def case_and_d2(family, n):
    """(Case, its checker matrix: d2_exact for n <= EXACT_MAX, d2_numpy above), computed once and shared; treat both as read-only"""
    far = family == "far"
    c, d2 = make_case(FAMILIES[family], n, seed=1000 * sorted(FAMILIES).index(family) + n,
                      origin_a=(2000.0, -1500.0, 30.0) if far else (0.0, 0.0, 0.0), origin_b=(1950.0, -1540.0, 28.0) if far else (30.0, -20.0, 1.0))
    d2.setflags(write=False)
    return c, d2


def case(family, n):
    return case_and_d2(family, n)[0]
