"""The checkers and the named inputs of the pose-graph solve (include/scl_engine.h "POSE-GRAPH SOLVE").

  linearize_exact(g)     the contract in mpmath at 40 digits on the float64 inputs, rounded to float64: a Lin (cost, grad[n,6],
                         diag[n,6,6], chi2[m]) -- and, for lm_exact, the unrounded pieces
  linearize_numpy(g)     a vectorised float64 restatement (dense adjoints, numpy's Cholesky and solves, [w]x^2 as a matrix product:
                         another order of every product than the device's): the same Lin, with the whitened Jacobians Ai, Aj of every
                         factor and the majorants below
  hessian(lin, lam)      H + lam diag(H) as a scipy.sparse matrix from Ai, Aj; hessian_majorant(lin, lam): the same with |.| of every term
  lm_numpy(g, params)    the contract's Levenberg-Marquardt loop with scipy's sparse direct solve in place of PCG: (poses, info)
  lm_exact(g, params)    the same loop in mpmath (dense LU) for graphs of <= EXACT_POSES poses: the 40-digit minimiser
  components_ok(...)     the union-find of the contract: every connected component holds a prior

Majorants.  A sum is held relative to the sum of the absolute values of its terms, taken where the rounding enters: the whitening.  With
cov = L L^T, the whitened residual y = L^-1 r is a sum of terms |L^-1| rbar, where rbar bounds what r is made of: 1 for every rotation
component (unit quaternions) plus |w|, and for the translation |t_E| + |t_Z| + |t_j - t_i| (a prior: |t_E| + |t_X - t_Z|) -- the lengths
that are rotated and added to give t_E.  So ybar = |L^-1| rbar, Abar = |L^-1| |J| and
    chi2_m[k] = ybar . ybar,  cost_m = 1/2 sum chi2_m,  grad_m = sum Abar^T ybar,  diag_m = sum Abar^T Abar,
and hessian_majorant for the operator.  A deviation is |got - exact| / majorant.

TAU_LIN: 16 x the largest deviation of linearize_numpy from linearize_exact over LIN_CASES (measured, written down below, pinned by
test_pgo_cases.py, which asserts that the restatement stays within TAU_LIN / 16).  The factor 16 is PCM's: it covers what separates the
device from numpy -- another atan2 / sqrt of a few ulp and another order inside the 6 x 6 products.

TAU_X: 16 x the deviation of lm_numpy, run with TIGHT parameters (stop tolerances 1e-14, CG 1e-12, so that what remains is rounding and
not the stopping rule), from lm_exact on the 16-pose ring, run with EXACT ones (to the minimiser itself).  pose_deviation(a, b) = max over poses of max(|dt| / max(1, |t|max),
|dq|) with both quaternions at w >= 0.  On a larger graph the bound is TAU_X * max(1, cond(H) / cond(H_ring)) with cond the 2-norm
condition number of H at the answer (condition(lin)): the error rounding leaves in a minimiser grows with the condition of the normal
equations, and the ring's own condition is what TAU_X was measured at.

OPT_NOISE.  The optimiser tests also hold the gradient at the answer within TAU_LIN of zero relative to grad_m.  The contract's first stop
is on the cost: an accepted step that lowers it by no more than 1e-14 of itself ends the solve.  The cost is quadratic around its minimum,
so that stop resolves the minimiser only to a distance d with d^T H d / 2 = 1e-14 cost, and leaves a gradient H d that grows with the
square root of the final cost -- whatever runs the loop, the checkers included: with measurements as noisy as their covariances say
(noise 1: a final cost of about 3 per loop), lm_numpy's own answers on the two-robot and the 4097-pose graph have gradients of 2.4e-13
and 9.4e-13 of grad_m, above TAU_LIN = 2e-13, and one more full step, which the stop does not allow, brings them to 3e-15 and 3e-14.
Those graphs therefore draw their measurement noise at OPT_NOISE = 0.03 of the stated covariances: the final cost is a thousandth and
the gradient the stop leaves a thirtieth.  On the two-robot graph lm_numpy's answer then has 4.5e-16 of grad_m, and the 16-pose ring, which
keeps noise 1, 1.3e-14: test_pgo_cases.py asserts that the checker's own answers meet the criterion with a factor 4 to spare.  The
rejected-step case also keeps noise 1 (lm_numpy: within TAU_LIN, asserted there too).  On 4097 poses the checker's own loop does not meet
it at any noise level: a sum of 4000 terms carries a rounding of its own of about 1e-15 of itself, so the comparison cost_new < cost
turns into a coin long before the gradient is at TAU_LIN, and the loop ends where the coin lets it (lm_numpy: 21 iterations and 6.7e-12
of grad_m at OPT_NOISE, 9.4e-13 at noise 1).  The criterion is on the device's answer, not on the checker's, and the 4097-pose test
asserts it there; the device is held to lm_numpy within the scaled TAU_X only."""
import functools
from collections import namedtuple
from types import SimpleNamespace

import mpmath
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import pcm_cases as pc

Graph = namedtuple("Graph", "poses f_i f_j f_z f_cov p_idx p_z p_cov")
Lin = SimpleNamespace
SERIES_BELOW = 0.05          # theta below which c(theta) is the series of the contract
EXACT_POSES = 16
STOP_COST, STOP_STEP, STOP_ITERATIONS, STOP_LAMBDA = 1, 2, 3, 4
DEFAULTS = dict(max_iterations=50, lambda_initial=1e-5, lambda_factor=10.0, lambda_max=1e10, relative_cost_tolerance=1e-10,
                step_tolerance=1e-10, cg_tolerance=1e-8, cg_max_iterations=500)
TIGHT = dict(DEFAULTS, relative_cost_tolerance=1e-14, step_tolerance=1e-14, cg_tolerance=1e-12)
EXACT = dict(DEFAULTS, relative_cost_tolerance=1e-34, step_tolerance=1e-34)      # lm_exact run to the minimiser, not to a float64 stop
# measured (test_pgo_cases.py prints them): the largest deviations of linearize_numpy are chain5 7.63e-15, one 5.31e-15, two 4.18e-15 (all
# in diag) and chain65 2.25e-9 (diag; its covariances reach a condition of 1e8, and a Cholesky solve loses that).  Times 16 (1.22e-13 and
# 3.6e-8), rounded up to one digit.  TAU_LIN holds for covariances of the kind every other case here has (pc.random_cov: condition < 1e3).
TAU_LIN = 2e-13
TAU_LIN_CASE = {"chain5": TAU_LIN, "one": TAU_LIN, "two": TAU_LIN, "chain65": 4e-8}
# measured: pose_deviation(lm_numpy(TIGHT), lm_exact(EXACT)) on ring16 is 8.22e-13 (cond(H) = 2.28e5); times 16, rounded up to one digit
TAU_X = 2e-11
OPT_NOISE = 0.03


def graph(poses, f_i, f_j, f_z, f_cov, p_idx, p_z, p_cov):
    f = lambda a, w: np.ascontiguousarray(a, np.float64).reshape(-1, w)
    i = lambda a: np.ascontiguousarray(a, np.int32).reshape(-1)
    return Graph(f(poses, 7), i(f_i), i(f_j), f(f_z, 7), f(f_cov, 36), i(p_idx), f(p_z, 7), f(p_cov, 36))


def components_ok(n_poses, f_i, f_j, p_idx):
    parent = list(range(n_poses))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v
    for a, b in zip(f_i, f_j):
        parent[find(int(a))] = find(int(b))
    anchored = {find(int(p)) for p in p_idx}
    return all(find(v) in anchored for v in range(n_poses))


def incidence(n_poses, f_i, f_j, p_idx):
    """(row_ptr, entries) of the contract: entry 2 k + side, factors numbered between factors first, every list ascending"""
    rows = [[] for _ in range(n_poses)]
    for k, (a, b) in enumerate(zip(f_i, f_j)):
        rows[int(a)].append(2 * k); rows[int(b)].append(2 * k + 1)
    for m, p in enumerate(p_idx):
        rows[int(p)].append(2 * (len(f_i) + m) + 1)
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    return ptr.tolist(), [e for r in rows for e in r]


# ---- float64, vectorised ------------------------------------------------------------------------------------------------------------

def _rel(a, b):
    """a^-1 b of (.,7) poses x, y, z, q: the difference of the translations first"""
    qa = pc.qconj(a[..., 3:])
    return np.concatenate([np.einsum("...ij,...j->...i", pc.qmat(qa), b[..., :3] - a[..., :3]), pc.qmul(qa, b[..., 3:])], -1)


def _c_of(theta, w, nv):
    t2 = theta * theta
    series = 1.0 / 12.0 + t2 / 720.0 + t2 * t2 / 30240.0 + t2 * t2 * t2 / 1209600.0
    with np.errstate(divide="ignore", invalid="ignore"):
        closed = 1.0 / t2 - w / (2.0 * theta * nv)
    return np.where(theta < SERIES_BELOW, series, closed)


def _log_and_jrinv(q):
    q = q * np.where(q[:, 3:4] < 0, -1.0, 1.0)
    nv = np.sqrt((q[:, :3] ** 2).sum(-1))
    half = np.arctan2(nv, q[:, 3])
    k = np.where(nv == 0, 2.0, 2.0 * half / np.where(nv == 0, 1.0, nv))
    w = k[:, None] * q[:, :3]
    theta = np.where(nv == 0, 0.0, 2.0 * half)
    K = pc._skew(w)
    J = np.eye(3) + 0.5 * K + _c_of(theta, q[:, 3], nv)[:, None, None] * (K @ K)
    return w, J


def _tri_solve_abs(L):
    return np.abs(np.linalg.inv(L))


def linearize_numpy(g, poses=None):
    X = pc._normalised(g.poses if poses is None else poses)
    n, F, P = len(X), len(g.f_i), len(g.p_idx)
    M = F + P
    Zf, Zp = pc._normalised(g.f_z), pc._normalised(g.p_z)
    fi = np.concatenate([g.f_i, np.full(P, -1, np.int32)]).astype(np.int64); fj = np.concatenate([g.f_j, g.p_idx]).astype(np.int64)
    h = _rel(X[g.f_i], X[g.f_j]); hinv = _rel(X[g.f_j], X[g.f_i])
    E = np.concatenate([pc.compose(pc.inverse(Zf), h), _rel(Zp, X[g.p_idx])], 0)
    w, Jri = _log_and_jrinv(E[:, 3:])
    r = np.concatenate([w, E[:, :3]], -1)
    D = np.zeros((M, 6, 6)); D[:, :3, :3] = Jri; D[:, 3:, 3:] = pc.qmat(E[:, 3:])
    Jj = D
    Ji = np.zeros((M, 6, 6)); Ji[:F] = -D[:F] @ pc.adjoint(hinv)
    L = np.linalg.cholesky(pc._sym(np.concatenate([g.f_cov, g.p_cov], 0)))
    y = np.linalg.solve(L, r[:, :, None])[:, :, 0]
    Ai, Aj = np.linalg.solve(L, Ji), np.linalg.solve(L, Jj)
    chi2 = (y * y).sum(-1)
    grad = np.zeros((n, 6)); diag = np.zeros((n, 6, 6))
    np.add.at(grad, fj, np.einsum("kma,km->ka", Aj, y)); np.add.at(grad, fi[:F], np.einsum("kma,km->ka", Ai[:F], y[:F]))
    np.add.at(diag, fj, np.einsum("kma,kmb->kab", Aj, Aj)); np.add.at(diag, fi[:F], np.einsum("kma,kmb->kab", Ai[:F], Ai[:F]))
    # majorants
    Li = _tri_solve_abs(L)
    dt = np.concatenate([np.linalg.norm(Zf[:, :3], axis=1) + np.linalg.norm(X[g.f_j, :3] - X[g.f_i, :3], axis=1),
                         np.linalg.norm(X[g.p_idx, :3] - Zp[:, :3], axis=1)])
    rbar = np.abs(r) + np.concatenate([np.ones((M, 3)), np.repeat((dt + np.linalg.norm(E[:, :3], axis=1))[:, None], 3, 1)], 1)
    ybar = np.einsum("kab,kb->ka", Li, rbar)
    Abi, Abj = Li @ np.abs(Ji), Li @ np.abs(Jj)
    grad_m = np.zeros((n, 6)); diag_m = np.zeros((n, 6, 6))
    np.add.at(grad_m, fj, np.einsum("kma,km->ka", Abj, ybar)); np.add.at(grad_m, fi[:F], np.einsum("kma,km->ka", Abi[:F], ybar[:F]))
    np.add.at(diag_m, fj, np.einsum("kma,kmb->kab", Abj, Abj)); np.add.at(diag_m, fi[:F], np.einsum("kma,kmb->kab", Abi[:F], Abi[:F]))
    chi2_m = (ybar * ybar).sum(-1)
    return Lin(n=n, F=F, M=M, fi=fi, fj=fj, cost=0.5 * chi2.sum(), grad=grad, diag=diag, chi2=chi2, Ai=Ai, Aj=Aj, Abi=Abi, Abj=Abj,
               cost_m=0.5 * chi2_m.sum(), grad_m=grad_m, diag_m=diag_m, chi2_m=chi2_m)


def _assemble(n, F, fi, fj, Ai, Aj, lam):
    rows, cols, vals = [], [], []
    a6 = np.arange(6)

    def add(pi, pj, B):
        rows.append((6 * pi[:, None, None] + a6[None, :, None]).repeat(6, 2).ravel())
        cols.append((6 * pj[:, None, None] + a6[None, None, :]).repeat(6, 1).ravel())
        vals.append(B.ravel())
    add(fj, fj, np.einsum("kma,kmb->kab", Aj, Aj))
    add(fi[:F], fi[:F], np.einsum("kma,kmb->kab", Ai[:F], Ai[:F]))
    W = np.einsum("kma,kmb->kab", Ai[:F], Aj[:F])
    add(fi[:F], fj[:F], W); add(fj[:F], fi[:F], np.swapaxes(W, 1, 2))
    H = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(6 * n, 6 * n)).tocsr()
    return (H + lam * sp.diags(H.diagonal())).tocsr()


def hessian(lin, lam=0.0):
    return _assemble(lin.n, lin.F, lin.fi, lin.fj, lin.Ai, lin.Aj, lam)


def hessian_majorant(lin, lam=0.0):
    return _assemble(lin.n, lin.F, lin.fi, lin.fj, lin.Abi, lin.Abj, lam)


def condition(lin):
    H = hessian(lin)
    if H.shape[0] <= 1600:
        ev = np.linalg.eigvalsh(H.toarray())
        return float(ev[-1] / ev[0])
    hi = spla.eigsh(H, k=1, which="LA", return_eigenvectors=False)[0]
    lo = spla.eigsh(H.tocsc(), k=1, sigma=0.0, which="LM", return_eigenvectors=False)[0]
    return float(hi / lo)


def retract(X, delta):
    """gtsam's default: R <- R Exp(dw), t <- t + R dv; X (n,7) with unit quaternions, delta (n,6)"""
    q = pc.qmul(X[:, 3:], pc.rotvec_to_quat(delta[:, :3]))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    t = X[:, :3] + np.einsum("nij,nj->ni", pc.qmat(X[:, 3:]), delta[:, 3:])
    return np.concatenate([t, q], 1)


def canonical(X):
    X = pc._normalised(X)
    X[:, 3:] *= np.where(X[:, 6:7] < 0, -1.0, 1.0)
    return X


def pose_deviation(a, b):
    a, b = canonical(a), canonical(b)
    scale = max(1.0, float(np.abs(b[:, :3]).max()))
    return max(float(np.abs(a[:, :3] - b[:, :3]).max()) / scale, float(np.abs(a[:, 3:] - b[:, 3:]).max()))


def _lm(X, params, linearize, solve, retract_fn, lt, le, sub):
    """the contract's loop; lt(a, b): a < b, le: a <= b, sub: a - b -- in the arithmetic of the costs"""
    p = dict(DEFAULTS, **(params or {}))
    lin = linearize(X)
    cost, lam = lin.cost, p["lambda_initial"]
    info = dict(iterations=0, accepted=0, rejected=0, initial_cost=float(cost), trace=[])
    while True:
        delta, step = solve(lin, lam)
        Xt = retract_fn(X, delta)
        lint = linearize(Xt)
        info["iterations"] += 1
        stop_cost = False
        ok = lt(lint.cost, cost)
        info["trace"].append((float(lam), bool(ok), float(lint.cost)))
        if ok:
            stop_cost = le(sub(cost, lint.cost), p["relative_cost_tolerance"] * cost)
            X, lin, cost = Xt, lint, lint.cost
            info["accepted"] += 1
            lam /= p["lambda_factor"]
        else:
            info["rejected"] += 1
            lam *= p["lambda_factor"]
        if stop_cost:
            info["stop_reason"] = STOP_COST; break
        if step <= p["step_tolerance"]:
            info["stop_reason"] = STOP_STEP; break
        if info["iterations"] >= p["max_iterations"]:
            info["stop_reason"] = STOP_ITERATIONS; break
        if lam > p["lambda_max"]:
            info["stop_reason"] = STOP_LAMBDA; break
    info.update(final_cost=float(cost), final_lambda=float(lam), lin=lin)
    return X, info


def lm_numpy(g, params=None):
    def solve(lin, lam):
        d = spla.spsolve(hessian(lin, lam).tocsc(), -lin.grad.ravel())
        return d.reshape(-1, 6), float(np.abs(d).max())
    X, info = _lm(pc._normalised(g.poses), params, lambda X: linearize_numpy(g, X), solve, retract,
                  lambda a, b: a < b, lambda a, b: a <= b, lambda a, b: a - b)
    return canonical(X), info


# ---- mpmath, 40 digits ---------------------------------------------------------------------------------------------------------------

def _mv(v):
    return [mpmath.mpf(float(x)) for x in v]


def _m_pose(row):
    """(q, t) of a float64 pose row, or of a row of mpf, the quaternion normalised at 40 digits"""
    v = [x if isinstance(x, mpmath.mpf) else mpmath.mpf(float(x)) for x in row]
    s = mpmath.sqrt(v[3] ** 2 + v[4] ** 2 + v[5] ** 2 + v[6] ** 2)
    return [c / s for c in v[3:]], v[:3]


def _m_mat_vec(R, v):
    return [sum(R[i][k] * v[k] for k in range(3)) for i in range(3)]


def _m_rel(a, b):
    qa = [-a[0][0], -a[0][1], -a[0][2], a[0][3]]
    return pc._mq_mul(qa, b[0]), _m_mat_vec(pc._mq_mat(qa), [b[1][k] - a[1][k] for k in range(3)])


def _m_compose(a, b):
    return pc._mq_mul(a[0], b[0]), [a[1][i] + x for i, x in enumerate(_m_mat_vec(pc._mq_mat(a[0]), b[1]))]


def _m_inverse(a):
    qi = [-a[0][0], -a[0][1], -a[0][2], a[0][3]]
    return qi, [-x for x in _m_mat_vec(pc._mq_mat(qi), a[1])]


def m_c_of(theta, w, nv, series_below=SERIES_BELOW):
    """c(theta) of the contract: the series below the switch, the half-angle closed form above"""
    if theta < series_below:
        t2 = theta * theta
        return mpmath.mpf(1) / 12 + t2 / 720 + t2 * t2 / 30240 + t2 * t2 * t2 / 1209600
    return 1 / (theta * theta) - w / (2 * theta * nv)


def _m_log_and_jrinv(q):
    if q[3] < 0:
        q = [-c for c in q]
    nv = mpmath.sqrt(q[0] ** 2 + q[1] ** 2 + q[2] ** 2)
    k = mpmath.mpf(2) if nv == 0 else 2 * mpmath.atan2(nv, q[3]) / nv
    w = [k * q[0], k * q[1], k * q[2]]
    theta = mpmath.mpf(0) if nv == 0 else 2 * mpmath.atan2(nv, q[3])
    c = m_c_of(theta, q[3], nv)
    ww = w[0] ** 2 + w[1] ** 2 + w[2] ** 2
    K = [[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]
    J = [[(1 if a == b else 0) + K[a][b] / 2 + c * (w[a] * w[b] - (ww if a == b else 0)) for b in range(3)] for a in range(3)]
    return w, J


def m_residual(Xi, Xj, Z):
    """r (6) of one factor at 40 digits; Xi None: a prior.  Poses as (q, t) of _m_pose"""
    E = _m_rel(Z, Xj) if Xi is None else _m_compose(_m_inverse(Z), _m_rel(Xi, Xj))
    return _m_log_and_jrinv(E[0])[0] + list(E[1])


def m_cholesky(S):
    """the lower L of S = L L^T from the upper triangle of S, column by column"""
    L = [[mpmath.mpf(0)] * 6 for _ in range(6)]
    for c in range(6):
        s = S[c][c] - sum(L[c][k] ** 2 for k in range(c))
        L[c][c] = mpmath.sqrt(s)
        for rr in range(c + 1, 6):
            L[rr][c] = (S[c][rr] - sum(L[rr][k] * L[c][k] for k in range(c))) / L[c][c]
    return L


def _m_factor(Xi, Xj, Z, S):
    """(y, Ai or None, Aj) of one factor: whitened residual and Jacobians, lists of mpf"""
    E = _m_rel(Z, Xj) if Xi is None else _m_compose(_m_inverse(Z), _m_rel(Xi, Xj))
    w, Jri = _m_log_and_jrinv(E[0])
    r = w + list(E[1])
    RE = pc._mq_mat(E[0])
    zero = mpmath.mpf(0)
    D = [Jri[a] + [zero] * 3 for a in range(3)] + [[zero] * 3 + RE[a] for a in range(3)]
    Ji = None
    if Xi is not None:
        hinv = _m_rel(Xj, Xi)
        R = pc._mq_mat(hinv[0]); t = hinv[1]
        K = [[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]
        B = pc._m_mul(K, R)
        Ad = [R[a] + [zero] * 3 for a in range(3)] + [B[a] + R[a] for a in range(3)]
        Ji = [[-v for v in row] for row in pc._m_mul(D, Ad)]
    L = m_cholesky(S)

    def fwd(v):
        o = []
        for a in range(6):
            o.append((v[a] - sum(L[a][k] * o[k] for k in range(a))) / L[a][a])
        return o

    def white(J):
        cols = [fwd([J[a][c] for a in range(6)]) for c in range(6)]
        return [[cols[c][a] for c in range(6)] for a in range(6)]
    return fwd(r), None if Ji is None else white(Ji), white(D)


def _m_linearize(g, X):
    """X: a list of (q, t) at 40 digits.  The unrounded pieces: cost, grad[n][6], diag[n][6][6], chi2[m], and the factors' (y, Ai, Aj)"""
    n, F = len(X), len(g.f_i)
    sym = pc._sym(np.concatenate([g.f_cov, g.p_cov], 0))
    zero = mpmath.mpf(0)
    grad = [[zero] * 6 for _ in range(n)]; diag = [[[zero] * 6 for _ in range(6)] for _ in range(n)]
    chi2, facs = [], []
    for k in range(F + len(g.p_idx)):
        i = int(g.f_i[k]) if k < F else None
        j = int(g.f_j[k]) if k < F else int(g.p_idx[k - F])
        Z = _m_pose(g.f_z[k] if k < F else g.p_z[k - F])
        S = [[mpmath.mpf(float(v)) for v in row] for row in sym[k]]
        y, Ai, Aj = _m_factor(None if i is None else X[i], X[j], Z, S)
        chi2.append(sum(v * v for v in y))
        facs.append((i, j, y, Ai, Aj))
        for p, A in ((i, Ai), (j, Aj)):
            if A is None:
                continue
            for a in range(6):
                grad[p][a] += sum(A[m][a] * y[m] for m in range(6))
                for b in range(6):
                    diag[p][a][b] += sum(A[m][a] * A[m][b] for m in range(6))
    return Lin(n=n, cost=sum(chi2) / 2, grad=grad, diag=diag, chi2=chi2, facs=facs)


def _rounded(lin):
    return Lin(n=lin.n, cost=float(lin.cost), grad=np.array([[float(v) for v in row] for row in lin.grad]),
               diag=np.array([[[float(v) for v in row] for row in blk] for blk in lin.diag]), chi2=np.array([float(v) for v in lin.chi2]))


def linearize_exact(g, poses=None):
    with mpmath.workdps(40):
        X = [_m_pose(row) for row in (g.poses if poses is None else poses)]
        return _rounded(_m_linearize(g, X))


def _m_retract(X, delta):
    out = []
    for (q, t), d in zip(X, delta):
        th = mpmath.sqrt(d[0] ** 2 + d[1] ** 2 + d[2] ** 2)
        k = mpmath.mpf(1) / 2 if th == 0 else mpmath.sin(th / 2) / th
        qn = pc._mq_mul(q, [k * d[0], k * d[1], k * d[2], mpmath.cos(th / 2)])
        s = mpmath.sqrt(sum(c * c for c in qn))
        out.append(([c / s for c in qn], [t[i] + x for i, x in enumerate(_m_mat_vec(pc._mq_mat(q), d[3:]))]))
    return out


def lm_exact(g, params=None):
    """the contract's loop at 40 digits with a dense LU solve: (poses (n,7) rounded to float64, info)"""
    assert len(g.poses) <= EXACT_POSES
    with mpmath.workdps(40):
        def solve(lin, lam):
            N = 6 * lin.n
            H = mpmath.zeros(N, N); rhs = mpmath.zeros(N, 1)
            for i, j, y, Ai, Aj in lin.facs:
                for (p, A), (q, B) in [((j, Aj), (j, Aj))] + ([] if Ai is None else [((i, Ai), (i, Ai)), ((i, Ai), (j, Aj)), ((j, Aj), (i, Ai))]):
                    for a in range(6):
                        for b in range(6):
                            H[6 * p + a, 6 * q + b] += sum(A[m][a] * B[m][b] for m in range(6))
            for p in range(lin.n):
                for a in range(6):
                    rhs[6 * p + a] = -lin.grad[p][a]
            for d in range(N):
                H[d, d] += mpmath.mpf(lam) * H[d, d]
            x = mpmath.lu_solve(H, rhs)
            delta = [[x[6 * p + a] for a in range(6)] for p in range(lin.n)]
            return delta, float(max(abs(v) for v in x))
        X, info = _lm([_m_pose(row) for row in g.poses], params, lambda X: _m_linearize(g, X), solve, _m_retract,
                      lambda a, b: a < b, lambda a, b: a <= b, lambda a, b: a - b)
        info["lin"] = _rounded(info["lin"])
        out = np.array([[float(v) for v in t + q] for q, t in X])
    return canonical(out), info


# ---- the inputs --------------------------------------------------------------------------------------------------------------------------

def pose(t, rotvec):
    return np.concatenate([np.asarray(t, np.float64), pc.rotvec_to_quat(np.asarray(rotvec, np.float64))])


def between(a, b):
    """a^-1 b of two poses (7,)"""
    z = _rel(a[None], b[None])[0]
    z[3:] /= np.linalg.norm(z[3:])
    return z


def perturb(p, xi):
    """p Exp(xi), xi rotation first (gtsam's retraction)"""
    return retract(pc._normalised(np.atleast_2d(p)), np.atleast_2d(np.asarray(xi, np.float64)))[0]


def spd(rs, cond, scale):
    """a 6 x 6 covariance of the given condition number, its largest eigenvalue `scale`"""
    Q, _ = np.linalg.qr(rs.standard_normal((6, 6)))
    ev = np.exp(rs.uniform(np.log(1.0 / cond), 0.0, 6)); ev[0], ev[1] = 1.0, 1.0 / cond
    A = (Q * (ev * scale)) @ Q.T
    return (A + A.T) / 2


def odom_cov(rs):
    return pc.random_cov(rs)


def trajectory(rs, n, origin=(0.0, 0.0, 0.0)):
    return pc.random_walk(rs, n, np.asarray(origin, np.float64))


def chain_graph(rs, truth, noise=1.0, loops=(), start_noise=0.0, exact=False, cov_fn=None):
    """Odometry between consecutive poses of `truth`, the loops (i, j) given, one prior at pose 0.  Measurements are the true relative
    poses behind a right perturbation drawn from their own covariance (exact: none); the initial estimate is the chained odometry
    (start_noise > 0: the truth behind a perturbation of that standard deviation instead)"""
    n = len(truth)
    pairs = [(k, k + 1) for k in range(n - 1)] + list(loops)
    covs, zs = [], []
    for i, j in pairs:
        cov = (cov_fn or odom_cov)(rs)
        z = between(truth[i], truth[j])
        if not exact:
            z = perturb(z, noise * (np.linalg.cholesky(cov) @ rs.standard_normal(6)))
        covs.append(cov); zs.append(z)
    if start_noise > 0:
        start = np.array([perturb(p, start_noise * rs.standard_normal(6)) for p in truth])
    else:
        start = [truth[0].copy()]
        for k in range(n - 1):
            nxt = pc.compose(start[-1], zs[k]); nxt[3:] /= np.linalg.norm(nxt[3:])
            start.append(nxt)
        start = np.array(start)
    pcov = np.diag([1e-6] * 3 + [1e-4] * 3)
    return graph(start, [p[0] for p in pairs], [p[1] for p in pairs], zs, np.array(covs).reshape(-1, 36), [0], truth[0][None], pcov.reshape(1, 36))


@functools.lru_cache(maxsize=None)
def lin_case(name):
    """the named inputs of the linearisation tests; treat as read-only"""
    rs = np.random.RandomState(sorted(LIN_CASES).index(name) + 500)
    if name == "one":                                       # 1 pose, 1 prior
        p = pose([1.0, -2.0, 0.5], [0.1, -0.3, 0.7])
        return graph(p[None], [], [], np.zeros((0, 7)), np.zeros((0, 36)), [0], perturb(p, [0.02, 0.01, -0.03, 0.1, -0.2, 0.05])[None],
                     odom_cov(rs).reshape(1, 36))
    if name == "two":                                       # 2 poses, f_i > f_j, a duplicate factor
        a, b = pose([0.0, 0.0, 0.0], [0.0, 0.0, 0.1]), pose([1.0, 0.2, 0.0], [0.05, 0.0, 0.4])
        z = perturb(between(b, a), [0.01, -0.02, 0.015, 0.03, 0.02, -0.01])
        return graph([a, b], [1, 1], [0, 0], [z, z], [odom_cov(rs).ravel(), odom_cov(rs).ravel()], [1], b[None], odom_cov(rs).reshape(1, 36))
    if name == "chain5":                                    # identical poses (theta = 0 exactly), exact and noisy factors mixed
        t = trajectory(rs, 5)
        t[2] = t[1]
        g = chain_graph(rs, t, loops=[(4, 0), (0, 3)])
        z = g.f_z.copy(); z[1] = [0, 0, 0, 0, 0, 0, 1]
        return g._replace(poses=t.copy(), f_z=z)
    if name == "chain65":                                   # 2 km from the origin, rotations near pi, condition numbers up to 1e8
        t = trajectory(rs, 65, origin=(2000.0, -1500.0, 30.0))
        conds = 10.0 ** rs.uniform(0, 8, 200); conds[0] = 1e8
        it = iter(conds)
        g = chain_graph(rs, t, loops=[(64, 0), (10, 40), (40, 10), (10, 40), (63, 1)], cov_fn=lambda r: spd(r, next(it), 10.0 ** r.uniform(-4, -2)))
        z = g.f_z.copy()
        for k, ang in ((3, np.pi - 1e-9), (17, np.pi - 1e-3), (30, 3.0)):       # measurements a half turn off their poses
            axis = rs.standard_normal(3); axis /= np.linalg.norm(axis)
            z[k] = pc.compose(z[k], np.concatenate([[0.0, 0.0, 0.0], pc.rotvec_to_quat(ang * axis)]))
        for k, ang in ((5, 0.0499), (6, 0.0501), (7, 1e-9)):                    # residual rotations on both sides of the switch
            axis = rs.standard_normal(3); axis /= np.linalg.norm(axis)
            z[k] = pc.compose(between(g.poses[g.f_i[k]], g.poses[g.f_j[k]]), np.concatenate([[0.01, 0.0, 0.0], pc.rotvec_to_quat(ang * axis)]))
        return g._replace(f_z=z)
    raise KeyError(name)


LIN_CASES = ("chain5", "chain65", "one", "two")


@functools.lru_cache(maxsize=None)
def lin_exact(name):
    return linearize_exact(lin_case(name))


def lin_deviations(got, exact, maj):
    """the largest |got - exact| / majorant of cost, grad, diag, chi2 (0 / 0 counts as 0)"""
    def dev(a, b, m):
        a, b, m = np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(m, np.float64)
        d = np.abs(a - b)
        with np.errstate(divide="ignore", invalid="ignore"):
            return float(np.where(d == 0, 0.0, d / m).max())
    return dict(cost=dev(got.cost, exact.cost, maj.cost_m), grad=dev(got.grad, exact.grad, maj.grad_m), diag=dev(got.diag, exact.diag, maj.diag_m),
                chi2=dev(got.chi2, exact.chi2, maj.chi2_m))


@functools.lru_cache(maxsize=None)
def ring16():
    """16 poses on a ring with drifted odometry and one loop back to the start"""
    rs = np.random.RandomState(16)
    t = np.array([pose([10 * np.cos(a), 10 * np.sin(a), 0.1 * k], [0.0, 0.0, a + np.pi / 2]) for k, a in enumerate(np.linspace(0, 2 * np.pi, 16, endpoint=False))])
    return chain_graph(rs, t, noise=1.0, loops=[(15, 0)])


@functools.lru_cache(maxsize=None)
def ring16_exact():
    return lm_exact(ring16(), EXACT)


@functools.lru_cache(maxsize=None)
def ring16_condition():
    return condition(linearize_numpy(ring16(), ring16_exact()[0]))


@functools.lru_cache(maxsize=None)
def rejected_case():
    """(graph, params) whose first step the contract rejects.  A 12-pose chain with two loops is started more than a radian off; its
    first Gauss-Newton step (lambda 1e-12) still lowers the cost, the second, taken from where the first one lands, raises it by half
    (1.1e6 -> 1.6e6: decided far above rounding) and is rejected until lambda has grown by ten decades.  The case starts where that
    first step landed, so the rejected step is its first; it then converges to a cost of 7.97 in about twenty iterations."""
    rs = np.random.RandomState(77)
    t = trajectory(rs, 12)
    g = chain_graph(rs, t, loops=[(11, 0), (8, 2)])
    start = np.array([perturb(p, np.concatenate([rs.normal(0, 1.2, 3), rs.normal(0, 0.5, 3)])) for p in t])
    params = dict(TIGHT, lambda_initial=1e-12)
    landed, info = lm_numpy(g._replace(poses=start), dict(params, max_iterations=1))
    assert info["accepted"] == 1
    return g._replace(poses=landed), params


def two_robot_graph():
    """2 x 32 poses, the second robot's odometry chain tied to the first by four inter-robot loops, one prior on robot 0"""
    rs = np.random.RandomState(232)
    a, b = trajectory(rs, 32), trajectory(rs, 32, origin=(5.0, 3.0, 0.0))
    t = np.concatenate([a, b])
    ga, gb = chain_graph(rs, a, noise=OPT_NOISE), chain_graph(rs, b, noise=OPT_NOISE)
    loops = [(3, 35), (12, 50), (25, 40), (30, 63)]
    zs, covs = [], []
    for i, j in loops:
        cov = odom_cov(rs); covs.append(cov.ravel())
        zs.append(perturb(between(t[i], t[j]), OPT_NOISE * (np.linalg.cholesky(cov) @ rs.standard_normal(6))))
    return graph(np.concatenate([ga.poses, gb.poses]), np.concatenate([ga.f_i, gb.f_i + 32, [l[0] for l in loops]]),
                 np.concatenate([ga.f_j, gb.f_j + 32, [l[1] for l in loops]]), np.concatenate([ga.f_z, gb.f_z, zs]),
                 np.concatenate([ga.f_cov, gb.f_cov, covs]), [0], ga.p_z, ga.p_cov)


def planted_graph(n=257, seed=257):
    """exact factors (odometry and 3 % loops) around a truth, a noisy start: (graph, truth)"""
    rs = np.random.RandomState(seed)
    t = trajectory(rs, n)
    loops = [(int(a), int(b)) for a, b in rs.randint(0, n, (max(1, int(0.03 * n)), 2)) if a != b]
    return chain_graph(rs, t, loops=loops, exact=True, start_noise=0.02), t


def drifting_graph(n, seed=None, loop_frac=0.03, noise=1.0):
    """a multi-loop trajectory with drifting odometry (the measurements' own covariance at `noise`) and loops at loop_frac of the poses,
    started from the chained odometry (the benchmark's graph)"""
    rs = np.random.RandomState(n if seed is None else seed)
    t = trajectory(rs, n)
    m = max(1, int(loop_frac * n))
    a = rs.randint(0, n, m); b = rs.randint(0, n, m)
    loops = [(int(x), int(y)) for x, y in zip(a, b) if x != y]
    return chain_graph(rs, t, noise=noise, loops=loops)


def anchored_graph(n, every=32, seed=None, noise=OPT_NOISE):
    """drifting_graph with a prior on every `every`-th pose (position fixes of 0.1 m, 0.03 rad around the truth): the bending modes of a
    long chain, which block-Jacobi PCG cannot reach, are held"""
    rs = np.random.RandomState(7 * n if seed is None else seed)
    t = trajectory(rs, n)
    m = max(1, int(0.03 * n))
    loops = [(int(x), int(y)) for x, y in zip(rs.randint(0, n, m), rs.randint(0, n, m)) if x != y]
    g = chain_graph(rs, t, noise=noise, loops=loops)
    idx = np.arange(0, n, every)
    cov = np.diag([1e-3] * 3 + [1e-2] * 3)
    pz = np.array([perturb(t[k], noise * (np.linalg.cholesky(cov) @ rs.standard_normal(6))) for k in idx])
    return g._replace(p_idx=idx.astype(np.int32), p_z=pz, p_cov=np.tile(cov.reshape(1, 36), (len(idx), 1)))


def hub_graph(n, degree, seed=0):
    """a chain of n poses whose pose 0 has exactly `degree` incident factors (the prior among them): duplicates and factors to every
    other pose in turn, some with f_i > f_j; the poses are the truth behind a small perturbation"""
    rs = np.random.RandomState(1000 * n + degree + seed)
    t = trajectory(rs, n)
    pairs = [(k, k + 1) for k in range(n - 1)]
    have = 1 + (1 if n > 1 else 0)
    k = 0
    while n > 1 and have < degree:
        o = 1 + k % (n - 1)
        pairs.append((0, o) if k % 3 else (o, 0)); have += 1; k += 1
    zs, covs = [], []
    for i, j in pairs:
        cov = odom_cov(rs); covs.append(cov.ravel())
        zs.append(perturb(between(t[i], t[j]), np.linalg.cholesky(cov) @ rs.standard_normal(6)))
    start = np.array([perturb(p, 0.01 * rs.standard_normal(6)) for p in t])
    pcov = np.diag([1e-6] * 3 + [1e-4] * 3)
    return graph(start, [p[0] for p in pairs], [p[1] for p in pairs], np.array(zs).reshape(-1, 7), np.array(covs).reshape(-1, 36), [0], t[0][None],
                 pcov.reshape(1, 36))
