"""CPU restatement of the M2DP descriptor (include/scl_m2dp.h, DESIGN.md section 4 "M2DP") in numpy and Python floats.

The reference's m2dp_descriptor (descriptor.h:1803-2040) step by step: PCA frame (fp64, numpy.linalg.eigh, the documented sign
rule, rounded to float), float projection, the maxRho quirk, bin edges in the reference's double expression order, the 64 planes
from libm, bins with math.atan2 and a correctly rounded sqrt, the signature from numpy.linalg.svd with the Perron sign, and the
detections (brute-force 1-NN in nanoflann's float order).  This is the yardstick of tests/test_gpu_m2dp.py.
"""
import math
from decimal import Decimal, getcontext

import numpy as np

NUM_T, NUM_R, NUM_P, NUM_Q = 16, 8, 4, 16
ROWS, COLS, DIM = 64, 128, 192


def theta_list():
    """thetaList[i] = -M_PI + i * 2 * M_PI / numT (D.h:1866-1870), the double expression order"""
    return [-math.pi + (i * 2) * math.pi / NUM_T for i in range(NUM_T + 1)]


def rho_list(max_rho):
    """rhoList[i] = (i * sqrt(maxRho) / numR)^2, last edge + 0.001 (D.h:1872-1880)"""
    out = []
    for i in range(NUM_R + 1):
        r = i * math.sqrt(max_rho) / NUM_R
        out.append(r * r)
    out[-1] = out[-1] + 0.001
    return out


def planes():
    """(px, py) of the 64 planes, D.h:1808-1818, 1885-1906: row = azimuth_i * 16 + elevation_j; (64, 3) each"""
    px = np.empty((ROWS, 3)); py = np.empty((ROWS, 3))
    for i in range(NUM_P):
        azm = -math.pi / 2 + i * math.pi / (NUM_P - 1)
        for j in range(NUM_Q):
            elv = j * (math.pi / 2) / (NUM_Q - 1)
            n = (1.0 * math.cos(elv) * math.cos(azm), 1.0 * math.cos(elv) * math.sin(azm), 1.0 * math.sin(elv))
            h = n[0]                                       # [1, 0, 0] . vecN
            p = (1.0 - h * n[0], 0.0 - h * n[1], 0.0 - h * n[2])
            q = (n[1] * p[2] - n[2] * p[1], n[2] * p[0] - n[0] * p[2], n[0] * p[1] - n[1] * p[0])   # vecN x px (Eigen's cross)
            px[i * NUM_Q + j] = p; py[i * NUM_Q + j] = q
    return px, py


# ---- the theta-edge constants of the device's exact path -------------------------------------------------------------------
def _dec_sin_cos(x, prec=70):
    getcontext().prec = prec
    s, c = Decimal(0), Decimal(0)
    term = Decimal(1)                                      # x^k / k!
    for k in range(0, 200):
        if k % 4 == 0: c += term
        elif k % 4 == 1: s += term
        elif k % 4 == 2: c -= term
        else: s -= term
        term = term * x / (k + 1)
        if abs(term) < Decimal(10) ** (-prec + 2):
            break
    return s, c


def theta_edge_constants():
    """For every theta edge t_i: the midpoint m_i between t_i and the next double below it, and (cos m_i, sin m_i) as
    double-double pairs (hi, lo).  A correctly rounded atan2 is < t_i exactly when the true angle is < m_i, which the device
    decides by the sign of pcy * cos(m_i) - pcx * sin(m_i).  Returns [(C_hi, C_lo, S_hi, S_lo)] * 17; edge 8 (t = 0) is
    (1, 0, 0, 0): the angle is < 0 exactly when pcy < 0."""
    out = []
    for i, t in enumerate(theta_list()):
        if t == 0.0:
            out.append((1.0, 0.0, 0.0, 0.0)); continue
        m = (Decimal(t) + Decimal(math.nextafter(t, -math.inf))) / 2
        s, c = _dec_sin_cos(m)
        ch = float(c); cl = float(c - Decimal(ch)); sh = float(s); sl = float(s - Decimal(sh))
        out.append((ch, cl, sh, sl))
    return out


# ---- frame --------------------------------------------------------------------------------------------------------------------
def _xyz(cloud):
    c = np.asarray(cloud, dtype=np.float32)
    return np.ascontiguousarray(c[:, :3])


def project(xyz, mean_f, axes_f):
    """float projection E^T (p - mean): each component a sequential 3-term dot product, no FMA"""
    d = xyz - mean_f[None, :]                              # float32
    out = np.empty_like(d)
    for k in range(3):
        a = axes_f[k]
        out[:, k] = (a[0] * d[:, 0] + a[1] * d[:, 1]) + a[2] * d[:, 2]
    return out


def frame(cloud):
    """(mean float32[3], axes float32[3, 3] with axis k = row k) -- fp64 PCA, descending eigenvalues, the sign rule, float"""
    xyz = _xyz(cloud)
    p = xyz.astype(np.float64)
    n = p.shape[0]
    mean = p.sum(axis=0) / n
    cov = (p.T @ p) / n - np.outer(mean, mean)
    w, V = np.linalg.eigh(cov)
    order = np.argsort(-w, kind="stable")
    a0, a1 = V[:, order[0]].copy(), V[:, order[1]].copy()
    mean_f = mean.astype(np.float32)
    s = []
    for a in (a0, a1):                                     # sum of cubed FLOAT projections along the unsigned float axis
        af = a.astype(np.float32)
        d = xyz - mean_f[None, :]
        c = (af[0] * d[:, 0] + af[1] * d[:, 1]) + af[2] * d[:, 2]
        s.append(1.0 if float(np.sum(c.astype(np.float64) ** 3)) >= 0.0 else -1.0)
    a0 = a0 * s[0]; a1 = a1 * s[1]
    a2 = np.array([a0[1] * a1[2] - a0[2] * a1[1], a0[2] * a1[0] - a0[0] * a1[2], a0[0] * a1[1] - a0[1] * a1[0]])
    return mean_f, np.stack([a0, a1, a2]).astype(np.float32)


def cloud_pca(cloud, fr=None):
    """(cloudPca rows (x, y, -z) as float64, maxRho as a Python float) for the frame `fr` (default: the checker's)"""
    xyz = _xyz(cloud)
    mean_f, axes_f = fr if fr is not None else frame(cloud)
    pr = project(xyz, np.asarray(mean_f, np.float32), np.asarray(axes_f, np.float32))
    x, z = pr[:, 0], pr[:, 2]
    rho = np.sqrt((x * x + x * x) + z * z)                 # float32, x twice and y absent (D.h:1836-1839)
    max_rho = float(rho.max()) if rho.size else 0.0
    pca = np.stack([pr[:, 0].astype(np.float64), pr[:, 1].astype(np.float64), -pr[:, 2].astype(np.float64)], axis=1)
    return pca, max_rho


def theta_bins(pcx, pcy, tl=None):
    """first i with atan2(pcy, pcx) < thetaList[i], minus 1 (glibc's atan2: numpy's arctan2 where it is far from every edge,
    math.atan2 near them)"""
    tl = np.asarray(theta_list() if tl is None else tl)
    th = np.arctan2(pcy, pcx)
    near = np.min(np.abs(th[:, None] - tl[None, :]), axis=1) < 1e-9
    for k in np.nonzero(near)[0]:
        th[k] = math.atan2(float(pcy[k]), float(pcx[k]))
    return np.searchsorted(tl, th, side="right") - 1, int(near.sum())


def signature_matrix(cloud, frame_in=None, return_near=False):
    """the 64 x 128 uint32 counts (row = plane, column = rho_bin * 16 + theta_bin) and maxRho; frame_in = (mean, axes) e.g.
    the GPU's, so that the counts can be compared bit for bit"""
    pca, max_rho = cloud_pca(cloud, frame_in)
    tl = theta_list(); rl = np.asarray(rho_list(max_rho))
    px, py = planes()
    counts = np.zeros((ROWS, COLS), np.uint32)
    near_total = 0
    x, y, z = pca[:, 0], pca[:, 1], pca[:, 2]
    for r in range(ROWS):
        pcx = (x * px[r, 0] + y * px[r, 1]) + z * px[r, 2]
        pcy = (x * py[r, 0] + y * py[r, 1]) + z * py[r, 2]
        rho = np.sqrt(pcx * pcx + pcy * pcy)
        tb, near = theta_bins(pcx, pcy, tl)
        near_total += near
        rb = np.searchsorted(rl, rho, side="right") - 1
        ok = (tb >= 0) & (tb < NUM_T) & (rb >= 0) & (rb < NUM_R)
        np.add.at(counts[r], (rb[ok] * NUM_T + tb[ok]), 1)
    if return_near:
        return counts, max_rho, near_total
    return counts, max_rho


def signature_from_counts(counts, n_points):
    """top singular pair of A = counts / n (numpy.linalg.svd), sum(u) >= 0, each double rounded to float: 192 float32"""
    A = counts.astype(np.float64) / n_points
    if not A.any():
        return np.zeros(DIM, np.float32)
    U, S, Vt = np.linalg.svd(A)
    u, v = U[:, 0], Vt[0]
    if u.sum() < 0:
        u, v = -u, -v
    return np.concatenate([u, v]).astype(np.float32)


def sigma_ratio(counts):
    S = np.linalg.svd(counts.astype(np.float64), compute_uv=False)
    return float(S[1] / S[0]) if S[0] > 0 else 1.0


def signature(cloud, frame_in=None):
    counts, _ = signature_matrix(cloud, frame_in)
    return signature_from_counts(counts, np.asarray(cloud).shape[0])


# ---- detection ----------------------------------------------------------------------------------------------------------------
def sqdist_nanoflann(a, b):
    """squared L2 in float: groups of four d0*d0 + d1*d1 + d2*d2 + d3*d3 added to the running sum"""
    d = (np.asarray(a, np.float32) - np.asarray(b, np.float32)).reshape(-1, 4)
    g = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) + d[:, 3] * d[:, 3]
    s = np.float32(0.0)
    for x in g:
        s = np.float32(s + x)
    return s


class CheckerDB:
    """the plugin layer: keyframes with (robot, index), per-robot lists, intra / inter detection"""

    def __init__(self, robot_num=1, this_id=0, num_exclude_recent=30, dist_thres=0.3):
        self.robot_num, self.this_id, self.excl, self.thres = robot_num, this_id, num_exclude_recent, dist_thres
        self.sigs, self.robots, self.indexs = [], [], []
        self.l2g = [[] for _ in range(robot_num)]

    def save(self, values, robot, index):
        self.l2g[robot].append(len(self.sigs))
        self.sigs.append(np.asarray(values, np.float32).copy()); self.robots.append(robot); self.indexs.append(index)

    def _nn(self, q, keys):
        best, bk = None, -1
        for k in sorted(keys):
            d = sqdist_nanoflann(self.sigs[q], self.sigs[k])
            if best is None or d < best:
                best, bk = d, k
        return bk, (np.float32(np.sqrt(best)) if best is not None else np.float32(np.inf))

    def detect_intra(self, cur):
        mine = self.l2g[self.this_id]
        hist = mine[:max(0, cur - self.excl)]
        k, d = self._nn(mine[cur], hist)
        if k < 0:
            return -1, d
        return (mine.index(k) if float(d) < self.thres else -1), d

    def detect_inter(self, cur):
        if self.robots[cur] == self.this_id:
            keys = [k for r in range(self.robot_num) if r != self.this_id for k in self.l2g[r]]
        else:
            keys = list(self.l2g[self.this_id])
        k, d = self._nn(cur, keys)
        if k < 0:
            return -1, d
        return (k if float(d) < self.thres else -1), d
