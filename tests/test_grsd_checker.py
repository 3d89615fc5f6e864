"""The GRSD CPU checker (tests/grsd_checker.py, tests/cpp/grsd_checker.c) held to the contract of DESIGN.md section 4 "GRSD":
answers derived by hand, a second restatement in numpy (brute force, Python integers for the scatter, Python floats for the fp64
steps) and independence of the traversal order.  No GPU."""
import math

import numpy as np

import fpfh_checker as fc
import grsd_cases as cs
import grsd_checker as gc


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- known answers ------------------------------------------------------------------------------------------------------------
def test_plane_known_answer():
    s = gc.stages(cs.plane())
    assert s["valid"].all()
    assert (_u32(s["normals"]) == _u32(s["normals"][0])).all() and s["normals"][0].tolist() == [0.0, 0.0, -1.0]
    assert s["centroids"].shape[0] == 16 and s["vidx"].tolist() == list(range(16)) and s["grid"].tolist()[3:] == [4, 4, 1]
    r = np.float32(float(np.float32(0.2)) * 1.1)                  # every angle is 0: A == 0, both radii 0.2f * 1.1
    assert (_u32(s["r_min"]) == _u32(r)).all() and (_u32(s["r_max"]) == _u32(r)).all()
    assert (s["classes"] == 1).all()
    # the 42 king-move pairs of a 4 x 4 board in both directions; the other 16 * 26 - 84 neighbour cells are empty
    want_T = np.zeros((6, 6), np.uint32); want_T[1, 1] = 84; want_T[1, 5] = 332
    assert np.array_equal(s["T"], want_T)
    want = np.zeros(21, np.float32); want[6] = 168; want[10] = 332
    assert np.array_equal(s["values"], want)
    v, T = gc.describe(cs.plane())
    assert np.array_equal(v, want) and np.array_equal(T, want_T)


def test_sparse_known_answer():
    """1.0 m lattice: every normal invalid, every voxel (8 points, all within 2 m of the centroid) class 1 by the A == 0 rule.  The
    COUNTERS sum to 26 per voxel; the histogram holds every diagonal counter twice (out = T[i][j] + T[j][i]), so its sum is
    26 * voxels + trace(T)."""
    s = gc.stages(cs.sparse())
    assert not s["valid"].any() and np.isnan(s["normals"]).all()
    nv = s["classes"].size
    assert nv == 32 and (s["classes"] == 1).all()
    assert int(s["T"].sum()) == 26 * nv
    assert int(s["T"][1, 1]) + int(s["T"][1, 5]) == 26 * nv
    assert float(s["values"].sum()) == 26 * nv + int(np.trace(s["T"]))
    assert s["values"][6] == 2 * s["T"][1, 1] and s["values"][10] == s["T"][1, 5]


def test_lonely_voxel_is_noise():
    s = gc.stages(cs.lonely())
    assert s["classes"].size == 17 and s["classes"][-1] == 0 and (s["classes"][:-1] == 1).all()
    assert s["r_min"][-1] == 0.0 and s["r_max"][-1] == 0.0
    assert s["T"][0, 5] == 26 and s["values"][5] == 26 and s["values"][6] == 168 and s["values"][10] == 332


def test_few_points():
    for n in (1, 2, 3):
        s = gc.stages(cs.plane()[:n])
        assert s["valid"].tolist() == [n >= 3] * n
        assert s["classes"].tolist() == [0 if n < 2 else 1]
        assert int(s["T"].sum()) == 26


def test_simple_type_rules():
    # the first matching rule decides (thresholds 0.1 / 0.175 / 0.015 / 0.05)
    assert gc.simple_type(0.11, 0.12) == 1 and gc.simple_type(0.05, 0.2) == 2 and gc.simple_type(0.01, 0.1) == 0
    assert gc.simple_type(0.05, 0.09) == 3 and gc.simple_type(0.02, 0.1) == 4


# ---- the second restatement ---------------------------------------------------------------------------------------------------
def _jacobi3(a):
    v = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    for _ in range(64):
        off = abs(a[0][1]) + abs(a[0][2]) + abs(a[1][2])
        diag = abs(a[0][0]) + abs(a[1][1]) + abs(a[2][2])
        if off == 0.0 or off <= 1e-300 or off < 1e-18 * diag:
            break
        for p in range(2):
            for q in range(p + 1, 3):
                apq = a[p][q]
                if apq == 0.0:
                    continue
                theta = (a[q][q] - a[p][p]) / (2.0 * apq)
                if abs(theta) > 1e150:
                    t = 0.5 / theta
                else:
                    t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
                c = 1.0 / math.sqrt(t * t + 1.0); s = t * c
                for k in range(3):
                    akp, akq = a[k][p], a[k][q]
                    a[k][p] = c * akp - s * akq; a[k][q] = s * akp + c * akq
                for k in range(3):
                    apk, aqk = a[p][k], a[q][k]
                    a[p][k] = c * apk - s * aqk; a[q][k] = s * apk + c * aqk
                for k in range(3):
                    vkp, vkq = v[k][p], v[k][q]
                    v[k][p] = c * vkp - s * vkq; v[k][q] = s * vkp + c * vkq
    return a, v


def _d2_to(P, c):
    d = P - c[None, :]                                           # float32, one IEEE operation each
    return d, (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def np_normals(P, ne_radius):
    n = P.shape[0]
    r2 = np.float32(ne_radius * ne_radius)
    out = np.full((n, 3), np.nan, np.float32); ok = np.zeros(n, np.uint8)
    for i in range(n):
        d, d2 = _d2_to(P, P[i])
        nb = np.nonzero(d2 < r2)[0]
        if nb.size < 3:
            continue
        q = [[int(x) for x in np.rint(d[nb, a].astype(np.float64) * 1048576.0)] for a in range(3)]      # Python integers
        S = [sum(q[a]) for a in range(3)]
        cnt = float(len(nb))
        cov = [[0.0] * 3 for _ in range(3)]
        for a in range(3):
            for b in range(a, 3):
                Sab = sum(x * y for x, y in zip(q[a], q[b]))
                cov[a][b] = cov[b][a] = float(Sab) - float(S[a]) * float(S[b]) / cnt
        a_, v = _jacobi3(cov)
        m = 0
        if a_[1][1] < a_[m][m]:
            m = 1
        if a_[2][2] < a_[m][m]:
            m = 2
        nv = np.array([v[0][m], v[1][m], v[2][m]], np.float64).astype(np.float32)
        vp = np.float32(0.0) - P[i]
        if (vp[0] * nv[0] + vp[1] * nv[1]) + vp[2] * nv[2] < np.float32(0.0):
            nv = -nv
        out[i] = nv; ok[i] = 1
    return out, ok


def np_voxels(P, leaf):
    inv = np.float32(1.0) / np.float32(leaf)
    ijk = np.floor(P * inv).astype(np.int64)
    minb = np.floor(P.min(axis=0) * inv).astype(np.int64); divb = np.floor(P.max(axis=0) * inv).astype(np.int64) - minb + 1
    ijk -= minb
    idx = ijk[:, 0] + ijk[:, 1] * divb[0] + ijk[:, 2] * divb[0] * divb[1]
    keys = np.unique(idx)
    cent = np.empty((keys.size, 3), np.float32)
    for v, k in enumerate(keys):
        pts = P[idx == k]                                        # input order
        for a in range(3):
            cent[v, a] = np.cumsum(pts[:, a], dtype=np.float32)[-1] / np.float32(pts.shape[0])      # cumsum adds sequentially
    return cent, keys, minb, divb


def np_rsd(P, nrm, ok, cent, R):
    r2 = np.float32(R * R)
    pi, pio2 = np.uint32(0x40490fdb).view(np.float32), np.uint32(0x3fc90fdb).view(np.float32)
    nv = cent.shape[0]
    rmin = np.zeros(nv, np.float32); rmax = np.zeros(nv, np.float32); cls = np.zeros(nv, np.int32)
    for v in range(nv):
        _, d2 = _d2_to(P, cent[v])
        nb = np.nonzero(d2 < r2)[0]
        if nb.size >= 2:
            ref = nb[np.argmin(d2[nb])]                          # the first of equal minima: the lowest index
            mn = {0: np.float32(0.0)}; mx = {0: np.float32(0.0)}
            if ok[ref]:
                for j in nb[ok[nb] == 1]:
                    a, b = nrm[ref], nrm[j]
                    cosine = min(np.float32(1.0), max(np.float32(-1.0), (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]))
                    ang = fc.acosf(cosine)
                    if ang > pio2:
                        ang = np.float32(pi - ang)
                    k = min(4, int(math.floor(5.0 * math.sqrt(float(d2[j])) / R)))
                    mn[k] = min(mn.get(k, ang), ang); mx[k] = max(mx.get(k, ang), ang)
            amin = amin_d = amax = amax_d = 0.0
            for k in sorted(mn):
                f = (float(k) + 0.5) * R / 5.0
                lo, hi = float(mn[k]), float(mx[k])
                amin += lo * lo; amin_d += lo * f; amax += hi * hi; amax_d += hi * f
            ra = 0.2 if amin == 0.0 else min(amin_d / amin, 0.2)
            rb = 0.2 if amax == 0.0 else min(amax_d / amax, 0.2)
            fa = np.float32(float(np.float32(ra)) * 1.1); fb = np.float32(float(np.float32(rb)) * 1.1)
            rmin[v], rmax[v] = min(fa, fb), max(fa, fb)
        a, b = float(rmin[v]), float(rmax[v])
        cls[v] = 1 if a > 0.1 else 2 if b > 0.175 else 0 if a < 0.015 else 3 if float(rmax[v] - rmin[v]) < 0.05 else 4
    return rmin, rmax, cls


def np_transitions(cent, keys, cls, minb, divb, leaf):
    inv = np.float32(1.0) / np.float32(leaf)
    where = {int(k): v for v, k in enumerate(keys)}
    T = np.zeros((6, 6), np.uint32)
    cc = np.floor(cent * inv).astype(np.int64) - minb
    for v in range(cent.shape[0]):
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if dx == dy == dz == 0:
                        continue
                    c = cc[v] + (dx, dy, dz)
                    inside = (c >= 0).all() and (c < divb).all()
                    at = where.get(int(c[0] + c[1] * divb[0] + c[2] * divb[0] * divb[1])) if inside else None
                    T[cls[v], 5 if at is None else cls[at]] += 1
    return T


def test_checker_equals_the_numpy_restatement():
    seen, bins = set(), np.zeros(21, bool)
    for name, (cloud, ne, R) in cs.restatement_clouds().items():
        P = np.ascontiguousarray(cloud[:, :3], np.float32)
        s = gc.stages(cloud, ne, R)
        nrm, ok = np_normals(P, ne)
        assert np.array_equal(ok, s["valid"]), name
        assert np.array_equal(_u32(nrm)[ok == 1], _u32(s["normals"])[ok == 1]), name
        cent, keys, minb, divb = np_voxels(P, R)
        assert np.array_equal(keys, s["vidx"]) and np.array_equal(_u32(cent), _u32(s["centroids"])), name
        assert s["grid"].tolist() == minb.tolist() + divb.tolist(), name
        rmin, rmax, cls = np_rsd(P, nrm, ok, cent, R)
        assert np.array_equal(_u32(rmin), _u32(s["r_min"])) and np.array_equal(_u32(rmax), _u32(s["r_max"])), name
        assert np.array_equal(cls, s["classes"]), name
        T = np_transitions(cent, keys, cls, minb, divb, R)
        assert np.array_equal(T, s["T"]), name
        want = np.array([np.float32(int(T[i, j]) + int(T[j, i])) for i in range(6) for j in range(i, 6)], np.float32)
        assert np.array_equal(_u32(want), _u32(s["values"])), name
        v, T2 = gc.describe(cloud, ne, R)
        assert np.array_equal(_u32(v), _u32(want)) and np.array_equal(T2, T), name
        seen |= set(cls.tolist()); bins |= want > 0
    # the comparison is worth something only if the clouds reach the rules: at least four of the five classes, eight of the 21 bins
    assert len(seen) >= 4, seen
    assert int(bins.sum()) >= 8, bins


# ---- traversal order ------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_the_order_of_the_points():
    cloud, ne, R = cs.restatement_clouds()["scene_b"]
    s = gc.stages(cloud, ne, R)
    perm = np.random.RandomState(3).permutation(cloud.shape[0])
    shuffled = np.ascontiguousarray(cloud[perm])
    nrm, ok = gc.normals(shuffled, ne)
    assert np.array_equal(ok, s["valid"][perm])
    assert np.array_equal(_u32(nrm)[ok == 1], _u32(s["normals"][perm])[ok == 1])
    # the histogram stage on the shuffled points, fed the centroids of the unshuffled cloud (centroids are input-order sums)
    rmin, rmax, cls = gc.rsd(shuffled, nrm, ok, s["centroids"], R)
    assert np.array_equal(_u32(rmin), _u32(s["r_min"])) and np.array_equal(_u32(rmax), _u32(s["r_max"])) and np.array_equal(cls, s["classes"])
    T = gc.transitions(s["centroids"], s["vidx"], cls, s["grid"], R)
    assert np.array_equal(_u32(gc.histogram(T)), _u32(s["values"]))
    # threads split the work, never a sum
    one = gc.normals(cloud, ne, threads=1)
    assert np.array_equal(_u32(one[0])[ok[np.argsort(perm)] == 1], _u32(s["normals"])[s["valid"] == 1])
