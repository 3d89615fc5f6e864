"""CPU restatement of the FPFH plugin (include/scl_fpfh.h, DESIGN.md section 4 "FPFH"): the heavy parts in C
(tests/cpp/fpfh_checker.c -> tests/cpp/libfpfh_checker.so, built by `make`), the database and both detections here in numpy
float32 (every operation one IEEE float operation, in nanoflann's order).  This is the yardstick of tests/test_gpu_fpfh.py."""
import ctypes
import os
from ctypes import POINTER, c_float, c_int, c_uint32, c_uint64, c_void_p

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "cpp", "libfpfh_checker.so")
DIM = 33
_L = None


def lib():
    global _L
    if _L is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with `make`")
        L = ctypes.CDLL(LIB_PATH)
        fp, ip, u32 = POINTER(c_float), POINTER(c_int), POINTER(c_uint32)
        for name, res, args in [
            ("fpc_acosf", c_float, [c_float]),
            ("fpc_acosf_exhaustive", c_int, [c_int, POINTER(c_uint64), POINTER(c_uint64)]),
            ("fpc_knn", None, [c_void_p, c_int, c_int, ip, c_int, ip, fp]),
            ("fpc_normals", None, [c_void_p, c_int, c_int, ip, c_int, fp]),
            ("fpc_pair_features", c_int, [fp, fp, fp, fp, fp]),
            ("fpc_bins", None, [fp, ip]),
            ("fpc_spfh_counts", None, [c_void_p, c_int, c_int, fp, u32, u32]),
            ("fpc_hist_value_loop", c_float, [c_uint32, c_float]),
            ("fpc_hist_values_prefix", None, [c_int, c_float, fp]),
            ("fpc_describe", c_int, [c_void_p, c_int, c_int, fp, u32, u32]),
        ]:
            fn = getattr(L, name); fn.restype = res; fn.argtypes = args
        _L = L
    return _L


def _p(a, t):
    return a.ctypes.data_as(POINTER(t))


def _cloud(points):
    a = np.ascontiguousarray(points, np.float32)
    return a, a.shape[0], a.shape[1] * 4


def acosf(x):
    return np.float32(lib().fpc_acosf(float(np.float32(x))))


def acosf_exhaustive(threads=None):
    """(differences from libm over all 2^32 inputs, 256 block checksums as hex strings)"""
    threads = threads or min(8, os.cpu_count() or 1)
    blocks = np.zeros(256, np.uint64); diffs = c_uint64()
    assert lib().fpc_acosf_exhaustive(threads, _p(blocks, c_uint64), ctypes.byref(diffs)) == 0
    return diffs.value, [f"{int(b):016x}" for b in blocks]


def knn(points, queries=None):
    a, n, st = _cloud(points)
    q = None if queries is None else np.ascontiguousarray(queries, np.int32)
    nq = n if q is None else q.size
    k = min(10, n)
    idx = np.empty((nq, k), np.int32); d2 = np.empty((nq, k), np.float32)
    lib().fpc_knn(a.ctypes.data_as(c_void_p), n, st, None if q is None else _p(q, c_int), nq, _p(idx, c_int), _p(d2, c_float))
    return idx, d2


def normals(points, queries=None):
    a, n, st = _cloud(points)
    q = None if queries is None else np.ascontiguousarray(queries, np.int32)
    nq = n if q is None else q.size
    out = np.empty((nq, 3), np.float32)
    lib().fpc_normals(a.ctypes.data_as(c_void_p), n, st, None if q is None else _p(q, c_int), nq, _p(out, c_float))
    return out


def pair_features(p1, n1, p2, n2):
    """(ok, f1, f2, f3, f4) of PCL's computePairFeatures; (ok, bins) via pair_bins"""
    arrs = [np.ascontiguousarray(v, np.float32) for v in (p1, n1, p2, n2)]
    f = np.zeros(4, np.float32)
    ok = lib().fpc_pair_features(*[_p(v, c_float) for v in arrs], _p(f, c_float))
    return bool(ok), f


def pair_bins(f):
    f = np.ascontiguousarray(f, np.float32); b = np.zeros(3, np.int32)
    lib().fpc_bins(_p(f, c_float), _p(b, c_int))
    return b


def spfh_counts(points, nrm):
    a, n, st = _cloud(points)
    nm = np.ascontiguousarray(nrm, np.float32)
    c = np.zeros(DIM, np.uint32); sk = c_uint32()
    lib().fpc_spfh_counts(a.ctypes.data_as(c_void_p), n, st, _p(nm, c_float), _p(c, c_uint32), ctypes.byref(sk))
    return c, sk.value


def hist_incr(n):
    return np.float32(np.float32(100.0) / np.float32(n - 2))


def value_loop(count, inc):
    return np.float32(lib().fpc_hist_value_loop(int(count), float(np.float32(inc))))


def values_prefix(nmax, inc):
    out = np.empty(nmax + 1, np.float32)
    lib().fpc_hist_values_prefix(nmax, float(np.float32(inc)), _p(out, c_float))
    return out


def describe(points):
    """(33 floats, counts[33], skipped) of one cloud: brute-force normals, SPFH, sequential values"""
    a, n, st = _cloud(points)
    out = np.empty(DIM, np.float32); c = np.zeros(DIM, np.uint32); sk = c_uint32()
    rc = lib().fpc_describe(a.ctypes.data_as(c_void_p), n, st, _p(out, c_float), _p(c, c_uint32), ctypes.byref(sk))
    assert rc == 0, rc
    return out, c, sk.value


# ---- 1-NN and the detections ---------------------------------------------------------------------------------------------------
def sq_dist(q, cands, dims=DIM):
    """squared L2 in nanoflann's float order over the first `dims` floats: groups of four added to the running sum, then the tail;
    q (dims,), cands (m, >= dims) -> float32 (m,)"""
    q = np.asarray(q, np.float32); c = np.asarray(cands, np.float32)
    s = np.zeros(c.shape[0], np.float32)
    k = 0
    while k + 4 <= dims:
        d = q[k:k + 4][None, :] - c[:, k:k + 4]
        s = s + (((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) + d[:, 3] * d[:, 3])
        k += 4
    while k < dims:
        d = q[k] - c[:, k]
        s = s + d * d
        k += 1
    return s


def nearest(q, cands):
    """position of the 1-NN in 33 dimensions (ties to the lowest position) and its float32 squared distance"""
    s = sq_dist(q, cands)
    i = int(np.argmin(s))                              # argmin returns the first of equal minima
    return i, s[i]


class FpfhChecker:
    """The database and detections of include/scl_fpfh.h, restated."""

    def __init__(self, dist_thres=100.0, num_exclude_recent=30, tree_making_period=10, report_dims=21, inter_mode=0, robot_num=1, this_id=0):
        self.thres, self.excl, self.period, self.rdims, self.mode = dist_thres, num_exclude_recent, tree_making_period, report_dims, inter_mode
        self.robot_num, self.this_id = robot_num, this_id
        self.keys, self.robots, self.indexs = [], [], []
        self.l2g = [[] for _ in range(robot_num)]
        self.counter, self.snap_n = 0, 0

    def save(self, values, robot=0, index=0):
        self.l2g[robot].append(len(self.keys))
        self.keys.append(np.asarray(values, np.float32).copy()); self.robots.append(robot); self.indexs.append(index)

    def _report(self, a, b):
        return np.float32(np.sqrt(sq_dist(self.keys[a], self.keys[b][None, :], self.rdims)[0]))

    def detect_intra(self, cur):
        mine = self.l2g[self.this_id]
        hist = cur - self.excl
        if hist <= 0:
            return -1, np.float32(np.inf)
        pos, _ = nearest(self.keys[mine[cur]], np.stack([self.keys[k] for k in mine[:hist]]))
        d = self._report(mine[cur], mine[pos])
        return (pos if d < self.thres else -1), d

    def detect_inter(self, cur):
        n = len(self.keys)
        if self.mode == 0:
            if n < self.excl + 1:
                return -1, np.float32(0.0)
            if self.counter % self.period == 0:
                self.snap_n = n - self.excl
            self.counter += 1
            lst = list(range(self.snap_n))
        else:
            if self.robots[cur] == self.this_id:
                lst = sorted(k for r in range(self.robot_num) if r != self.this_id for k in self.l2g[r])
            else:
                lst = list(self.l2g[self.this_id])
            if not lst:
                return -1, np.float32(np.inf)
        pos, _ = nearest(self.keys[cur], np.stack([self.keys[k] for k in lst]))
        key = lst[pos]
        d = self._report(cur, key)
        return (key if d < self.thres else -1), d
