"""What the plugin test modules share (tests/test_gpu_plugins_at_scale.py, tests/test_gpu_iris_configs.py, tests/test_plugin_cases.py):
drawn inputs, bit-pattern comparisons, and the vector plugins' checkers with nanoflann's rule for NaN distances and a vectorised
1-NN (tests/test_plugin_cases.py holds both to the loop form on the CPU).  A plain module, no fixtures."""
import math

import numpy as np

import fpfh_checker as fc
import m2dp_checker as mc
from test_iris_fftmatch import _iris_like as iris_like  # noqa: F401  (the drawn Iris image: one definition, shared from here)


def f32_bits(x):
    return int(np.float32(x).view(np.uint32))


def same_f32(a, b, nan_ok=False):
    """equal uint32 patterns; with nan_ok two NaNs of any payload count as equal"""
    return f32_bits(a) == f32_bits(b) or (nan_ok and math.isnan(float(a)) and math.isnan(float(b)))


def same_detection(g, o, nan_ok=False):
    """(loop, distance) of a vector plugin's detection: loop id and the float distance by its bit pattern"""
    return int(g[0]) == int(o[0]) and same_f32(g[1], o[1], nan_ok)


def same_iris_detection(g, o):
    """(loop, shift, distance) of an Iris detection: ids and shifts equal, the distance by its bit pattern"""
    return (int(g[0]), float(g[1])) == (int(o[0]), float(o[1])) and same_f32(g[2], o[2])


def m2dp_rows(n, seed):
    """n rows of 192 floats shaped like test_gpu_m2dp._wire_scenario: six prototypes, 60 % with noise, 15 % exact copies of
    prototype 0 (ties)"""
    rs = np.random.RandomState(seed)
    protos = np.abs(rs.standard_normal((6, 192))).astype(np.float32) * np.float32(0.1)
    rows = protos[rs.randint(6, size=n)].copy()
    noisy = rs.rand(n) < 0.6
    rows[noisy] += (rs.standard_normal((int(noisy.sum()), 192)) * 0.01).astype(np.float32)
    rows[rs.rand(n) < 0.15] = protos[0]
    return np.ascontiguousarray(rows, np.float32)


def fpfh_rows(n, seed):
    """n rows of 33 floats shaped like tests/golden/gen_fpfh_nn_golden.golden_keys(..., "hist"): three 11-bin histograms of 100
    votes each; 10 % exact copies of row 0 (ties)"""
    rs = np.random.RandomState(seed)
    rows = (100.0 * rs.dirichlet(np.full(11, 0.7), size=(n, 3))).astype(np.float32).reshape(n, 33)
    rows[rs.rand(n) < 0.10] = rows[0]
    return np.ascontiguousarray(rows, np.float32)


def vector_rows(plugin, n, seed):
    return m2dp_rows(n, seed) if plugin == "m2dp" else fpfh_rows(n, seed)


# ---- 1-NN as nanoflann's result set does it: a candidate is admitted only when dist < worst, so a NaN distance never wins -------
def sq_dist_rows(q, cands, dims=None):
    """squared L2 between q and every row of cands over the first `dims` floats, in nanoflann's float order (groups of four
    ((d0*d0 + d1*d1) + d2*d2) + d3*d3 added to the running sum, then the tail one element at a time): the operations of
    m2dp_checker.sqdist_nanoflann / fpfh_checker.sq_dist, one numpy operation per step over all rows, non-finite values allowed"""
    q = np.asarray(q, np.float32); c = np.asarray(cands, np.float32)
    dims = q.size if dims is None else dims
    s = np.zeros(c.shape[0], np.float32)
    k = 0
    with np.errstate(invalid="ignore", over="ignore"):
        while k + 4 <= dims:
            d = q[k:k + 4][None, :] - c[:, k:k + 4]
            s = s + (((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) + d[:, 3] * d[:, 3])
            k += 4
        while k < dims:
            d = q[k] - c[:, k]
            s = s + d * d
            k += 1
    return s


def first_minimum(s):
    """position of the smallest non-NaN element of s, the first of equal ones; -1 when s is empty or all NaN"""
    ok = ~np.isnan(s)
    if not ok.any():
        return -1
    i = int(np.argmin(np.where(ok, s, np.float32(np.inf))))
    return i if ok[i] else int(np.argmax(ok))                  # the minimum is +inf itself: the first element that really is +inf


class M2dpChecker(mc.CheckerDB):
    """m2dp_checker.CheckerDB with nanoflann's rule for NaN distances (CheckerDB._nn takes a NaN as `best` when it comes first and
    then never replaces it): a NaN never beats another distance, and when every candidate's distance is NaN nothing is found,
    (-1, NaN); an empty search set stays (-1, +inf).  `_nn_loop` is the definition, pair by pair with sqdist_nanoflann;
    vectorised=True answers from sq_dist_rows."""

    def __init__(self, vectorised=False, **kw):
        super().__init__(**kw)
        self.vectorised, self._mat = vectorised, None

    def _nn_loop(self, q, keys):
        best, bk, seen = None, -1, False
        with np.errstate(invalid="ignore", over="ignore"):
            for k in sorted(keys):
                d = mc.sqdist_nanoflann(self.sigs[q], self.sigs[k])
                seen = True
                if not np.isnan(d) and (best is None or d < best):
                    best, bk = d, k
        if best is None:
            return -1, np.float32(np.nan if seen else np.inf)
        return bk, np.float32(np.sqrt(best))

    def _nn(self, q, keys):
        if not self.vectorised:
            return self._nn_loop(q, keys)
        keys = np.sort(np.asarray(list(keys), np.int64))
        if keys.size == 0:
            return -1, np.float32(np.inf)
        if self._mat is None or self._mat.shape[0] != len(self.sigs):
            self._mat = np.stack(self.sigs)
        s = sq_dist_rows(self.sigs[q], self._mat[keys])
        i = first_minimum(s)
        if i < 0:
            return -1, np.float32(np.nan)
        return int(keys[i]), np.float32(np.sqrt(s[i]))


class FpfhChecker(fc.FpfhChecker):
    """fpfh_checker.FpfhChecker with the same rule (its nearest() is numpy's argmin, which answers the first NaN): when every 33-D
    distance is NaN the detections report loop -1 and a NaN distance, whatever report_dims is (include/scl_fpfh.h)"""

    def __init__(self, **kw):
        super().__init__(**kw)
        self._mat = None

    def _nearest(self, q, keys):
        if self._mat is None or self._mat.shape[0] != len(self.keys):
            self._mat = np.stack(self.keys)
        return first_minimum(sq_dist_rows(self.keys[q], self._mat[np.asarray(keys, np.int64)]))

    def _report(self, a, b):
        return np.float32(np.sqrt(sq_dist_rows(self.keys[a], self.keys[b][None, :], self.rdims)[0]))

    def detect_intra(self, cur):
        mine = self.l2g[self.this_id]
        hist = cur - self.excl
        if hist <= 0:
            return -1, np.float32(np.inf)
        pos = self._nearest(mine[cur], mine[:hist])
        if pos < 0:
            return -1, np.float32(np.nan)
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
        pos = self._nearest(cur, lst)
        if pos < 0:
            return -1, np.float32(np.nan)
        d = self._report(cur, lst[pos])
        return (lst[pos] if d < self.thres else -1), d
