"""ctypes binding of include/scl_m2dp.h: the M2DP descriptor (signature, database, 1-NN detection) on the GPU."""
import ctypes
from ctypes import POINTER, byref, c_char_p, c_double, c_float, c_int, c_int8, c_uint32, c_ulonglong, c_void_p

import numpy as np

from ._native import load_library

DIM, ROWS, COLS, MAX_GROUP = 192, 64, 128, 16


class M2dpConfig(ctypes.Structure):
    """scl_m2dp_config"""
    _fields_ = [("device", c_int), ("dist_thres", c_double), ("num_exclude_recent", c_int), ("robot_num", c_int), ("this_id", c_int)]


_bound = None


def _lib():
    global _bound
    if _bound is not None:
        return _bound
    L = load_library()
    P, fp, ip, u32 = c_void_p, POINTER(c_float), POINTER(c_int), POINTER(c_uint32)
    sig = {
        "scl_m2dp_default_config": (c_int, [POINTER(M2dpConfig)]),
        "scl_m2dp_create": (c_int, [POINTER(M2dpConfig), POINTER(P)]),
        "scl_m2dp_destroy": (c_int, [P]),
        "scl_m2dp_last_error": (c_char_p, [P]),
        "scl_m2dp_make": (c_int, [P, P, c_int, c_int, fp]),
        "scl_m2dp_make_and_save": (c_int, [P, P, c_int, c_int, c_int8, c_int, fp]),
        "scl_m2dp_make_and_save_many": (c_int, [P, POINTER(c_void_p), ip, c_int, POINTER(c_int8), ip, c_int, fp]),
        "scl_m2dp_save_from_wire": (c_int, [P, fp, c_int8, c_int]),
        "scl_m2dp_get_size": (c_int, [P]),
        "scl_m2dp_get_size_of": (c_int, [P, c_int]),
        "scl_m2dp_get_index": (c_int, [P, c_int, POINTER(c_int8), ip]),
        "scl_m2dp_local_to_global": (c_int, [P, c_int, c_int, ip]),
        "scl_m2dp_get_signature": (c_int, [P, c_int, fp]),
        "scl_m2dp_detect_intra": (c_int, [P, c_int, ip, fp]),
        "scl_m2dp_detect_inter": (c_int, [P, c_int, ip, fp]),
        "scl_m2dp_signature_matrix": (c_int, [P, P, c_int, c_int, u32, fp, fp, fp]),
        "scl_m2dp_stats": (c_int, [P, POINTER(c_ulonglong), POINTER(c_ulonglong), POINTER(c_double)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name); fn.restype = res; fn.argtypes = args
    _bound = L
    return L


class M2dpError(RuntimeError):
    def __init__(self, where, status, message=""):
        super().__init__(f"{where}: status {status} ({message})")
        self.status = status


class M2dpEngine:
    """Mirror of m2dp_descriptor (descriptor.h:1803-2040) with working detections: make_and_save, make_and_save_many,
    save_from_wire, detect_intra, detect_inter, get_index, get_size, and the test hook signature_matrix."""

    def __init__(self, dist_thres=0.3, num_exclude_recent=30, robot_num=1, this_id=0, device=0):
        self.L = _lib()
        cfg = M2dpConfig()
        self.L.scl_m2dp_default_config(byref(cfg))
        cfg.device, cfg.dist_thres, cfg.num_exclude_recent, cfg.robot_num, cfg.this_id = device, dist_thres, num_exclude_recent, robot_num, this_id
        self.cfg = cfg
        self.h = c_void_p()
        rc = self.L.scl_m2dp_create(byref(cfg), byref(self.h))
        if rc != 0:
            self.h = c_void_p()
            raise M2dpError("scl_m2dp_create", rc)

    def _check(self, rc, where):
        if rc != 0:
            raise M2dpError(where, rc, self.L.scl_m2dp_last_error(self.h).decode())

    def close(self):
        if self.h and self.h.value:
            self.L.scl_m2dp_destroy(self.h); self.h = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _cloud(points):
        a = np.ascontiguousarray(points, dtype=np.float32)
        if a.ndim != 2 or a.shape[1] < 3:
            raise ValueError("points: (n, >= 3) float32 records")
        return a, a.shape[0], a.shape[1] * 4

    def make(self, points):
        a, n, st = self._cloud(points)
        out = np.empty(DIM, np.float32)
        self._check(self.L.scl_m2dp_make(self.h, a.ctypes.data_as(c_void_p), n, st, out.ctypes.data_as(POINTER(c_float))), "scl_m2dp_make")
        return out

    def make_and_save(self, points, robot=0, index=0):
        a, n, st = self._cloud(points)
        out = np.empty(DIM, np.float32)
        self._check(self.L.scl_m2dp_make_and_save(self.h, a.ctypes.data_as(c_void_p), n, st, robot, index, out.ctypes.data_as(POINTER(c_float))),
                    "scl_m2dp_make_and_save")
        return out

    def make_and_save_many(self, clouds, robots=None, indexs=None, want_values=True):
        """clouds: list of (n_i, k) float32 arrays with one record width k; returns (count, 192) float32 (None if not wanted)"""
        arrs = [self._cloud(c) for c in clouds]
        count = len(arrs)
        if count and len({st for _, _, st in arrs}) != 1:
            raise ValueError("make_and_save_many: one stride for all clouds")
        st = arrs[0][2] if count else 12
        ptrs = (c_void_p * max(count, 1))(*[a.ctypes.data for a, _, _ in arrs])
        ns = np.ascontiguousarray([n for _, n, _ in arrs], np.int32)
        rb = np.ascontiguousarray(robots if robots is not None else np.zeros(count), np.int8)
        ix = np.ascontiguousarray(indexs if indexs is not None else np.arange(count), np.int32)
        out = np.empty((count, DIM), np.float32) if want_values else None
        self._check(self.L.scl_m2dp_make_and_save_many(self.h, ptrs, ns.ctypes.data_as(POINTER(c_int)), st, rb.ctypes.data_as(POINTER(c_int8)),
                                                       ix.ctypes.data_as(POINTER(c_int)), count,
                                                       out.ctypes.data_as(POINTER(c_float)) if out is not None else None),
                    "scl_m2dp_make_and_save_many")
        return out

    def save_from_wire(self, values, robot=0, index=0):
        v = np.ascontiguousarray(values, np.float32)
        assert v.size == DIM
        self._check(self.L.scl_m2dp_save_from_wire(self.h, v.ctypes.data_as(POINTER(c_float)), robot, index), "scl_m2dp_save_from_wire")

    def get_size(self, robot=-1):
        n = self.L.scl_m2dp_get_size_of(self.h, robot)
        if n < 0:
            self._check(n, "scl_m2dp_get_size_of")
        return n

    def get_index(self, key):
        r, i = c_int8(), c_int()
        self._check(self.L.scl_m2dp_get_index(self.h, key, byref(r), byref(i)), "scl_m2dp_get_index")
        return r.value, i.value

    def local_to_global(self, robot, local):
        k = c_int()
        self._check(self.L.scl_m2dp_local_to_global(self.h, robot, local, byref(k)), "scl_m2dp_local_to_global")
        return k.value

    def get_signature(self, key):
        out = np.empty(DIM, np.float32)
        self._check(self.L.scl_m2dp_get_signature(self.h, key, out.ctypes.data_as(POINTER(c_float))), "scl_m2dp_get_signature")
        return out

    def detect_intra(self, cur):
        """(loop local index or -1, float32 distance to the nearest; +inf if none)"""
        loop, d = c_int(), c_float()
        self._check(self.L.scl_m2dp_detect_intra(self.h, cur, byref(loop), byref(d)), "scl_m2dp_detect_intra")
        return loop.value, np.float32(d.value)

    def detect_inter(self, cur):
        """(loop global key or -1, float32 distance to the nearest; +inf if none)"""
        loop, d = c_int(), c_float()
        self._check(self.L.scl_m2dp_detect_inter(self.h, cur, byref(loop), byref(d)), "scl_m2dp_detect_inter")
        return loop.value, np.float32(d.value)

    def signature_matrix(self, points):
        """test hook: (uint32 counts (64, 128), mean float32[3], axes float32[3, 3] (row k = axis k), maxRho float32)"""
        a, n, st = self._cloud(points)
        counts = np.empty((ROWS, COLS), np.uint32); mean = np.empty(3, np.float32); axes = np.empty((3, 3), np.float32); mr = c_float()
        self._check(self.L.scl_m2dp_signature_matrix(self.h, a.ctypes.data_as(c_void_p), n, st, counts.ctypes.data_as(POINTER(c_uint32)),
                                                     mean.ctypes.data_as(POINTER(c_float)), axes.ctypes.data_as(POINTER(c_float)), byref(mr)),
                    "scl_m2dp_signature_matrix")
        return counts, mean, axes, np.float32(mr.value)

    def stats(self):
        """(decisions, exact-path decisions, kernel microseconds) since creation"""
        d, e, us = c_ulonglong(), c_ulonglong(), c_double()
        self._check(self.L.scl_m2dp_stats(self.h, byref(d), byref(e), byref(us)), "scl_m2dp_stats")
        return d.value, e.value, us.value
