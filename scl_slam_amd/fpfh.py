"""ctypes binding of include/scl_fpfh.h: the FPFH descriptor (normals, SPFH, database, 1-NN detection) on the GPU."""
import ctypes
from ctypes import POINTER, byref, c_char_p, c_double, c_float, c_int, c_int8, c_uint32, c_uint64, c_ulonglong, c_void_p

import numpy as np

from ._native import load_library

DIM, BINS, K, MAX_GROUP = 33, 11, 10, 16


class FpfhConfig(ctypes.Structure):
    """scl_fpfh_config"""
    _fields_ = [("device", c_int), ("dist_thres", c_double), ("num_exclude_recent", c_int), ("tree_making_period", c_int),
                ("report_dims", c_int), ("inter_mode", c_int), ("robot_num", c_int), ("this_id", c_int)]


_bound = None


def _lib():
    global _bound
    if _bound is not None:
        return _bound
    L = load_library()
    P, fp, ip, u32 = c_void_p, POINTER(c_float), POINTER(c_int), POINTER(c_uint32)
    sig = {
        "scl_fpfh_default_config": (c_int, [POINTER(FpfhConfig)]),
        "scl_fpfh_create": (c_int, [POINTER(FpfhConfig), POINTER(P)]),
        "scl_fpfh_destroy": (c_int, [P]),
        "scl_fpfh_last_error": (c_char_p, [P]),
        "scl_fpfh_make": (c_int, [P, P, c_int, c_int, fp]),
        "scl_fpfh_make_and_save": (c_int, [P, P, c_int, c_int, c_int8, c_int, fp]),
        "scl_fpfh_make_and_save_many": (c_int, [P, POINTER(c_void_p), ip, c_int, POINTER(c_int8), ip, c_int, fp]),
        "scl_fpfh_save_from_wire": (c_int, [P, fp, c_int8, c_int]),
        "scl_fpfh_get_size": (c_int, [P]),
        "scl_fpfh_get_size_of": (c_int, [P, c_int]),
        "scl_fpfh_get_index": (c_int, [P, c_int, POINTER(c_int8), ip]),
        "scl_fpfh_local_to_global": (c_int, [P, c_int, c_int, ip]),
        "scl_fpfh_get_signature": (c_int, [P, c_int, fp]),
        "scl_fpfh_detect_intra": (c_int, [P, c_int, ip, fp]),
        "scl_fpfh_detect_inter": (c_int, [P, c_int, ip, fp]),
        "scl_fpfh_neighbors": (c_int, [P, P, c_int, c_int, ip, fp]),
        "scl_fpfh_normals": (c_int, [P, P, c_int, c_int, fp]),
        "scl_fpfh_counts": (c_int, [P, P, c_int, c_int, u32, u32]),
        "scl_fpfh_values": (c_int, [u32, c_int, c_float, fp]),
        "scl_fpfh_acosf_blocks": (c_int, [P, c_int, c_int, POINTER(c_uint64)]),
        "scl_fpfh_stats": (c_int, [P, POINTER(c_ulonglong), POINTER(c_ulonglong), POINTER(c_double)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name); fn.restype = res; fn.argtypes = args
    _bound = L
    return L


class FpfhError(RuntimeError):
    def __init__(self, where, status, message=""):
        super().__init__(f"{where}: status {status} ({message})")
        self.status = status


def default_config():
    cfg = FpfhConfig()
    _lib().scl_fpfh_default_config(byref(cfg))
    return cfg


def hist_values(counts, hist_incr):
    """scl_fpfh_values on the host (no device): the float after counts[i] sequential `+= hist_incr`"""
    c = np.ascontiguousarray(counts, np.uint32)
    out = np.empty(c.shape, np.float32)
    rc = _lib().scl_fpfh_values(c.ctypes.data_as(POINTER(c_uint32)), c.size, float(np.float32(hist_incr)), out.ctypes.data_as(POINTER(c_float)))
    if rc != 0:
        raise FpfhError("scl_fpfh_values", rc)
    return out


class FpfhEngine:
    """Mirror of fpfh_descriptor (descriptor.h:253-460) with a working intra detection: make_and_save, make_and_save_many,
    save_from_wire, detect_intra, detect_inter, get_index, get_size, and the test hooks neighbors / normals / counts."""

    def __init__(self, dist_thres=100.0, num_exclude_recent=30, tree_making_period=10, report_dims=21, inter_mode=0,
                 robot_num=1, this_id=0, device=0):
        self.L = _lib()
        cfg = default_config()
        cfg.device, cfg.dist_thres, cfg.num_exclude_recent, cfg.tree_making_period = device, dist_thres, num_exclude_recent, tree_making_period
        cfg.report_dims, cfg.inter_mode, cfg.robot_num, cfg.this_id = report_dims, inter_mode, robot_num, this_id
        self.cfg = cfg
        self.h = c_void_p()
        rc = self.L.scl_fpfh_create(byref(cfg), byref(self.h))
        if rc != 0:
            self.h = c_void_p()
            raise FpfhError("scl_fpfh_create", rc)

    def _check(self, rc, where):
        if rc != 0:
            raise FpfhError(where, rc, self.L.scl_fpfh_last_error(self.h).decode())

    def close(self):
        if self.h and self.h.value:
            self.L.scl_fpfh_destroy(self.h); self.h = c_void_p()

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
        self._check(self.L.scl_fpfh_make(self.h, a.ctypes.data_as(c_void_p), n, st, out.ctypes.data_as(POINTER(c_float))), "scl_fpfh_make")
        return out

    def make_and_save(self, points, robot=0, index=0):
        a, n, st = self._cloud(points)
        out = np.empty(DIM, np.float32)
        self._check(self.L.scl_fpfh_make_and_save(self.h, a.ctypes.data_as(c_void_p), n, st, robot, index, out.ctypes.data_as(POINTER(c_float))),
                    "scl_fpfh_make_and_save")
        return out

    def make_and_save_many(self, clouds, robots=None, indexs=None, want_values=True):
        """clouds: list of (n_i, k) float32 arrays with one record width k; returns (count, 33) float32 (None if not wanted)"""
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
        self._check(self.L.scl_fpfh_make_and_save_many(self.h, ptrs, ns.ctypes.data_as(POINTER(c_int)), st, rb.ctypes.data_as(POINTER(c_int8)),
                                                       ix.ctypes.data_as(POINTER(c_int)), count,
                                                       out.ctypes.data_as(POINTER(c_float)) if out is not None else None),
                    "scl_fpfh_make_and_save_many")
        return out

    def save_from_wire(self, values, robot=0, index=0):
        v = np.ascontiguousarray(values, np.float32)
        assert v.size == DIM
        self._check(self.L.scl_fpfh_save_from_wire(self.h, v.ctypes.data_as(POINTER(c_float)), robot, index), "scl_fpfh_save_from_wire")

    def get_size(self, robot=-1):
        n = self.L.scl_fpfh_get_size_of(self.h, robot)
        if n < 0:
            self._check(n, "scl_fpfh_get_size_of")
        return n

    def get_index(self, key):
        r, i = c_int8(), c_int()
        self._check(self.L.scl_fpfh_get_index(self.h, key, byref(r), byref(i)), "scl_fpfh_get_index")
        return r.value, i.value

    def local_to_global(self, robot, local):
        k = c_int()
        self._check(self.L.scl_fpfh_local_to_global(self.h, robot, local, byref(k)), "scl_fpfh_local_to_global")
        return k.value

    def get_signature(self, key):
        out = np.empty(DIM, np.float32)
        self._check(self.L.scl_fpfh_get_signature(self.h, key, out.ctypes.data_as(POINTER(c_float))), "scl_fpfh_get_signature")
        return out

    def detect_intra(self, cur):
        """(loop local index or -1, float32 distance over report_dims floats; +inf if the range is empty)"""
        loop, d = c_int(), c_float()
        self._check(self.L.scl_fpfh_detect_intra(self.h, cur, byref(loop), byref(d)), "scl_fpfh_detect_intra")
        return loop.value, np.float32(d.value)

    def detect_inter(self, cur):
        """(loop global key or -1, float32 distance over report_dims floats)"""
        loop, d = c_int(), c_float()
        self._check(self.L.scl_fpfh_detect_inter(self.h, cur, byref(loop), byref(d)), "scl_fpfh_detect_inter")
        return loop.value, np.float32(d.value)

    def neighbors(self, points):
        """test hook: (int32 (n, min(10, n)) indices, float32 d2), rows in input order"""
        a, n, st = self._cloud(points)
        k = min(K, n)
        idx = np.empty((n, k), np.int32); d2 = np.empty((n, k), np.float32)
        self._check(self.L.scl_fpfh_neighbors(self.h, a.ctypes.data_as(c_void_p), n, st, idx.ctypes.data_as(POINTER(c_int)),
                                              d2.ctypes.data_as(POINTER(c_float))), "scl_fpfh_neighbors")
        return idx, d2

    def normals(self, points):
        """test hook: float32 (n, 3) normals in input order"""
        a, n, st = self._cloud(points)
        out = np.empty((n, 3), np.float32)
        self._check(self.L.scl_fpfh_normals(self.h, a.ctypes.data_as(c_void_p), n, st, out.ctypes.data_as(POINTER(c_float))), "scl_fpfh_normals")
        return out

    def counts(self, points):
        """test hook: (uint32 counts[33], skipped pairs)"""
        a, n, st = self._cloud(points)
        c = np.empty(DIM, np.uint32); sk = c_uint32()
        self._check(self.L.scl_fpfh_counts(self.h, a.ctypes.data_as(c_void_p), n, st, c.ctypes.data_as(POINTER(c_uint32)), byref(sk)),
                    "scl_fpfh_counts")
        return c, sk.value

    def acosf_blocks(self, first_block, n_blocks):
        out = np.empty(n_blocks, np.uint64)
        self._check(self.L.scl_fpfh_acosf_blocks(self.h, first_block, n_blocks, out.ctypes.data_as(POINTER(c_uint64))), "scl_fpfh_acosf_blocks")
        return out

    def stats(self):
        """(points described, candidate distances evaluated, kernel microseconds) since creation"""
        p, c, us = c_ulonglong(), c_ulonglong(), c_double()
        self._check(self.L.scl_fpfh_stats(self.h, byref(p), byref(c), byref(us)), "scl_fpfh_stats")
        return p.value, c.value, us.value
