"""ctypes binding of include/scl_fpfh.h: the FPFH descriptor (normals, SPFH, database, 1-NN detection) on the GPU."""
import ctypes
from ctypes import POINTER, byref, c_double, c_float, c_int, c_uint32, c_uint64, c_ulonglong, c_void_p

import numpy as np

from ._native import load_library
from ._plugin import PluginError, VectorPluginEngine, bind, vector_signatures

DIM, BINS, K, MAX_GROUP = 33, 11, 10, 16


class FpfhConfig(ctypes.Structure):
    """scl_fpfh_config"""
    _fields_ = [("device", c_int), ("dist_thres", c_double), ("num_exclude_recent", c_int), ("tree_making_period", c_int),
                ("report_dims", c_int), ("inter_mode", c_int), ("robot_num", c_int), ("this_id", c_int)]


_P, _fp, _u32 = c_void_p, POINTER(c_float), POINTER(c_uint32)
_SIG = vector_signatures("scl_fpfh", FpfhConfig)
_SIG.update({
    "scl_fpfh_neighbors": (c_int, [_P, _P, c_int, c_int, POINTER(c_int), _fp]),
    "scl_fpfh_normals": (c_int, [_P, _P, c_int, c_int, _fp]),
    "scl_fpfh_counts": (c_int, [_P, _P, c_int, c_int, _u32, _u32]),
    "scl_fpfh_values": (c_int, [_u32, c_int, c_float, _fp]),
    "scl_fpfh_acosf_blocks": (c_int, [_P, c_int, c_int, POINTER(c_uint64)]),
    "scl_fpfh_stats": (c_int, [_P, POINTER(c_ulonglong), POINTER(c_ulonglong), POINTER(c_double)]),
})


def _lib():
    return bind(load_library(), _SIG)


class FpfhError(PluginError):
    pass


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


class FpfhEngine(VectorPluginEngine):
    """Mirror of fpfh_descriptor (descriptor.h:253-460) with a working intra detection: make_and_save, make_and_save_many,
    save_from_wire, detect_intra, detect_inter, get_index, get_size, and the test hooks neighbors / normals / counts.
    Detection distances are over the first report_dims floats."""
    PREFIX, CONFIG, ERROR, DIM = "scl_fpfh", FpfhConfig, FpfhError, DIM

    def __init__(self, dist_thres=100.0, num_exclude_recent=30, tree_making_period=10, report_dims=21, inter_mode=0,
                 robot_num=1, this_id=0, device=0):
        super().__init__(_lib(), device=device, dist_thres=dist_thres, num_exclude_recent=num_exclude_recent,
                         tree_making_period=tree_making_period, report_dims=report_dims, inter_mode=inter_mode, robot_num=robot_num,
                         this_id=this_id)

    def neighbors(self, points):
        """test hook: (int32 (n, min(10, n)) indices, float32 d2), rows in input order"""
        a, n, st = self._cloud(points)
        k = min(K, n)
        idx = np.empty((n, k), np.int32); d2 = np.empty((n, k), np.float32)
        self._call("neighbors", a.ctypes.data_as(c_void_p), n, st, idx.ctypes.data_as(POINTER(c_int)), d2.ctypes.data_as(POINTER(c_float)))
        return idx, d2

    def normals(self, points):
        """test hook: float32 (n, 3) normals in input order"""
        a, n, st = self._cloud(points)
        out = np.empty((n, 3), np.float32)
        self._call("normals", a.ctypes.data_as(c_void_p), n, st, out.ctypes.data_as(POINTER(c_float)))
        return out

    def counts(self, points):
        """test hook: (uint32 counts[33], skipped pairs)"""
        a, n, st = self._cloud(points)
        c = np.empty(DIM, np.uint32); sk = c_uint32()
        self._call("counts", a.ctypes.data_as(c_void_p), n, st, c.ctypes.data_as(POINTER(c_uint32)), byref(sk))
        return c, sk.value

    def acosf_blocks(self, first_block, n_blocks):
        out = np.empty(n_blocks, np.uint64)
        self._call("acosf_blocks", first_block, n_blocks, out.ctypes.data_as(POINTER(c_uint64)))
        return out

    def stats(self):
        """(points described, candidate distances evaluated, kernel microseconds) since creation"""
        p, c, us = c_ulonglong(), c_ulonglong(), c_double()
        self._call("stats", byref(p), byref(c), byref(us))
        return p.value, c.value, us.value
