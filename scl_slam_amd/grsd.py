"""ctypes binding of include/scl_grsd.h: the GRSD descriptor (radius normals, RSD classes per voxel, class transitions, database,
1-NN detection) on the GPU."""
import ctypes
from ctypes import POINTER, byref, c_double, c_float, c_int, c_int32, c_uint8, c_uint32, c_ulonglong, c_void_p

import numpy as np

from ._native import load_library
from ._plugin import PluginError, VectorPluginEngine, bind, vector_signatures

DIM, CLASSES, MAX_GROUP, MAX_POINTS = 21, 6, 16, 1 << 22


class GrsdConfig(ctypes.Structure):
    """scl_grsd_config"""
    _fields_ = [("device", c_int), ("ne_radius", c_double), ("grsd_radius", c_double), ("dist_thres", c_double),
                ("num_exclude_recent", c_int), ("tree_making_period", c_int), ("inter_mode", c_int), ("robot_num", c_int),
                ("this_id", c_int)]


_P, _fp = c_void_p, POINTER(c_float)
_SIG = vector_signatures("scl_grsd", GrsdConfig)
_SIG.update({
    "scl_grsd_normals": (c_int, [_P, _P, c_int, c_int, _fp, POINTER(c_uint8)]),
    "scl_grsd_voxels": (c_int, [_P, _P, c_int, c_int, POINTER(c_int), _fp, _fp, _fp, POINTER(c_int32)]),
    "scl_grsd_transitions": (c_int, [_P, _P, c_int, c_int, POINTER(c_uint32)]),
    "scl_grsd_stats": (c_int, [_P, POINTER(c_ulonglong), POINTER(c_ulonglong), POINTER(c_double)]),
})


def _lib():
    return bind(load_library(), _SIG)


class GrsdError(PluginError):
    pass


def default_config():
    cfg = GrsdConfig()
    _lib().scl_grsd_default_config(byref(cfg))
    return cfg


class GrsdEngine(VectorPluginEngine):
    """Mirror of grsd_descriptor (descriptor.h:38-196) with a working intra detection: make_and_save, make_and_save_many,
    save_from_wire, detect_intra, detect_inter, get_index, get_size, and the test hooks normals / voxels / transitions."""
    PREFIX, CONFIG, ERROR, DIM = "scl_grsd", GrsdConfig, GrsdError, DIM

    def __init__(self, ne_radius=0.5, grsd_radius=2.0, dist_thres=160.0, num_exclude_recent=30, tree_making_period=10, inter_mode=0,
                 robot_num=1, this_id=0, device=0):
        super().__init__(_lib(), device=device, ne_radius=ne_radius, grsd_radius=grsd_radius, dist_thres=dist_thres,
                         num_exclude_recent=num_exclude_recent, tree_making_period=tree_making_period, inter_mode=inter_mode,
                         robot_num=robot_num, this_id=this_id)

    def normals(self, points):
        """test hook: (float32 (n, 3) normals in input order, NaN where invalid; uint8 (n,) validity)"""
        a, n, st = self._cloud(points)
        out = np.empty((n, 3), np.float32); ok = np.empty(n, np.uint8)
        self._call("normals", a.ctypes.data_as(c_void_p), n, st, out.ctypes.data_as(_fp), ok.ctypes.data_as(POINTER(c_uint8)))
        return out, ok

    def voxels(self, points):
        """test hook: (centroids (v, 3), r_min (v,), r_max (v,), classes (v,)) in ascending voxel index"""
        a, n, st = self._cloud(points)
        nv = c_int()
        cent = np.empty((n, 3), np.float32); rmin = np.empty(n, np.float32); rmax = np.empty(n, np.float32); cls = np.empty(n, np.int32)
        self._call("voxels", a.ctypes.data_as(c_void_p), n, st, byref(nv), cent.ctypes.data_as(_fp), rmin.ctypes.data_as(_fp),
                   rmax.ctypes.data_as(_fp), cls.ctypes.data_as(POINTER(c_int32)))
        v = nv.value
        return cent[:v].copy(), rmin[:v].copy(), rmax[:v].copy(), cls[:v].copy()

    def transitions(self, points):
        """test hook: uint32 (6, 6) counters T[class][neighbour's class]"""
        a, n, st = self._cloud(points)
        T = np.empty((CLASSES, CLASSES), np.uint32)
        self._call("transitions", a.ctypes.data_as(c_void_p), n, st, T.ctypes.data_as(POINTER(c_uint32)))
        return T

    def stats(self):
        """(points described, voxels classified, kernel microseconds) since creation"""
        p, v, us = c_ulonglong(), c_ulonglong(), c_double()
        self._call("stats", byref(p), byref(v), byref(us))
        return p.value, v.value, us.value
