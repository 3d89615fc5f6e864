"""ctypes binding of include/scl_m2dp.h: the M2DP descriptor (signature, database, 1-NN detection) on the GPU."""
import ctypes
from ctypes import POINTER, byref, c_double, c_float, c_int, c_uint32, c_ulonglong, c_void_p

import numpy as np

from ._native import load_library
from ._plugin import PluginError, VectorPluginEngine, bind, vector_signatures

DIM, ROWS, COLS, MAX_GROUP = 192, 64, 128, 16


class M2dpConfig(ctypes.Structure):
    """scl_m2dp_config"""
    _fields_ = [("device", c_int), ("dist_thres", c_double), ("num_exclude_recent", c_int), ("robot_num", c_int), ("this_id", c_int)]


_SIG = vector_signatures("scl_m2dp", M2dpConfig)
_SIG.update({
    "scl_m2dp_signature_matrix": (c_int, [c_void_p, c_void_p, c_int, c_int, POINTER(c_uint32), POINTER(c_float), POINTER(c_float),
                                          POINTER(c_float)]),
    "scl_m2dp_stats": (c_int, [c_void_p, POINTER(c_ulonglong), POINTER(c_ulonglong), POINTER(c_double)]),
})


def _lib():
    return bind(load_library(), _SIG)


class M2dpError(PluginError):
    pass


class M2dpEngine(VectorPluginEngine):
    """Mirror of m2dp_descriptor (descriptor.h:1803-2040) with working detections: make_and_save, make_and_save_many,
    save_from_wire, detect_intra, detect_inter, get_index, get_size, and the test hook signature_matrix."""
    PREFIX, CONFIG, ERROR, DIM = "scl_m2dp", M2dpConfig, M2dpError, DIM

    def __init__(self, dist_thres=0.3, num_exclude_recent=30, robot_num=1, this_id=0, device=0):
        super().__init__(_lib(), device=device, dist_thres=dist_thres, num_exclude_recent=num_exclude_recent, robot_num=robot_num,
                         this_id=this_id)

    def signature_matrix(self, points):
        """test hook: (uint32 counts (64, 128), mean float32[3], axes float32[3, 3] (row k = axis k), maxRho float32)"""
        a, n, st = self._cloud(points)
        counts = np.empty((ROWS, COLS), np.uint32); mean = np.empty(3, np.float32); axes = np.empty((3, 3), np.float32); mr = c_float()
        self._call("signature_matrix", a.ctypes.data_as(c_void_p), n, st, counts.ctypes.data_as(POINTER(c_uint32)),
                   mean.ctypes.data_as(POINTER(c_float)), axes.ctypes.data_as(POINTER(c_float)), byref(mr))
        return counts, mean, axes, np.float32(mr.value)

    def stats(self):
        """(decisions, exact-path decisions, kernel microseconds) since creation"""
        d, e, us = c_ulonglong(), c_ulonglong(), c_double()
        self._call("stats", byref(d), byref(e), byref(us))
        return d.value, e.value, us.value
