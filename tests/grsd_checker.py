"""CPU restatement of the GRSD plugin (include/scl_grsd.h, DESIGN.md section 4 "GRSD"): brute force in C
(tests/cpp/grsd_checker.c -> tests/cpp/libgrsd_checker.so, built by `make`).  This is the yardstick of tests/test_gpu_grsd.py;
tests/test_grsd_checker.py holds it to known answers and to a second restatement in numpy."""
import ctypes
import os
from ctypes import POINTER, c_double, c_float, c_int, c_int32, c_uint8, c_uint32, c_void_p

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "cpp", "libgrsd_checker.so")
DIM = 21
THREADS = min(16, os.cpu_count() or 1)
_L = None


def lib():
    global _L
    if _L is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with `make`")
        L = ctypes.CDLL(LIB_PATH)
        fp, ip, i32, u8, u32 = POINTER(c_float), POINTER(c_int), POINTER(c_int32), POINTER(c_uint8), POINTER(c_uint32)
        for name, res, args in [
            ("grc_normals", c_int, [c_void_p, c_int, c_int, c_double, ip, c_int, c_int, fp, u8]),
            ("grc_voxels", c_int, [c_void_p, c_int, c_int, c_float, fp, i32, i32]),
            ("grc_simple_type", c_int, [c_float, c_float]),
            ("grc_rsd", c_int, [c_void_p, c_int, c_int, fp, u8, fp, c_double, ip, c_int, c_int, fp, fp, i32]),
            ("grc_transitions", None, [fp, i32, i32, c_int, c_float, i32, u32]),
            ("grc_histogram", None, [u32, fp]),
            ("grc_describe", c_int, [c_void_p, c_int, c_int, c_double, c_double, c_int, fp, u32]),
        ]:
            fn = getattr(L, name); fn.restype = res; fn.argtypes = args
        _L = L
    return _L


def _p(a, t):
    return a.ctypes.data_as(POINTER(t))


def _cloud(points):
    a = np.ascontiguousarray(points, np.float32)
    return a, a.shape[0], a.shape[1] * 4


def normals(points, ne_radius=0.5, queries=None, threads=THREADS):
    """(float32 (nq, 3) normals, NaN where invalid; uint8 (nq,) validity) of the queries (None: all points)"""
    a, n, st = _cloud(points)
    q = None if queries is None else np.ascontiguousarray(queries, np.int32)
    nq = n if q is None else q.size
    out = np.empty((nq, 3), np.float32); ok = np.empty(nq, np.uint8)
    rc = lib().grc_normals(a.ctypes.data_as(c_void_p), n, st, ne_radius, None if q is None else _p(q, c_int), nq, threads,
                           _p(out, c_float), _p(ok, c_uint8))
    assert rc == 0, rc
    return out, ok


def voxels(points, leaf=2.0):
    """(centroids (v, 3), voxel indices (v,) ascending, grid = [min_b x 3, div_b x 3]); raises ValueError when the index range
    overflows int32 or a coordinate is not finite"""
    a, n, st = _cloud(points)
    cent = np.empty((n, 3), np.float32); vidx = np.empty(n, np.int32); grid = np.empty(6, np.int32)
    v = lib().grc_voxels(a.ctypes.data_as(c_void_p), n, st, leaf, _p(cent, c_float), _p(vidx, c_int32), _p(grid, c_int32))
    if v < 0:
        raise ValueError(f"grc_voxels: {v}")
    return cent[:v].copy(), vidx[:v].copy(), grid


def simple_type(r_min, r_max):
    return lib().grc_simple_type(float(np.float32(r_min)), float(np.float32(r_max)))


def rsd(points, nrm, valid, centroids, grsd_radius=2.0, queries=None, threads=THREADS):
    """(r_min, r_max, class) of the voxels `queries` (None: all centroids)"""
    a, n, st = _cloud(points)
    nm = np.ascontiguousarray(nrm, np.float32); ok = np.ascontiguousarray(valid, np.uint8)
    c = np.ascontiguousarray(centroids, np.float32)
    q = None if queries is None else np.ascontiguousarray(queries, np.int32)
    nq = c.shape[0] if q is None else q.size
    rmin = np.empty(nq, np.float32); rmax = np.empty(nq, np.float32); cls = np.empty(nq, np.int32)
    rc = lib().grc_rsd(a.ctypes.data_as(c_void_p), n, st, _p(nm, c_float), _p(ok, c_uint8), _p(c, c_float), grsd_radius,
                       None if q is None else _p(q, c_int), nq, threads, _p(rmin, c_float), _p(rmax, c_float), _p(cls, c_int32))
    assert rc == 0, rc
    return rmin, rmax, cls


def transitions(centroids, vidx, classes, grid, leaf=2.0):
    """uint32 (6, 6) counters T[class][neighbour's class]"""
    c = np.ascontiguousarray(centroids, np.float32); vi = np.ascontiguousarray(vidx, np.int32)
    cl = np.ascontiguousarray(classes, np.int32); g = np.ascontiguousarray(grid, np.int32)
    T = np.zeros((6, 6), np.uint32)
    lib().grc_transitions(_p(c, c_float), _p(vi, c_int32), _p(cl, c_int32), c.shape[0], leaf, _p(g, c_int32), _p(T, c_uint32))
    return T


def histogram(T):
    t = np.ascontiguousarray(T, np.uint32); out = np.empty(DIM, np.float32)
    lib().grc_histogram(_p(t, c_uint32), _p(out, c_float))
    return out


def describe(points, ne_radius=0.5, grsd_radius=2.0, threads=THREADS):
    """(21 floats, T (6, 6)) of one cloud"""
    a, n, st = _cloud(points)
    out = np.empty(DIM, np.float32); T = np.zeros((6, 6), np.uint32)
    rc = lib().grc_describe(a.ctypes.data_as(c_void_p), n, st, ne_radius, grsd_radius, threads, _p(out, c_float), _p(T, c_uint32))
    if rc != 0:
        raise ValueError(f"grc_describe: {rc}")
    return out, T


def stages(points, ne_radius=0.5, grsd_radius=2.0):
    """every stage of one cloud: dict(normals, valid, centroids, vidx, grid, r_min, r_max, classes, T, values)"""
    nrm, ok = normals(points, ne_radius)
    cent, vidx, grid = voxels(points, grsd_radius)
    rmin, rmax, cls = rsd(points, nrm, ok, cent, grsd_radius)
    T = transitions(cent, vidx, cls, grid, grsd_radius)
    return dict(normals=nrm, valid=ok, centroids=cent, vidx=vidx, grid=grid, r_min=rmin, r_max=rmax, classes=cls, T=T, values=histogram(T))
