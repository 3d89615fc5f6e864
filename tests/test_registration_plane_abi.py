"""The C ABI of the point-to-plane registration scoring (include/scl_engine.h "POINT-TO-PLANE REGISTRATION SCORING") without a GPU:
the five calls declared and exported, the binding's argument types those of the declarations, the ABI version moved to 11, a NULL
engine refused with nothing written, and scl_registration_information_plane -- host code, no engine -- bit for bit a numpy
restatement.  (The technique of tests/test_registration_eval_abi.py.)"""
import ctypes
import inspect
import os
import re
from ctypes import POINTER, c_double, c_float, c_int, c_void_p

import numpy as np

import registration_plane_cases as pc
from scl_slam_amd import RegistrationPlaneEval, load_library
from scl_slam_amd.engine import ScanContextEngine, _bind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("scl_target_normals", "scl_registration_eval_plane_batch", "scl_registration_eval_plane_batch_from_store",
         "scl_loop_eval_plane_batch_from_store", "scl_registration_information_plane")
INVALID_ARG = -1
C_TYPES = {"scl_engine *": c_void_p, "const void *": c_void_p, "const void *const *": POINTER(c_void_p), "int": c_int, "float": c_float,
           "double": c_double, "const int *": POINTER(c_int), "int *": POINTER(c_int), "const float *": POINTER(c_float),
           "float *": POINTER(c_float), "double *": POINTER(c_double), "const double *": POINTER(c_double)}


def _declaration(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scl_engine.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared in scl_engine.h"
    args = []
    for a in m.group(1).split(","):
        a = " ".join(a.split())
        array = re.search(r"\[\d*\]$", a)
        a = re.sub(r"\[\d*\]$", "", a)
        t = re.match(r"(.*?)(\w+)$", a).group(1).strip()
        args.append(t + " *" if array else t)
    return args


def test_declared_exported_and_typed():
    lib = load_library(); _bind(lib)
    assert lib.scl_abi_version() >= 11
    for name in NAMES:
        fn = getattr(lib, name)
        want = [C_TYPES[t] for t in _declaration(name)]
        assert fn.restype is c_int and list(fn.argtypes) == want, (name, fn.argtypes, want)
    assert [len(_declaration(n)) for n in NAMES] == [6, 14, 22, 20, 3]
    # the existing calls' arguments with normal_radius behind max_dist and n_planar, sums where moments stood
    for plane, point in zip(NAMES[1:4], ("scl_registration_eval_batch", "scl_registration_eval_batch_from_store", "scl_loop_eval_batch_from_store")):
        a, b = _declaration(plane), _declaration(point)
        k = next(i for i in range(len(b)) if b[i] == "double")            # max_dist
        assert a[:k + 1] == b[:k + 1] and a[k + 1] == "double" and a[k + 2:k + 6] == ["int *", "int *", "int *", "double *"]
        assert b[k + 1:k + 4] == ["int *", "int *", "double *"] and a[k + 6:] == b[k + 4:]


def test_a_null_engine_is_refused_and_nothing_is_written():
    lib = load_library(); _bind(lib)
    nv = c_int(7); ni = c_int(7); npl = c_int(7); ns = c_int(7); nt = c_int(7); su = (c_double * 29)(*([7.0] * 29))
    cloud = (c_float * 8)(); ptrs = (c_void_p * 1)(ctypes.addressof(cloud)); counts = (c_int * 1)(1); keys = (c_int * 1)(0)
    poses = (c_float * 16)(); T = (c_float * 16)(*[1.0 if k % 5 == 0 else 0.0 for k in range(16)])
    nrm = (c_float * 3)(7.0, 7.0, 7.0)
    assert lib.scl_target_normals(None, ctypes.addressof(cloud), 1, 32, 1.0, nrm) == INVALID_ARG
    assert lib.scl_registration_eval_plane_batch(None, ctypes.addressof(cloud), 1, ptrs, counts, 1, 32, T, 0.5, 1.0,
                                                 ctypes.byref(nv), ctypes.byref(ni), ctypes.byref(npl), su) == INVALID_ARG
    assert lib.scl_registration_eval_plane_batch_from_store(None, ctypes.addressof(cloud), 1, 32, 0.2, 0, 1, keys, 0, poses, 0.3, T, 300, 1000,
                                                            0.5, 1.0, ctypes.byref(nv), ctypes.byref(ni), ctypes.byref(npl), su,
                                                            ctypes.byref(ns), ctypes.byref(nt)) == INVALID_ARG
    assert lib.scl_loop_eval_plane_batch_from_store(None, 0, 0, poses, 1, keys, 0, poses, 0.3, T, 300, 1000, 0.5, 1.0,
                                                    ctypes.byref(nv), ctypes.byref(ni), ctypes.byref(npl), su,
                                                    ctypes.byref(ns), ctypes.byref(nt)) == INVALID_ARG
    assert (nv.value, ni.value, npl.value, ns.value, nt.value) == (7, 7, 7, 7, 7) and list(su) == [7.0] * 29 and list(nrm) == [7.0] * 3


def test_information_plane_is_the_numpy_restatement_bit_for_bit():
    lib = load_library(); _bind(lib)
    rs = np.random.RandomState(3)
    dp = POINTER(c_double)
    for trial in range(200):
        S = rs.standard_normal(29) * 10.0 ** rs.randint(-3, 9, 29)
        if trial % 7 == 0:
            S[rs.randint(0, 27)] = -0.0                                # a zero keeps its sign
        info = np.full(36, 7.0); grad = np.full(6, 7.0)
        assert lib.scl_registration_information_plane(S.ctypes.data_as(dp), info.ctypes.data_as(dp), grad.ctypes.data_as(dp)) == 0
        want_info, want_grad = pc.information_plane(S)
        assert np.array_equal(info.view(np.uint64), want_info.reshape(36).view(np.uint64)), trial
        assert np.array_equal(grad.view(np.uint64), want_grad.view(np.uint64)), trial
        tri = info.reshape(6, 6)[np.triu_indices(6)]
        assert np.array_equal(tri.view(np.uint64), S[:21].view(np.uint64)) and np.array_equal(info.reshape(6, 6), info.reshape(6, 6).T)
        assert np.array_equal(info.reshape(6, 6).T[np.triu_indices(6)].view(np.uint64), S[:21].view(np.uint64))
        got_info, got_grad = ScanContextEngine.registration_information_plane(S)
        assert got_info.shape == (6, 6) and np.array_equal(got_info.view(np.uint64), info.reshape(6, 6).view(np.uint64))
        assert np.array_equal(got_grad.view(np.uint64), S[21:27].view(np.uint64))
    # the hand-written case of the checker's test: three points 0.25 above the plane z = 0
    info, grad = ScanContextEngine.registration_information_plane([20, -12, 0, 0, 0, 6, 10, 0, 0, 0, -4] + [0] * 9 + [3] + [-1.5, 1, 0, 0, 0, -0.75, 0.1875, 0.1875])
    assert np.diag(info).tolist() == [20, 10, 0, 0, 0, 3] and info[0, 1] == info[1, 0] == -12 and info[5, 0] == 6 and info[5, 1] == -4
    assert grad.tolist() == [-1.5, 1, 0, 0, 0, -0.75]


def test_information_plane_answers_its_errors():
    lib = load_library(); _bind(lib)
    dp = POINTER(c_double)
    S = np.arange(29, dtype=np.float64); info = np.full(36, 7.0); grad = np.full(6, 7.0)
    Sp, ip, gp = S.ctypes.data_as(dp), info.ctypes.data_as(dp), grad.ctypes.data_as(dp)
    assert lib.scl_registration_information_plane(None, ip, gp) == INVALID_ARG
    assert lib.scl_registration_information_plane(Sp, None, gp) == INVALID_ARG
    assert (info == 7.0).all() and (grad == 7.0).all()
    assert lib.scl_registration_information_plane(Sp, ip, None) == 0 and info[35] == 20.0 and info[6] == 1.0 and (grad == 7.0).all()


def test_the_binding_follows_the_point_forms():
    """the Python methods: the point forms' parameters with normal_radius behind max_dist; the result's information, gradient and
    plane RMSE per candidate"""
    def names(f):
        return [n for n in inspect.signature(f).parameters if n != "self"]
    E = ScanContextEngine
    assert names(E.target_normals) == ["tgt", "radius"]
    for plane, point in ((E.registration_eval_plane_batch, E.registration_eval_batch),
                         (E.registration_eval_plane_batch_from_store, E.registration_eval_batch_from_store),
                         (E.loop_eval_plane_batch_from_store, E.loop_eval_batch_from_store)):
        a, b = names(plane), names(point)
        k = b.index("max_dist")
        assert a == b[:k + 1] + ["normal_radius"] + b[k + 1:]
    sums = np.zeros((3, 29)) + np.arange(29.0)
    r = RegistrationPlaneEval(4, np.int32([4, 2, 0]), np.int32([3, 2, 0]), np.int32([3, 1, 0]), sums)
    assert len(r) == 3 and r.rmse_plane(0) == 3.0 and r.rmse_plane(1) == np.sqrt(27.0) and np.isnan(r.rmse_plane(2))
    assert r.information(0)[0].tolist() == [0, 1, 2, 3, 4, 5] and r.information(1)[5, 5] == 20 and r.gradient(2).tolist() == [21, 22, 23, 24, 25, 26]
    assert np.array_equal(r.information(0), pc.information_plane(sums[0])[0])
