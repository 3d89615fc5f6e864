"""The C ABI of the batched registration scoring (include/scl_engine.h "BATCHED REGISTRATION SCORING") without a GPU: the four calls
declared and exported, the binding's argument types those of the declarations, the ABI version moved to 10, a NULL engine refused
with nothing written, and scl_registration_information -- host code, no engine -- bit for bit a numpy restatement.  (The technique
of tests/test_verification_guess_abi.py.)"""
import ctypes
import inspect
import os
import re
from ctypes import POINTER, c_double, c_float, c_int, c_void_p

import numpy as np

import registration_eval_cases as rc
from scl_slam_amd import load_library
from scl_slam_amd.engine import RegistrationEval, ScanContextEngine, _bind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("scl_registration_eval_batch", "scl_registration_eval_batch_from_store", "scl_loop_eval_batch_from_store",
         "scl_registration_information")
INVALID_ARG = -1
C_TYPES = {"scl_engine *": c_void_p, "const void *": c_void_p, "const void *const *": POINTER(c_void_p), "int": c_int, "float": c_float,
           "double": c_double, "const int *": POINTER(c_int), "int *": POINTER(c_int), "const float *": POINTER(c_float),
           "double *": POINTER(c_double), "const double *": POINTER(c_double)}


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
    assert lib.scl_abi_version() >= 10
    for name in NAMES:
        fn = getattr(lib, name)
        want = [C_TYPES[t] for t in _declaration(name)]
        assert fn.restype is c_int and list(fn.argtypes) == want, (name, fn.argtypes, want)
    assert [len(_declaration(n)) for n in NAMES] == [12, 20, 18, 3]


def test_a_null_engine_is_refused_and_nothing_is_written():
    lib = load_library(); _bind(lib)
    nv = c_int(7); ni = c_int(7); ns = c_int(7); nt = c_int(7); mo = (c_double * 10)(*([7.0] * 10))
    cloud = (c_float * 8)(); ptrs = (c_void_p * 1)(ctypes.addressof(cloud)); counts = (c_int * 1)(1); keys = (c_int * 1)(0)
    poses = (c_float * 16)(); T = (c_float * 16)(*[1.0 if k % 5 == 0 else 0.0 for k in range(16)])
    assert lib.scl_registration_eval_batch(None, ctypes.addressof(cloud), 1, ptrs, counts, 1, 32, T, 0.5,
                                           ctypes.byref(nv), ctypes.byref(ni), mo) == INVALID_ARG
    assert lib.scl_registration_eval_batch_from_store(None, ctypes.addressof(cloud), 1, 32, 0.2, 0, 1, keys, 0, poses, 0.3, T, 300, 1000, 0.5,
                                                      ctypes.byref(nv), ctypes.byref(ni), mo, ctypes.byref(ns), ctypes.byref(nt)) == INVALID_ARG
    assert lib.scl_loop_eval_batch_from_store(None, 0, 0, poses, 1, keys, 0, poses, 0.3, T, 300, 1000, 0.5,
                                              ctypes.byref(nv), ctypes.byref(ni), mo, ctypes.byref(ns), ctypes.byref(nt)) == INVALID_ARG
    assert (nv.value, ni.value, ns.value, nt.value) == (7, 7, 7, 7) and list(mo) == [7.0] * 10


def test_information_is_the_numpy_restatement_bit_for_bit():
    lib = load_library(); _bind(lib)
    rs = np.random.RandomState(3)
    for trial in range(200):
        S = rs.standard_normal(10) * 10.0 ** rs.randint(-3, 9, 10)
        if trial % 7 == 0:
            S[rs.randint(0, 9)] = 0.0                                 # the negated entries keep the sign of a zero
        m = int(rs.randint(0, 2 ** 31 - 1))
        info = np.full(36, 7.0)
        assert lib.scl_registration_information(m, S.ctypes.data_as(POINTER(c_double)), info.ctypes.data_as(POINTER(c_double))) == 0
        want = rc.information(m, S)
        assert np.array_equal(info.view(np.uint64), want.reshape(36).view(np.uint64)), trial
        got = ScanContextEngine.registration_information(m, S)
        assert got.shape == (6, 6) and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    info = ScanContextEngine.registration_information(3, [1, 2, 3, 1, 4, 9, 0, 0, 0, 0])      # the hand-written case of the checker's test
    assert np.diag(info).tolist() == [13, 10, 5, 3, 3, 3] and np.array_equal(info, info.T)
    assert (info[0, 4], info[0, 5], info[1, 3], info[1, 5], info[2, 3], info[2, 4]) == (-3, 2, 3, -1, -2, 1)


def test_information_answers_its_errors():
    lib = load_library(); _bind(lib)
    S = np.arange(10, dtype=np.float64); info = np.full(36, 7.0)
    Sp, ip = S.ctypes.data_as(POINTER(c_double)), info.ctypes.data_as(POINTER(c_double))
    assert lib.scl_registration_information(-1, Sp, ip) == INVALID_ARG
    assert lib.scl_registration_information(5, None, ip) == INVALID_ARG
    assert lib.scl_registration_information(5, Sp, None) == INVALID_ARG
    assert (info == 7.0).all()
    assert lib.scl_registration_information(0, Sp, ip) == 0 and info[21] == 0.0


def test_the_binding_follows_the_guessed_forms():
    """the Python methods: the guessed methods' leading parameters with `transforms, max_dist` in the place of `guesses` and of the
    parameters of the fit; the result's overlap and RMSE are properties"""
    def names(f):
        return [n for n in inspect.signature(f).parameters if n != "self"]
    E = ScanContextEngine
    assert names(E.registration_eval_batch) == names(E.geometric_verification_batch_guess)[:2] + ["transforms", "max_dist"]
    assert names(E.registration_eval_batch_from_store) == names(E.geometric_verification_batch_from_store_guess)[:7] + \
        ["transforms", "max_dist", "min_src_points", "min_tgt_points"]
    assert names(E.loop_eval_batch_from_store) == names(E.loop_icp_batch_from_store_guess)[:7] + \
        ["transforms", "max_dist", "min_src_points", "min_tgt_points"]
    r = RegistrationEval(4, np.int32([4, 2, 0]), np.int32([2, 1, 0]), np.zeros((3, 10)) + np.arange(10.0))
    assert r.overlap.tolist() == [0.5, 0.25, 0.0] and r.rmse[:2].tolist() == [np.sqrt(4.5), 3.0] and np.isnan(r.rmse[2])
    assert r.information(0)[3, 3] == 2.0 and len(r) == 3
    assert RegistrationEval(0, np.int32([0]), np.int32([0]), np.zeros((1, 10))).overlap.tolist() == [0.0]
