"""The C ABI of the pairwise consistency of loop closures (include/scl_engine.h "PAIRWISE CONSISTENCY OF LOOP CLOSURES") without a GPU:
the calls declared and exported, the binding's argument types those of the declarations, the ABI version moved to 12, a NULL engine
refused with nothing written, and scl_loop_covariance -- host code, no engine -- against numpy.  (The technique of
tests/test_registration_eval_abi.py.)"""
import os
import re
from ctypes import POINTER, byref, c_double, c_int, c_uint64, c_void_p

import numpy as np
import pytest

from scl_slam_amd import load_library
from scl_slam_amd.engine import ScanContextEngine, SclError, _bind, pcm_bool_to_words, pcm_words_to_bool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("scl_pcm_consistency", "scl_pcm_max_clique", "scl_pcm_select", "scl_loop_covariance", "scl_pcm_last_timing")
INVALID_ARG = -1
C_TYPES = {"scl_engine *": c_void_p, "int": c_int, "double": c_double, "const int *": POINTER(c_int), "int *": POINTER(c_int),
           "double *": POINTER(c_double), "const double *": POINTER(c_double), "uint64_t *": POINTER(c_uint64),
           "const uint64_t *": POINTER(c_uint64)}


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
    assert lib.scl_abi_version() >= 12
    for name in NAMES:
        fn = getattr(lib, name)
        want = [C_TYPES[t] for t in _declaration(name)]
        assert fn.restype is c_int and list(fn.argtypes) == want, (name, fn.argtypes, want)
    assert [len(_declaration(n)) for n in NAMES] == [15, 6, 16, 3, 3]


def test_a_null_engine_is_refused_and_nothing_is_written():
    lib = load_library(); _bind(lib)
    poses = np.tile([0.0, 0, 0, 0, 0, 0, 1], (2, 1)); idx = np.int32([0, 1]); cov = np.tile(np.eye(6).reshape(36), (2, 1))
    d2 = np.full(4, 7.0); adj = np.full(2, 7, np.uint64); deg = np.full(2, 7, np.int32); mem = np.full(2, 7, np.int32); nm = c_int(7); seed = c_int(7)
    dp = lambda a: a.ctypes.data_as(POINTER(c_double)); ip = lambda a: a.ctypes.data_as(POINTER(c_int))
    common = (None, dp(poses), 2, dp(poses), 2, ip(idx), ip(idx), dp(poses), dp(cov), 2, None, 7.8)
    assert lib.scl_pcm_consistency(*common, dp(d2), adj.ctypes.data_as(POINTER(c_uint64)), ip(deg)) == INVALID_ARG
    assert lib.scl_pcm_select(*common, ip(mem), byref(nm), byref(seed), ip(deg)) == INVALID_ARG
    g = np.uint64([2, 1])
    assert lib.scl_pcm_max_clique(None, g.ctypes.data_as(POINTER(c_uint64)), 2, ip(mem), byref(nm), byref(seed)) == INVALID_ARG
    a, b = c_double(7.0), c_double(7.0)
    assert lib.scl_pcm_last_timing(None, byref(a), byref(b)) == INVALID_ARG
    assert (d2 == 7).all() and (adj == 7).all() and (deg == 7).all() and (mem == 7).all() and (nm.value, seed.value, a.value, b.value) == (7, 7, 7, 7)


def _spd(rs, cond):
    Q, _ = np.linalg.qr(rs.standard_normal((6, 6)))
    ev = np.exp(rs.uniform(0.0, np.log(cond), 6)); ev[0], ev[1] = 1.0, cond
    A = (Q * ev) @ Q.T * 10.0 ** rs.randint(-3, 6)
    return (A + A.T) / 2


def test_loop_covariance_against_numpy():
    """bound: max |cov info / s2 - I| <= 64 * 2^-53 * cond(info), on matrices of condition up to 1e8 -- the textbook backward error of
    a 6 x 6 Cholesky solve with room; numpy's own inverse is held to the same bound on the same matrices"""
    rs = np.random.RandomState(12)
    worst = worst_np = 0.0
    for trial in range(300):
        cond = 10.0 ** rs.uniform(0, 8)
        info = _spd(rs, cond); s2 = 10.0 ** rs.uniform(-4, 2)
        k = np.linalg.cond(info)
        cov = ScanContextEngine.loop_covariance(info, s2)
        assert np.array_equal(cov, cov.T)
        bound = 64 * 2.0 ** -53 * k
        err = np.abs(cov @ info / s2 - np.eye(6)).max(); err_np = np.abs(np.linalg.inv(info) @ info - np.eye(6)).max()
        worst, worst_np = max(worst, err / bound), max(worst_np, err_np / bound)
        assert err <= bound, (trial, err, bound)
        assert np.allclose(cov, s2 * np.linalg.inv(info), rtol=1e-6 * max(1.0, k / 1e4), atol=0)
    print("largest error / bound: scl_loop_covariance", worst, "numpy.linalg.inv", worst_np)
    assert worst_np <= 1.0
    junk = np.diag([4.0, 1, 1, 1, 1, 2]); junk[3, 0] = 99.0                     # only the upper triangle is read
    assert np.allclose(ScanContextEngine.loop_covariance(junk, 2.0), np.diag([0.5, 2, 2, 2, 2, 1]), rtol=1e-15, atol=0)


def test_loop_covariance_answers_its_errors():
    lib = load_library(); _bind(lib)
    info = np.eye(6).reshape(36).copy(); cov = np.full(36, 7.0)
    dp = lambda a: a.ctypes.data_as(POINTER(c_double))
    assert lib.scl_loop_covariance(None, 1.0, dp(cov)) == INVALID_ARG and lib.scl_loop_covariance(dp(info), 1.0, None) == INVALID_ARG
    for s2 in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.scl_loop_covariance(dp(info), s2, dp(cov)) == INVALID_ARG
    for bad in (np.nan, np.inf):
        b = info.copy(); b[7] = bad
        assert lib.scl_loop_covariance(dp(b), 1.0, dp(cov)) == INVALID_ARG
    rank5 = np.diag([1.0, 1, 1, 1, 1, 0]).reshape(36)                          # a corridor: nothing constrains the last axis
    assert lib.scl_loop_covariance(dp(rank5), 1.0, dp(cov)) == INVALID_ARG
    J = np.random.RandomState(2).standard_normal((5, 6))
    jtj = np.ascontiguousarray((J.T @ J).reshape(36))                         # rank 5 up to rounding: the last pivot is noise
    assert lib.scl_loop_covariance(dp(jtj), 1.0, dp(cov)) == INVALID_ARG
    neg = np.diag([1.0, 1, -1, 1, 1, 1]).reshape(36).copy()
    assert lib.scl_loop_covariance(dp(neg), 1.0, dp(cov)) == INVALID_ARG
    assert (cov == 7.0).all()
    with pytest.raises(SclError):
        ScanContextEngine.loop_covariance(rank5, 1.0)
    assert lib.scl_loop_covariance(dp(jtj + 1e-6 * np.eye(6).reshape(36)), 1.0, dp(cov)) == 0     # regularised first: accepted


def test_adjacency_words_round_trip():
    rs = np.random.RandomState(1)
    for n in (0, 1, 63, 64, 65, 130):
        a = rs.rand(n, n) < 0.4
        w = pcm_bool_to_words(a)
        assert w.shape == (n, (n + 63) // 64) and np.array_equal(pcm_words_to_bool(w, n), a)
    a = np.zeros((70, 70), bool); a[3, 66] = True
    assert int(pcm_bool_to_words(a)[3, 1]) == 1 << 2
