"""The C ABI of the guessed batched verification (include/scl_engine.h "THE BATCHED VERIFICATION WITH INITIAL GUESSES") and of
scl_loop_guess_from_shift without a GPU: the three calls declared and exported, the binding's argument types those of the
declarations, the ABI version moved to 7, a NULL engine refused with nothing written.  (The technique of
tests/test_verification_batch_abi.py; an array parameter `const float p[6]` is the pointer it decays to.)"""
import ctypes
import inspect
import os
import re
from ctypes import POINTER, c_double, c_float, c_int, c_uint64, c_void_p

from scl_slam_amd import load_library
from scl_slam_amd.engine import ScanContextEngine, _bind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("scl_geometric_verification_batch_guess", "scl_geometric_verification_batch_from_store_guess", "scl_loop_guess_from_shift")
INVALID_ARG = -1
C_TYPES = {"scl_engine *": c_void_p, "const void *": c_void_p, "const void *const *": POINTER(c_void_p), "int": c_int, "float": c_float,
           "double": c_double, "uint64_t": c_uint64, "const int *": POINTER(c_int), "int *": POINTER(c_int),
           "const float *": POINTER(c_float), "float *": POINTER(c_float)}


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
    assert lib.scl_abi_version() >= 7
    for name in NAMES:
        fn = getattr(lib, name)
        want = [C_TYPES[t] for t in _declaration(name)]
        assert fn.restype is c_int and list(fn.argtypes) == want, (name, fn.argtypes, want)
    assert len(_declaration(NAMES[0])) == 17 and len(_declaration(NAMES[1])) == 25 and len(_declaration(NAMES[2])) == 5


def test_a_null_engine_is_refused_and_nothing_is_written():
    lib = load_library(); _bind(lib)
    T = (c_float * 16)(*([7.0] * 16)); Tf = (c_float * 16)(*([7.0] * 16))
    ok = c_int(7); ns = c_int(7); nt = c_int(7); nc = c_int(7); ni = c_int(7)
    cloud = (c_float * 8)(); ptrs = (c_void_p * 1)(ctypes.addressof(cloud)); counts = (c_int * 1)(1); keys = (c_int * 1)(0)
    poses = (c_float * 16)(); G = (c_float * 16)(*[1.0 if k % 5 == 0 else 0.0 for k in range(16)])
    rc = lib.scl_geometric_verification_batch_guess(None, ctypes.addressof(cloud), 1, ptrs, counts, 1, 32, G, 10, 0.25, 0.45, 1,
                                                    T, Tf, ctypes.byref(ok), ctypes.byref(nc), ctypes.byref(ni))
    assert rc == INVALID_ARG
    rc = lib.scl_geometric_verification_batch_from_store_guess(None, ctypes.addressof(cloud), 1, 32, 0.2, 0, 1, keys, 0, poses, 0.3, G, 300, 1000,
                                                               10, 0.25, 0.45, 1, T, Tf, ctypes.byref(ok), ctypes.byref(ns), ctypes.byref(nt),
                                                               ctypes.byref(nc), ctypes.byref(ni))
    assert rc == INVALID_ARG
    assert list(T) == [7.0] * 16 and list(Tf) == [7.0] * 16 and (ok.value, ns.value, nt.value, nc.value, ni.value) == (7, 7, 7, 7, 7)


def test_the_binding_follows_the_unguessed_forms():
    """the Python methods: the unguessed methods' parameters and defaults with `guesses` behind the candidates"""
    def spec(f):
        p = inspect.signature(f).parameters
        return [(n, v.default) for n, v in p.items() if n != "self"]
    E = ScanContextEngine
    plain, guessed = spec(E.geometric_verification_batch), spec(E.geometric_verification_batch_guess)
    assert guessed == plain[:2] + [("guesses", inspect.Parameter.empty)] + plain[2:]
    plain, guessed = spec(E.geometric_verification_batch_from_store), spec(E.geometric_verification_batch_from_store_guess)
    assert guessed == plain[:7] + [("guesses", inspect.Parameter.empty)] + plain[7:]
    assert [n for n, _ in spec(E.loop_guess_from_shift)] == ["shift", "num_sector", "pose_cur", "pose_pre"]
