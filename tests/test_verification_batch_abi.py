"""The C ABI of the batched geometric verification (include/scl_engine.h "THE BATCHED VERIFICATION") without a GPU: both calls
declared and exported, a NULL engine refused, the binding's argument types those of the declarations, the ABI version moved."""
import ctypes
import inspect
import os
import re
from ctypes import POINTER, c_double, c_float, c_int, c_uint64, c_void_p

from scl_slam_amd import load_library
from scl_slam_amd.engine import ScanContextEngine, _bind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("scl_geometric_verification_batch", "scl_geometric_verification_batch_from_store")
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
        t = re.match(r"(.*?)(\w+)$", a).group(1).strip()
        args.append(t)
    return args


def test_declared_exported_and_typed():
    lib = load_library(); _bind(lib)
    assert lib.scl_abi_version() >= 6
    for name in NAMES:
        fn = getattr(lib, name)
        want = [C_TYPES[t] for t in _declaration(name)]
        assert fn.restype is c_int and list(fn.argtypes) == want, (name, fn.argtypes, want)


def test_a_null_engine_is_refused_and_nothing_is_written():
    lib = load_library(); _bind(lib)
    T = (c_float * 16)(*([7.0] * 16)); ok = c_int(7); ns = c_int(7); nt = c_int(7); nc = c_int(7); ni = c_int(7)
    cloud = (c_float * 8)(); ptrs = (c_void_p * 1)(ctypes.addressof(cloud)); counts = (c_int * 1)(1); keys = (c_int * 1)(0)
    poses = (c_float * 16)()
    rc = lib.scl_geometric_verification_batch(None, ctypes.addressof(cloud), 1, ptrs, counts, 1, 32, 10, 0.25, 0.45, 1,
                                              T, ctypes.byref(ok), ctypes.byref(nc), ctypes.byref(ni))
    assert rc == INVALID_ARG
    rc = lib.scl_geometric_verification_batch_from_store(None, ctypes.addressof(cloud), 1, 32, 0.2, 0, 1, keys, 0, poses, 0.3, 300, 1000,
                                                         10, 0.25, 0.45, 1, T, ctypes.byref(ok), ctypes.byref(ns), ctypes.byref(nt),
                                                         ctypes.byref(nc), ctypes.byref(ni))
    assert rc == INVALID_ARG
    assert list(T) == [7.0] * 16 and (ok.value, ns.value, nt.value, nc.value, ni.value) == (7, 7, 7, 7, 7)


def test_the_binding_follows_the_single_forms():
    """defaults and argument order of the Python methods: those of geometric_verification / geometric_verification_from_store, with a
    list of targets / of keys in place of one"""
    def spec(f):
        p = inspect.signature(f).parameters
        return [(n, v.default) for n, v in p.items() if n != "self"]
    one, many = spec(ScanContextEngine.geometric_verification), spec(ScanContextEngine.geometric_verification_batch)
    assert [n for n, _ in many] == ["src", "tgts"] + [n for n, _ in one[2:]] and many[2:] == one[2:]
    one, many = spec(ScanContextEngine.geometric_verification_from_store), spec(ScanContextEngine.geometric_verification_batch_from_store)
    assert [n.replace("keys_pre", "key_pre") for n, _ in many] == [n for n, _ in one] and [d for _, d in many] == [d for _, d in one]
