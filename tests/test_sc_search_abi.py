"""The ranked search of the Scan Context engine (include/scl_engine.h, THE RANKED SEARCH) without a GPU: the two declarations after
preprocessing the header as C99, their export from the built library, their binding in scl_slam_amd/engine.py, the NULL-engine
answer and the list length's macro."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")

OUT = "int *cand_ids, int *cand_shifts, double *cand_dists, int *n_found"
SIGNATURES = {
    "scl_sc_search_range": f"int scl_sc_search_range(scl_engine *e, const int *queries, const int *lo, const int *hi, int n_queries, int k, {OUT});",
    "scl_sc_search": f"int scl_sc_search(scl_engine *e, const int *curs, int count, int k, {OUT});",
}


def _squeeze(text):
    """one spelling of a declaration: no line breaks, single blanks, none around punctuation"""
    text = re.sub(r"\s+", " ", text)
    return re.sub(r"\s*([(),;*])\s*", r"\1", text).strip()


def _macro(header, name):
    m = re.search(rf"^#define\s+{name}\s+(\d+)", open(os.path.join(INCLUDE, header)).read(), flags=re.M)
    assert m, f"{name} not defined in {header}"
    return int(m.group(1))


def test_header_declares_the_search_as_c99(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    r = subprocess.run(["gcc", "-std=c99", "-E", "-P", "-I", INCLUDE, os.path.join(INCLUDE, "scl_engine.h")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = _squeeze(r.stdout)
    for name, sig in SIGNATURES.items():
        assert _squeeze(sig) in text, name
    src = tmp_path / "cabi.c"
    src.write_text('#include "scl_engine.h"\n#include "scl_iris.h"\n#include "scl_plugin_batch.h"\n'
                   'int main(void) { return SCL_SC_SEARCH_MAX == SCL_PLUGIN_TOPK_MAX && SCL_SC_SEARCH_MAX == SCL_IRIS_SEARCH_MAX ? 0 : 1; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INCLUDE, "-fsyntax-only", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_longest_list_is_the_plugins():
    assert _macro("scl_engine.h", "SCL_SC_SEARCH_MAX") == _macro("scl_plugin_batch.h", "SCL_PLUGIN_TOPK_MAX") == _macro("scl_iris.h", "SCL_IRIS_SEARCH_MAX") == 32


def test_library_exports_the_search():
    from scl_slam_amd import load_library, LIB_PATH
    assert os.path.exists(LIB_PATH), "build first: make (or __graft_entry__.build())"
    lib = load_library()
    missing = [n for n in SIGNATURES if not hasattr(lib, n)]
    assert not missing, f"declared in scl_engine.h but not exported: {missing}"


def test_python_binds_the_search():
    from scl_slam_amd import load_library
    from scl_slam_amd import engine
    lib = load_library(); engine._bind(lib)
    for name, sig in SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == sig.count(",") + 1, name
    for method in ("sc_search", "sc_search_range"):
        assert callable(getattr(engine.ScanContextEngine, method)), method


def test_null_engine_is_an_invalid_argument():
    """no engine, no device touched: SCL_ERR_INVALID_ARG (-1), whatever else is passed; nothing written"""
    from scl_slam_amd import load_library
    from scl_slam_amd import engine
    lib = load_library(); engine._bind(lib)
    ip, dp = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
    q = (ctypes.c_int * 2)(0, 1); ids = (ctypes.c_int * 10)(*([-7] * 10)); sh = (ctypes.c_int * 10)(*([-7] * 10))
    d = (ctypes.c_double * 10)(*([-7.0] * 10)); nf = (ctypes.c_int * 2)(-7, -7)
    as_ip = lambda a: ctypes.cast(a, ip)
    assert lib.scl_sc_search(None, as_ip(q), 2, 5, as_ip(ids), as_ip(sh), ctypes.cast(d, dp), as_ip(nf)) == -1
    assert lib.scl_sc_search_range(None, as_ip(q), as_ip(q), as_ip(q), 2, 5, as_ip(ids), as_ip(sh), ctypes.cast(d, dp), as_ip(nf)) == -1
    assert lib.scl_sc_search(None, None, 0, 5, None, None, None, None) == -1
    assert lib.scl_sc_search_range(None, None, None, None, 0, 5, None, None, None, None) == -1
    assert list(ids) == [-7] * 10 and list(sh) == [-7] * 10 and list(d) == [-7.0] * 10 and list(nf) == [-7, -7]
