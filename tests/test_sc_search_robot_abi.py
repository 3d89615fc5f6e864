"""The per-robot ranked searches of the Scan Context engine (include/scl_engine.h, THE RANKED SEARCH PER ROBOT) without a GPU: the two
declarations after preprocessing the header as C99, the macro, their export from the built library, their binding in
scl_slam_amd/engine.py with the two methods, the ABI version and the NULL-engine answer."""
import ctypes
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")

OUT = "int *cand_ids, int *cand_shifts, double *cand_dists, int *n_found"
SIGNATURES = {
    "scl_sc_search_intra": f"int scl_sc_search_intra(scl_engine *e, const int *curs, int count, int k, {OUT});",
    "scl_sc_search_inter": f"int scl_sc_search_inter(scl_engine *e, const int *curs, int count, int robot_pre, int k, {OUT});",
}


def _squeeze(text):
    """one spelling of a declaration: no line breaks, single blanks, none around punctuation"""
    text = re.sub(r"\s+", " ", text)
    return re.sub(r"\s*([(),;*])\s*", r"\1", text).strip()


def test_header_declares_the_searches_as_c99(tmp_path):
    r = subprocess.run(["gcc", "-std=c99", "-E", "-P", "-I", INCLUDE, os.path.join(INCLUDE, "scl_engine.h")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = _squeeze(r.stdout)
    for name, sig in SIGNATURES.items():
        assert _squeeze(sig) in text, name
    src = tmp_path / "cabi.c"
    src.write_text('#include "scl_engine.h"\n'
                   'int main(void) { return SCL_SC_ANY_OTHER_ROBOT == -1 && -SCL_SC_ANY_OTHER_ROBOT == 1 ? 0 : 1; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INCLUDE, "-fsyntax-only", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_macro_is_minus_one_in_parentheses():
    m = re.search(r"^#define\s+SCL_SC_ANY_OTHER_ROBOT\s+(\S+)\s*$", open(os.path.join(INCLUDE, "scl_engine.h")).read(), flags=re.M)
    assert m and m.group(1) == "(-1)", m


def test_library_exports_the_searches_and_the_version():
    from scl_slam_amd import load_library, LIB_PATH
    assert os.path.exists(LIB_PATH), "build first: make (or __graft_entry__.build())"
    lib = load_library()
    missing = [n for n in SIGNATURES if not hasattr(lib, n)]
    assert not missing, f"declared in scl_engine.h but not exported: {missing}"
    assert lib.scl_abi_version() >= 8


def test_python_binds_the_searches():
    from scl_slam_amd import load_library
    from scl_slam_amd import engine
    lib = load_library(); engine._bind(lib)
    for name, sig in SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == sig.count(",") + 1, name
    intra = inspect.signature(engine.ScanContextEngine.sc_search_intra)
    inter = inspect.signature(engine.ScanContextEngine.sc_search_inter)
    assert list(intra.parameters) == ["self", "curs", "k", "out"] and intra.parameters["out"].default is None
    assert list(inter.parameters) == ["self", "curs", "k", "robot_pre", "out"]
    assert inter.parameters["robot_pre"].default == -1 and inter.parameters["out"].default is None


def test_null_engine_is_an_invalid_argument():
    """no engine, no device touched: SCL_ERR_INVALID_ARG (-1), whatever else is passed; nothing written"""
    from scl_slam_amd import load_library
    from scl_slam_amd import engine
    lib = load_library(); engine._bind(lib)
    ip, dp = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
    q = (ctypes.c_int * 2)(0, 1); ids = (ctypes.c_int * 10)(*([-7] * 10)); sh = (ctypes.c_int * 10)(*([-7] * 10))
    d = (ctypes.c_double * 10)(*([-7.0] * 10)); nf = (ctypes.c_int * 2)(-7, -7)
    as_ip = lambda a: ctypes.cast(a, ip)
    assert lib.scl_sc_search_intra(None, as_ip(q), 2, 5, as_ip(ids), as_ip(sh), ctypes.cast(d, dp), as_ip(nf)) == -1
    for robot_pre in (-1, 0, 127, 128, -2):
        assert lib.scl_sc_search_inter(None, as_ip(q), 2, robot_pre, 5, as_ip(ids), as_ip(sh), ctypes.cast(d, dp), as_ip(nf)) == -1
    assert lib.scl_sc_search_intra(None, None, 0, 5, None, None, None, None) == -1
    assert lib.scl_sc_search_inter(None, None, 0, -1, 5, None, None, None, None) == -1
    assert list(ids) == [-7] * 10 and list(sh) == [-7] * 10 and list(d) == [-7.0] * 10 and list(nf) == [-7, -7]
