"""The batch forms of the LiDAR-Iris C ABI (include/scl_iris.h "THE BATCH FORMS") without a GPU: the five declarations after
preprocessing the header as C99, their export from the built library, their binding in scl_slam_amd/iris.py, and the NULL-handle
answer."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")

CLOUDS = "const void *const *clouds, const int *n_points, int stride_bytes, const int8_t *robots, const int *indexs, int count"
SIGNATURES = {
    "scl_iris_make_and_save_many": f"int scl_iris_make_and_save_many(scl_iris *h, {CLOUDS}, float *out_values);",
    "scl_iris_save_from_wire_many": "int scl_iris_save_from_wire_many(scl_iris *h, const float *values, const int8_t *robots, const int *indexs, int count);",
    "scl_iris_detect_intra_many": "int scl_iris_detect_intra_many(scl_iris *h, const int *curs, int count, int *loop_ids, float *biases, float *dists);",
    "scl_iris_detect_inter_many": "int scl_iris_detect_inter_many(scl_iris *h, const int *curs, int count, int *loop_ids, float *biases, float *dists);",
    "scl_iris_make_save_and_detect": f"int scl_iris_make_save_and_detect(scl_iris *h, {CLOUDS}, int *loop_ids, float *biases, float *dists, float *out_values);",
}


def _squeeze(text):
    """one spelling of a declaration: no line breaks, single blanks, none around punctuation"""
    text = re.sub(r"\s+", " ", text)
    return re.sub(r"\s*([(),;*])\s*", r"\1", text).strip()


def _preprocessed():
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    r = subprocess.run(["gcc", "-std=c99", "-E", "-P", "-I", INCLUDE, os.path.join(INCLUDE, "scl_iris.h")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_header_declares_the_batch_forms_as_c99(tmp_path):
    text = _squeeze(_preprocessed())
    for name, sig in SIGNATURES.items():
        assert _squeeze(sig) in text, name
    # the group sizes are plain macros, and the whole header with them compiles as pedantic C99
    src = tmp_path / "cabi.c"
    src.write_text('#include "scl_iris.h"\nint main(void) { return SCL_IRIS_MAX_GROUP == 16 && SCL_IRIS_DETECT_GROUP == 16 && '
                   'scl_iris_detect_intra_many(0, 0, 0, 0, 0, 0) == SCL_ERR_INVALID_ARG ? 0 : 1; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INCLUDE, "-fsyntax-only", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_library_exports_the_batch_forms():
    from scl_slam_amd import load_library, LIB_PATH
    assert os.path.exists(LIB_PATH), "build first: make (or __graft_entry__.build())"
    lib = load_library()
    missing = [n for n in SIGNATURES if not hasattr(lib, n)]
    assert not missing, f"declared in scl_iris.h but not exported: {missing}"


def test_python_binds_the_batch_forms():
    from scl_slam_amd import iris
    lib = iris._lib()
    for name in SIGNATURES:
        res, args = iris._SIG[name]
        fn = getattr(lib, name)
        assert fn.restype is res is ctypes.c_int and list(fn.argtypes) == args, name
    n_args = {name: sig.count(",") + 1 for name, sig in SIGNATURES.items()}
    assert {name: len(iris._SIG[name][1]) for name in SIGNATURES} == n_args
    for method in ("make_and_save_many", "save_from_wire_many", "detect_intra_many", "detect_inter_many", "make_save_and_detect"):
        assert callable(getattr(iris.IrisEngine, method)), method
    assert (iris.MAX_GROUP, iris.DETECT_GROUP) == (16, 16)


def test_null_handle_is_an_invalid_argument():
    """no handle, no device touched: SCL_ERR_INVALID_ARG (-1) from every batch call, whatever else is passed"""
    from scl_slam_amd import iris
    lib = iris._lib()
    one = (ctypes.c_int * 1)(0)
    f = (ctypes.c_float * 1)(0.0)
    r8 = (ctypes.c_int8 * 1)(0)
    ptrs = (ctypes.c_void_p * 1)(None)
    ip, fp, i8p = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int8)
    as_ip, as_fp = ctypes.cast(one, ip), ctypes.cast(f, fp)
    assert lib.scl_iris_make_and_save_many(None, ptrs, as_ip, 16, ctypes.cast(r8, i8p), as_ip, 0, None) == -1
    assert lib.scl_iris_save_from_wire_many(None, as_fp, ctypes.cast(r8, i8p), as_ip, 0) == -1
    assert lib.scl_iris_detect_intra_many(None, as_ip, 1, as_ip, as_fp, None) == -1
    assert lib.scl_iris_detect_inter_many(None, as_ip, 0, as_ip, as_fp, None) == -1
    assert lib.scl_iris_make_save_and_detect(None, ptrs, as_ip, 16, ctypes.cast(r8, i8p), as_ip, 0, as_ip, as_fp, None, None) == -1
    assert one[0] == 0 and f[0] == 0.0
