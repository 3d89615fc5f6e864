"""The C ABI of the vector plugins (include/scl_m2dp.h, scl_fpfh.h, scl_grsd.h and the two declaring macros of scl_plugin_batch.h)
without a GPU: every declared function is exported by the library, and the calls answer a null handle, a null argument and a bad
config as the headers say -- with SCL_ERR_INVALID_ARG before a device is looked for."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
PLUGINS = ("scl_m2dp", "scl_fpfh", "scl_grsd")
SCL_OK, SCL_ERR_INVALID_ARG = 0, -1                     # scl_engine.h: scl_status
# what every vector plugin declares beside its own hooks and stats (scl_X.h), the batch forms and the candidate lists included
COMMON = ("default_config", "create", "destroy", "last_error", "make", "make_and_save", "make_and_save_many", "save_from_wire",
          "save_from_wire_many", "get_size", "get_size_of", "get_index", "local_to_global", "get_signature", "detect_intra",
          "detect_inter", "detect_intra_many", "detect_inter_many", "detect_intra_topk", "detect_inter_topk", "make_save_and_detect")


def _text(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, name)).read(), flags=re.S)


def _macro_suffixes():
    """{macro name: the suffixes of the functions it declares} from the #define bodies of scl_plugin_batch.h"""
    out = {}
    for name, body in re.findall(r"#define\s+(SCL_PLUGIN_\w+_API)\(X\)((?:.*\\\n)*.*)", _text("scl_plugin_batch.h")):
        out[name] = re.findall(r"X##_([a-z0-9_]+)\s*\(", body)
    return out


def declared(prefix):
    text = _text(prefix + ".h")
    names = set(re.findall(r"\b(%s_[a-z0-9_]+)\s*\(" % prefix, text))
    for macro, suffixes in _macro_suffixes().items():
        if re.search(r"\b%s\(%s\)" % (macro, prefix), text):
            names.update(f"{prefix}_{s}" for s in suffixes)
    return sorted(names)


@pytest.fixture(scope="module")
def lib():
    from scl_slam_amd import LIB_PATH
    assert os.path.exists(LIB_PATH), "build first: make (or __graft_entry__.build())"
    return ctypes.CDLL(LIB_PATH)                        # its own function objects: the prototypes set here stay here


def _configs():
    from scl_slam_amd.fpfh import FpfhConfig
    from scl_slam_amd.grsd import GrsdConfig
    from scl_slam_amd.m2dp import M2dpConfig
    return {"scl_m2dp": M2dpConfig, "scl_fpfh": FpfhConfig, "scl_grsd": GrsdConfig}


def test_the_macros_declare_the_batch_forms_and_the_candidate_lists():
    m = _macro_suffixes()
    assert sorted(m["SCL_PLUGIN_BATCH_API"]) == ["detect_inter_many", "detect_intra_many", "make_save_and_detect", "save_from_wire_many"]
    assert sorted(m["SCL_PLUGIN_TOPK_API"]) == ["detect_inter_topk", "detect_intra_topk"]


@pytest.mark.parametrize("prefix", PLUGINS)
def test_every_declared_function_is_exported(lib, prefix):
    names = declared(prefix)
    assert not [n for n in COMMON if f"{prefix}_{n}" not in names], "the header lost a common entry point"
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, f"declared in {prefix}.h but not exported: {missing}"


@pytest.mark.parametrize("prefix", PLUGINS)
def test_null_arguments_answer_as_the_headers_say(lib, prefix):
    cfg_t = _configs()[prefix]
    f = lambda name: getattr(lib, f"{prefix}_{name}")
    assert f("default_config")(None) == SCL_ERR_INVALID_ARG
    h = ctypes.c_void_p()
    assert f("create")(None, ctypes.byref(h)) == SCL_ERR_INVALID_ARG and not h.value
    cfg = cfg_t()
    assert f("default_config")(ctypes.byref(cfg)) == SCL_OK
    assert f("create")(ctypes.byref(cfg), None) == SCL_ERR_INVALID_ARG
    assert f("destroy")(None) == SCL_OK
    f("last_error").restype = ctypes.c_char_p
    assert f("last_error")(None) == b"null handle"
    assert f("get_size")(None) == SCL_ERR_INVALID_ARG


@pytest.mark.parametrize("prefix", PLUGINS)
def test_a_bad_config_is_an_invalid_argument_not_a_device_error(lib, prefix):
    """robot_num = 0 (and the other shared fields out of range) is refused whether or not a device is present"""
    cfg_t = _configs()[prefix]
    for field, value in [("robot_num", 0), ("robot_num", 128), ("this_id", -1), ("this_id", 1), ("num_exclude_recent", -1),
                         ("dist_thres", float("nan"))]:
        cfg = cfg_t()
        assert getattr(lib, prefix + "_default_config")(ctypes.byref(cfg)) == SCL_OK
        setattr(cfg, field, value)
        h = ctypes.c_void_p(1)
        assert getattr(lib, prefix + "_create")(ctypes.byref(cfg), ctypes.byref(h)) == SCL_ERR_INVALID_ARG, field
        assert not h.value, field                       # *out is cleared before the config is judged
