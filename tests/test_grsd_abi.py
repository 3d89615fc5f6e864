"""The GRSD plugin's C ABI (include/scl_grsd.h) without a GPU: a plain C99 header, every declared symbol exported, the reference's
defaults, and a loud error where no device is present."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scl_grsd.h")


def declared_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(scl_grsd_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_the_plugin_calls():
    names = declared_symbols()
    for n in ["default_config", "create", "destroy", "last_error", "make", "make_and_save", "make_and_save_many", "save_from_wire",
              "get_size", "get_size_of", "get_index", "local_to_global", "get_signature", "detect_intra", "detect_inter", "stats",
              "normals", "voxels", "transitions"]:
        assert f"scl_grsd_{n}" in names


def test_library_exports_every_declared_symbol():
    from scl_slam_amd import load_library, LIB_PATH
    assert os.path.exists(LIB_PATH), "build first: make (or __graft_entry__.build())"
    lib = load_library()
    missing = [n for n in declared_symbols() if not hasattr(lib, n)]
    assert not missing, f"declared in scl_grsd.h but not exported: {missing}"


def test_header_is_plain_c99(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    src = tmp_path / "cabi.c"
    src.write_text('#include "scl_grsd.h"\nint main(void) { scl_grsd_config c; return scl_grsd_default_config(&c) == SCL_OK ? 0 : 1; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_defaults_are_the_references():
    from scl_slam_amd.grsd import DIM, MAX_GROUP, default_config
    c = default_config()
    # D.h:186-189 (neRadius, numExcludeRecent, treeMakingPeriod), D.h:155 (the loop threshold), setRadiusSearch(2.0) (D.h:89)
    assert (c.ne_radius, c.num_exclude_recent, c.tree_making_period) == (0.5, 30, 10)
    assert c.dist_thres == 160.0 and c.grsd_radius == 2.0
    assert (c.inter_mode, c.robot_num, c.this_id, c.device) == (0, 1, 0, 0)
    assert (DIM, MAX_GROUP) == (21, 16)


def test_bad_config_is_rejected_before_the_device_is_touched():
    from scl_slam_amd.grsd import _lib, default_config
    lib = _lib()
    for field, value in [("ne_radius", 0.0), ("ne_radius", 1.5), ("ne_radius", float("nan")), ("grsd_radius", 0.0),
                         ("grsd_radius", -2.0), ("tree_making_period", 0), ("inter_mode", 2), ("this_id", 1)]:
        c = default_config(); setattr(c, field, value)
        h = ctypes.c_void_p()
        assert lib.scl_grsd_create(ctypes.byref(c), ctypes.byref(h)) == -1, field      # SCL_ERR_INVALID_ARG
        assert not h.value


def test_no_device_is_a_loud_error_not_a_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from scl_slam_amd import GrsdEngine, GrsdError
    with pytest.raises(GrsdError) as ei:
        GrsdEngine()
    assert ei.value.status == -2        # SCL_ERR_NO_DEVICE
