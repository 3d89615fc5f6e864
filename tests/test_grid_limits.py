"""The grid contract without a GPU: which num_ring x num_sector scl_create takes (scl_slam_amd/csrc/grid_limits.hpp).

tests/cpp/grid_limits_check.cpp, built by `make` under ASan + UBSan as a program of its own, sweeps all 256 x 1024 grids against the
kernels' constraints restated.  The Python tests create an engine on each refused and each accepted literal: scl_create checks the
configuration before it looks for a device, so a refused grid answers SCL_ERR_UNSUPPORTED here, and an accepted one anything else
(SCL_ERR_NO_DEVICE without a GPU, an engine with one).  No kernel is launched on a refused grid."""
import os
import subprocess

import pytest

from grid_cases import GRIDS, REFUSED_GRIDS, RMAX_224

ROOT = os.path.dirname(os.path.abspath(__file__))
SCL_ERR_INVALID_ARG, SCL_ERR_UNSUPPORTED = -1, -6


def test_the_predicate_over_all_grids_against_the_kernels_constraints():
    exe = os.path.join(ROOT, "cpp", "grid_limits_check")
    assert os.path.exists(exe), "build it with `make`"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "grid_limits_check: ok" in r.stdout, r.stdout + r.stderr


def _create_status(R, S):
    from scl_slam_amd import ScanContextEngine, SclError
    try:
        eng = ScanContextEngine(num_ring=R, num_sector=S, initial_capacity=4)
    except SclError as err:
        return err.status
    eng.close()
    return 0


def test_the_refused_literals_are_the_issue_s():
    assert set(REFUSED_GRIDS) == {(1, 1), (16, 225), (20, 1024), (256, 224), (RMAX_224 + 1, 224)} and RMAX_224 == 174


@pytest.mark.parametrize("R,S", REFUSED_GRIDS, ids=[f"{r}x{s}" for r, s in REFUSED_GRIDS])
def test_a_refused_grid_is_never_created(R, S):
    assert _create_status(R, S) == SCL_ERR_UNSUPPORTED


@pytest.mark.parametrize("R,S", GRIDS, ids=[f"{r}x{s}" for r, s in GRIDS])
def test_an_accepted_grid_is_not_refused(R, S):
    assert _create_status(R, S) not in (SCL_ERR_UNSUPPORTED, SCL_ERR_INVALID_ARG)


@pytest.mark.parametrize("R,S", [(0, 60), (257, 60), (20, 0), (20, 1025)])
def test_what_create_always_refused_keeps_its_status(R, S):
    assert _create_status(R, S) == SCL_ERR_INVALID_ARG
