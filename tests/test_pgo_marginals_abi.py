"""The C ABI of the many-column solve and the marginals (include/scl_engine.h "POSE-GRAPH SOLVE, MANY RIGHT-HAND SIDES AND MARGINAL
COVARIANCES") without a GPU: the two calls and three macros declared, exported and bound with the declarations' argument types, a NULL
engine refused with nothing written, and the host-only plan (scl_slam_amd/csrc/pgo_marginal_plan.hpp: column groups, query selection)
through tests/cpp/pgo_marginal_plan_check -- a program of its own under ASan + UBSan, built by the test -- against the rule restated
here.  (The technique of tests/test_pgo_condensed_abi.py.)"""
import os
import re
import subprocess
from ctypes import POINTER, c_double, c_int, c_void_p

import numpy as np

import pgo_cases as pg
from scl_slam_amd import ScanContextEngine, load_library
from scl_slam_amd.engine import _bind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("scl_pgo_solve_condensed_many", "scl_pgo_marginals")
INVALID_ARG = -1
C_TYPES = {"scl_engine *": c_void_p, "int": c_int, "double": c_double, "const int *": POINTER(c_int), "double *": POINTER(c_double),
           "const double *": POINTER(c_double)}
BUDGET, MIN_GROUP, TILE, MAX_COLUMNS, NODE_DOUBLES = 256 << 20, 6, 16, 1536, 18


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scl_engine.h")).read(), flags=re.S)


def _declaration(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", _header(), flags=re.S)
    assert m, f"{name} is not declared in scl_engine.h"
    return [re.match(r"(.*?)(\w+)$", " ".join(a.split())).group(1).strip() for a in m.group(1).split(",")]


def test_declared_exported_and_typed():
    lib = load_library(); _bind(lib)
    assert lib.scl_abi_version() >= 15
    for name in NAMES:
        fn = getattr(lib, name)
        want = [C_TYPES[t] for t in _declaration(name)]
        assert fn.restype is c_int and list(fn.argtypes) == want, (name, fn.argtypes, want)
    assert [len(_declaration(n)) for n in NAMES] == [16, 17]
    h = _header()
    assert re.search(r"#define\s+SCL_PGO_MAX_RHS\s+1536\b", h) and re.search(r"#define\s+SCL_PGO_MAX_MARGINAL_POSES\s+256\b", h)
    assert re.search(r"#define\s+SCL_PGO_MAX_MARGINAL_QUERIES\s+4096\b", h)
    assert callable(ScanContextEngine.pgo_solve_condensed_many) and callable(ScanContextEngine.pgo_marginals)


def test_a_null_engine_is_refused_and_nothing_is_written():
    lib = load_library(); _bind(lib)
    g = pg.lin_case("two")
    dp = lambda a: a.ctypes.data_as(POINTER(c_double)); ip = lambda a: a.ctypes.data_as(POINTER(c_int))
    common = (None, dp(g.poses), 2, ip(g.f_i), ip(g.f_j), dp(g.f_z), dp(g.f_cov), 2, ip(g.p_idx), dp(g.p_z), dp(g.p_cov), 1)
    rhs = np.ones(24); x = np.full(24, 7.0); blocks = np.full(72, 7.0); rel = np.full(72, 7.0)
    q = np.int32([0, 1])
    assert lib.scl_pgo_solve_condensed_many(*common, 1e-5, dp(rhs), 2, dp(x)) == INVALID_ARG
    assert lib.scl_pgo_marginals(*common, ip(q), ip(q[::-1].copy()), 2, dp(blocks), dp(rel)) == INVALID_ARG
    assert all((v == 7).all() for v in (x, blocks, rel))


def _ask(text):
    exe = os.path.join(ROOT, "tests", "cpp", "pgo_marginal_plan_check")
    # built here by the Makefile's rule (ASan + UBSan), so that a binary older than the header is never what answers
    r = subprocess.run(["make", "-C", ROOT, "tests/cpp/pgo_marginal_plan_check"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and os.path.exists(exe), r.stdout + r.stderr
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    return [line.split() for line in r.stdout.splitlines()]


def group_columns(n_poses, n_nodes):
    """the contract's rule"""
    c = min(BUDGET // (8 * (6 * n_poses + NODE_DOUBLES * n_nodes)), MAX_COLUMNS)
    if c >= TILE:
        c -= c % TILE
    return max(c, MIN_GROUP)


def test_the_group_rule_of_the_plan_header():
    assert group_columns(100000, 100000) == 13              # one loop-free chain of 100 000 poses (the header's figure)
    assert group_columns(4097, 4097) == 336                 # chain4097: what tests/test_gpu_pgo_marginals.py reaches a second group with
    assert group_columns(257, 0) == MAX_COLUMNS and group_columns(1 << 20, 1 << 20) == MIN_GROUP
    asks = [(100000, 100000, 1536), (4097, 4097, 340), (4097, 4097, 336), (4097, 4097, 337), (257, 0, 1536), (1 << 20, 1 << 20, 7),
            (1 << 20, 0, 5), (12, 12, 1), (43700, 43700, 33), (1000, 1200, 96)]
    lines = _ask("".join(f"group {n} {nodes} {cols}\n" for n, nodes, cols in asks))
    assert len(lines) == len(asks)
    for (n, nodes, cols), line in zip(asks, lines):
        g = group_columns(n, nodes)
        want = [f"{f}:{min(g, cols - f)}" for f in range(0, cols, g)]
        assert line == ["group", str(g), str(len(want))] + want, (n, nodes, cols, line[:6])


def test_the_query_selection_of_the_plan_header():
    rs = np.random.RandomState(3)
    asks = [(5, [(0, 0)]), (5, [(4, 1), (1, 4), (1, 1), (4, 4), (2, 1)]), (300, [(k, k) for k in range(256)]),
            (300, [(k, 299 - k) for k in range(128)]), (300, [(k, k) for k in range(257)]), (5, [(0, 5)]), (5, [(-1, 0)]), (5, [(0, -1)]),
            (1000, [tuple(int(v) for v in rs.randint(0, 1000, 2)) for _ in range(100)]),
            (100000, [(int(rs.randint(0, 64)), 99999 - int(rs.randint(0, 64))) for _ in range(4096)])]
    lines = _ask("".join(f"select {n} {len(q)}\n" + " ".join(f"{a} {b}" for a, b in q) + "\n" for n, q in asks))
    assert len(lines) == len(asks)
    for (n, q), line in zip(asks, lines):
        poses = sorted({v for pair in q for v in pair})
        if any(v < 0 or v >= n for v in poses):
            assert line[:2] == ["refused", "a"] and "range" in line, line
        elif len(poses) > 256:
            assert line[:3] == ["refused", "more", "than"], line
        else:
            pos = {p: k for k, p in enumerate(poses)}
            assert line == ["select", str(len(poses))] + [str(p) for p in poses] + ["|"] + [f"{pos[a]}:{pos[b]}" for a, b in q], (n, line[:8])
