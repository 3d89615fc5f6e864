"""The C ABI of the condensed direct step (include/scl_engine.h "POSE-GRAPH SOLVE, CONDENSED DIRECT STEP") without a GPU: the calls
declared and exported, the binding's argument types those of the declarations, a NULL engine refused with nothing written,
scl_pgo_count_junctions on the named graphs, and the host-only plan (scl_slam_amd/csrc/pgo_condense_plan.hpp) through
tests/cpp/pgo_condense_plan_check -- a program of its own under ASan + UBSan, built by the test -- against the rule and the level order
of tests/pgo_condensed_cases.py.  (The technique of tests/test_pgo_abi.py.)"""
import os
import re
import subprocess
from ctypes import POINTER, byref, c_double, c_int, c_void_p

import numpy as np
import pytest

import pgo_cases as pg
import pgo_condensed_cases as cc
from scl_slam_amd import PgoParams, PgoResult, ScanContextEngine, load_library
from scl_slam_amd.engine import _bind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("scl_pgo_count_junctions", "scl_pgo_solve_condensed", "scl_pgo_optimize_condensed")
INVALID_ARG = -1
C_TYPES = {"scl_engine *": c_void_p, "int": c_int, "double": c_double, "const int *": POINTER(c_int), "int *": POINTER(c_int),
           "double *": POINTER(c_double), "const double *": POINTER(c_double), "const scl_pgo_params *": POINTER(PgoParams),
           "scl_pgo_result *": POINTER(PgoResult)}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scl_engine.h")).read(), flags=re.S)


def _declaration(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", _header(), flags=re.S)
    assert m, f"{name} is not declared in scl_engine.h"
    return [re.match(r"(.*?)(\w+)$", " ".join(a.split())).group(1).strip() for a in m.group(1).split(",")]


def test_declared_exported_and_typed():
    lib = load_library(); _bind(lib)
    assert lib.scl_abi_version() >= 14
    for name in NAMES:
        fn = getattr(lib, name)
        want = [C_TYPES[t] for t in _declaration(name)]
        assert fn.restype is c_int and list(fn.argtypes) == want, (name, fn.argtypes, want)
    assert [len(_declaration(n)) for n in NAMES] == [9, 14, 17]
    assert re.search(r"#define\s+SCL_PGO_MAX_JUNCTIONS\s+1024\b", _header()) and re.search(r"SCL_ERR_NUMERIC\s*=\s*-7\b", _header())
    assert lib.scl_status_string(-7) == b"a factorisation failed"


def test_a_null_engine_is_refused_and_nothing_is_written():
    lib = load_library(); _bind(lib)
    g = pg.lin_case("two")
    dp = lambda a: a.ctypes.data_as(POINTER(c_double)); ip = lambda a: a.ctypes.data_as(POINTER(c_int))
    common = (None, dp(g.poses), 2, ip(g.f_i), ip(g.f_j), dp(g.f_z), dp(g.f_cov), 2, ip(g.p_idx), dp(g.p_z), dp(g.p_cov), 1)
    delta = np.full(12, 7.0); out = np.full(14, 7.0); chi2 = np.full(3, 7.0)
    res = PgoResult(); res.iterations = 7
    failed = c_int(7)
    assert lib.scl_pgo_solve_condensed(*common, 1e-5, dp(delta)) == INVALID_ARG
    assert lib.scl_pgo_optimize_condensed(*common, None, dp(out), byref(res), dp(chi2), byref(failed)) == INVALID_ARG
    ms = np.full(4, 7.0)
    assert lib.scl_pgo_condensed_last_timing(None, dp(ms)) == INVALID_ARG
    assert (res.iterations, failed.value) == (7, 7) and all((v == 7).all() for v in (delta, out, chi2, ms))


def test_count_junctions_on_the_named_graphs():
    for n in (3, 4):
        g, junctions, segments, _ = cc.hand_case(n)
        assert ScanContextEngine.pgo_count_junctions(n, g.f_i, g.f_j, g.p_idx) == (2, 1, n - 2)
    for name, want in cc.COUNTS.items():
        g = cc.step_case(name)
        got = ScanContextEngine.pgo_count_junctions(len(g.poses), g.f_i, g.f_j, g.p_idx)
        assert all(w is None or w == v for w, v in zip(want, got)), (name, got, want)
        J, segs = cc.classify(len(g.poses), g.f_i, g.f_j, g.p_idx)
        assert got == (len(J), len(segs), max([b - a + 1 for a, b in segs], default=0))
    g = cc.many_junctions()
    assert ScanContextEngine.pgo_count_junctions(len(g.poses), g.f_i, g.f_j, g.p_idx) == (cc.MAX_JUNCTIONS + 1, 0, 0)
    # errors: nothing written
    lib = load_library(); _bind(lib)
    ip = lambda a: np.ascontiguousarray(a, np.int32).ctypes.data_as(POINTER(c_int))
    a, b, c = c_int(7), c_int(7), c_int(7)
    for args in ((0, ip([0]), ip([1]), 0, ip([0]), 1), (3, ip([0, 1]), ip([1, 3]), 2, ip([0]), 1), (3, ip([0, -1]), ip([1, 2]), 2, ip([0]), 1),
                 (3, ip([0, 1]), ip([1, 2]), 2, ip([3]), 1), (3, None, ip([1, 2]), 2, ip([0]), 1), (3, ip([0, 1]), ip([1, 2]), 2, None, 1),
                 (3, ip([0, 1]), ip([1, 2]), -1, ip([0]), 1), (3, ip([0, 1]), ip([1, 2]), 2, ip([0]), -1)):
        assert lib.scl_pgo_count_junctions(*args, byref(a), byref(b), byref(c)) == INVALID_ARG
    assert (a.value, b.value, c.value) == (7, 7, 7)
    assert lib.scl_pgo_count_junctions(3, ip([0, 1]), ip([1, 2]), 2, ip([0]), 1, None, None, byref(c)) == 0 and c.value == 1


def _ask(graphs):
    exe = os.path.join(ROOT, "tests", "cpp", "pgo_condense_plan_check")
    # built here by the Makefile's rule (ASan + UBSan), so that a binary older than the header is never what answers
    r = subprocess.run(["make", "-C", ROOT, "tests/cpp/pgo_condense_plan_check"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and os.path.exists(exe), r.stdout + r.stderr
    text = "".join(f"{n} {len(fi)} {len(pi)}\n" + " ".join(f"{a} {b}" for a, b in zip(fi, fj)) + "\n" + " ".join(map(str, pi)) + "\n"
                   for n, fi, fj, pi in graphs)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    answers, cur = [], None
    for line in r.stdout.splitlines():
        if line.startswith("counts"):
            cur = []
        cur.append(line.split())
        if line == "end":
            answers.append(cur)
    return answers


def _expected(n, fi, fj, pi):
    """the lines of pgo_condense_plan_check by the checker's rule and level order"""
    J, segs = cc.classify(n, fi, fj, pi)
    jof = {p: j for j, p in enumerate(J)}
    levels, absorbs = {}, {}
    for s, (a, b) in enumerate(segs):
        for l, level in enumerate(cc.path_levels(b - a + 3)):
            out = levels.setdefault(l, []); ab = absorbs.setdefault(l, [])
            left, right, order = {}, {}, []
            for node, lf, r in level:
                out += [f"{node}:{s}", f"{lf}:{s}", f"{r}:{s}"]
                for surv in (lf, r):
                    if surv not in order:
                        order.append(surv)
                right[lf] = node; left[r] = node
            for surv in order:
                ab += [f"{surv}:{s}", f"{left[surv]}:{s}" if surv in left else "-1", f"{right[surv]}:{s}" if surv in right else "-1"]
    n_levels = len(levels)
    lines = [["counts", len(J), len(segs), max([b - a + 1 for a, b in segs], default=0), n_levels, sum(b - a + 3 for a, b in segs)],
             ["junctions"] + J, ["segments"] + [v for ab in segs for v in ab]]
    for l in range(n_levels):
        lines += [["level", l] + levels[l], ["absorb", l] + absorbs[l]]
    blocks = {}
    for j in range(len(J)):
        blocks[(j, j)] = [f"0:{J[j]}"]
    for k, (a, b) in enumerate(zip(fi, fj)):
        if a in jof and b in jof:
            ja, jb = jof[a], jof[b]
            blocks.setdefault((max(ja, jb), min(ja, jb)), []).append(f"1:{k}" if ja > jb else f"2:{k}")
    rhs = {}
    for s, (a, b) in enumerate(segs):
        ja, jb, last = jof[a - 1], jof[b + 1], b - a + 2
        blocks[(ja, ja)].append(f"3:0:{s}"); blocks[(jb, jb)].append(f"3:{last}:{s}")
        blocks.setdefault((jb, ja), []).append(f"4:0:{s}")
        rhs.setdefault(ja, []).append(f"0:{s}"); rhs.setdefault(jb, []).append(f"{last}:{s}")
    lines += [["block", r, c] + blocks[(r, c)] for r, c in sorted(blocks)]
    lines += [["rhs", j] + rhs[j] for j in sorted(rhs)]
    return [[str(v) for v in line] for line in lines] + [["end"]]


def test_the_plan_header_against_the_checkers_rule_and_level_order():
    rs = np.random.RandomState(5)
    graphs = []
    for n in (3, 4):
        g = cc.hand_case(n)[0]
        graphs.append((n, g.f_i.tolist(), g.f_j.tolist(), g.p_idx.tolist()))
    for name in ("one", "two_poses", "reversed", "duplicate", "mid_prior", "adjacent", "two_robots", "segment7", "segment64", "segment65", "segment257"):
        g = cc.step_case(name)
        graphs.append((len(g.poses), g.f_i.tolist(), g.f_j.tolist(), g.p_idx.tolist()))
    graphs.append((5, [0, 1, 3, 2], [1, 2, 4, 4], [0]))                          # an odometry step that skips an index: 2 - 4
    graphs.append((6, [0, 1, 2, 3, 4, 1], [1, 2, 3, 4, 5, 3], [0, 5]))
    for _ in range(40):                                                         # chains with random loops, reversed steps, priors and gaps
        n = int(rs.randint(2, 60))
        fi, fj = [], []
        for k in range(n - 1):
            if rs.rand() < 0.05:
                continue                                                        # a gap: two blocks
            a, b = (k, k + 1) if rs.rand() < 0.7 else (k + 1, k)
            fi.append(a); fj.append(b)
            if rs.rand() < 0.05:
                fi.append(a); fj.append(b)                                      # a duplicate
        for _ in range(int(rs.randint(0, 4))):
            a, b = rs.randint(0, n, 2)
            if a != b:
                fi.append(int(a)); fj.append(int(b))
        graphs.append((n, fi, fj, rs.randint(0, n, int(rs.randint(0, 3))).tolist()))
    answers = _ask(graphs)
    assert len(answers) == len(graphs)
    for (n, fi, fj, pi), got in zip(graphs, answers):
        want = _expected(n, fi, fj, pi)
        got = [line for line in got if line[0] != "couplings"]                  # checked by the program itself against f_i, f_j
        assert got == want, (n, fi, fj, pi, [(a, b) for a, b in zip(got, want) if a != b][:3])
