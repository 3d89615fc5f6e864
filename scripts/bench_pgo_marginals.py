#!/usr/bin/env python
"""The many-column solve (scl_pgo_solve_condensed_many) and the marginals (scl_pgo_marginals) on the graphs of DESIGN's condensed table:
one JSON line.

The graphs are tests/pgo_cases.py drifting_graph at 1 000, 4 097 and 10 000 poses with loops at 3 % of the poses and at 100 000 poses
with loops at 0.3 %.  Per graph, medians of --reps runs after a warm-up call: the marginals of 1, 16 and 256 poses (evenly spread over
the trajectory, blocks and rel of every pose with the next of the list) and the solve of 96 and 1 536 random columns -- the wall time of
the call (inputs and columns over PCIe) and, under scl_profile_enable(1), the four device times of scl_pgo_condensed_last_timing
(elimination, assembly of S, factorisation, the columns' forward eliminations + triangular solves + ways back).  Beside them two
baselines: scipy.sparse.linalg.splu on the same matrix (the checker's H at lambda = 1e-5 resp. 0) and the same columns on the CPU,
factorisation and solve apart, where the columns fit in --host-bytes; and the single step's own ms[3] (scl_pgo_solve_condensed: one
right-hand side through cond_tri_solve_kernel and the way back) times the column count -- what one-by-one solves would cost.  What is
not measured is null, with the reason beside it.

    python scripts/bench_pgo_marginals.py [--reps 3] [--host-bytes 2e9] [--only NAME ...]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse.linalg as spla

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pgo_cases as pg                                    # noqa: E402
from scl_slam_amd import ScanContextEngine                # noqa: E402

GRAPHS = {
    "drifting1000": lambda: pg.drifting_graph(1000),
    "drifting4097": lambda: pg.drifting_graph(4097),
    "drifting10000": lambda: pg.drifting_graph(10000),
    "drifting100000_0.3pct": lambda: pg.drifting_graph(100000, loop_frac=0.003),
}
LAM = 1e-5
MARGINAL_POSES = (1, 16, 256)
COLUMNS = (96, 1536)


def _timed(e, fn, reps):
    fn()                                                   # warm-up: allocations
    wall, parts = [], []
    e.profile_enable(1)
    for _ in range(reps):
        t = time.perf_counter(); fn(); wall.append((time.perf_counter() - t) * 1e3)
        parts.append(e.pgo_condensed_last_timing())
    e.profile_enable(0)
    p = np.median(np.array(parts), axis=0)
    return {"wall_ms": float(np.median(wall)), "elimination_ms": float(p[0]), "assembly_ms": float(p[1]), "factorisation_ms": float(p[2]),
            "columns_ms": float(p[3])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-bytes", type=float, default=2e9)
    ap.add_argument("--only", nargs="*", default=list(GRAPHS))
    a = ap.parse_args()
    e = ScanContextEngine(initial_capacity=16)
    out = {"bench": "pgo_marginals", "device": e.device_name(), "reps": a.reps, "lambda_of_the_column_solves": LAM,
           "not_measured": ["hardware counters of marg_trsm_kernel", "the gaps between the launches of a group", "graphs near the cap of 1 024 junctions"],
           "graphs": {}}
    for name in a.only:
        print(f"{name}: building the graph", file=sys.stderr, flush=True)
        g = GRAPHS[name]()
        n = len(g.poses)
        nj, ns, longest = e.pgo_count_junctions(n, g.f_i, g.f_j, g.p_idx)
        row = {"poses": n, "factors": int(len(g.f_i)), "junctions": nj, "segments": ns, "longest_segment": longest, "marginals": {}, "solve_many": {}}
        out["graphs"][name] = row
        # the single step: one right-hand side
        e.pgo_solve_condensed(*g, LAM)
        e.profile_enable(1)
        single = []
        for _ in range(a.reps):
            e.pgo_solve_condensed(*g, LAM); single.append(e.pgo_condensed_last_timing())
        e.profile_enable(0)
        single = np.median(np.array(single), axis=0)
        row["single_step_ms"] = {"elimination": float(single[0]), "assembly": float(single[1]), "factorisation": float(single[2]),
                                 "solve_and_back_substitution": float(single[3])}
        print(f"{name}: the checker's matrix and scipy's factorisation", file=sys.stderr, flush=True)
        lin = pg.linearize_numpy(g)
        lu, lu_ms = {}, {}
        for lam in (0.0, LAM):
            H = pg.hessian(lin, lam).tocsc()
            t = time.perf_counter(); lu[lam] = spla.splu(H); lu_ms[lam] = (time.perf_counter() - t) * 1e3
        row["splu_factorisation_ms"] = {"lambda_0": lu_ms[0.0], "lambda_1e-5": lu_ms[LAM]}
        for k in MARGINAL_POSES:
            print(f"{name}: marginals of {k} poses", file=sys.stderr, flush=True)
            sel = np.unique(np.linspace(0, n - 1, k).astype(np.int32))
            qi, qj = sel, np.roll(sel, -1)
            r = _timed(e, lambda: e.pgo_marginals(*g, qi, qj), a.reps)
            cols = 6 * len(sel)
            r["columns"] = cols
            r["single_step_ms3_times_columns"] = float(single[3]) * cols
            if 8.0 * 6 * n * cols <= a.host_bytes:
                B = np.zeros((6 * n, cols))
                for u, p in enumerate(sel):
                    B[6 * p:6 * p + 6, 6 * u:6 * u + 6] = np.eye(6)
                t = time.perf_counter(); lu[0.0].solve(B); r["splu_solve_ms"] = (time.perf_counter() - t) * 1e3
            else:
                r["splu_solve_ms"] = None; r["splu_left_out"] = "the columns exceed --host-bytes"
            row["marginals"][str(k)] = r
        rs = np.random.RandomState(n)
        for cols in COLUMNS:
            if 2 * 8.0 * 6 * n * cols > a.host_bytes:
                row["solve_many"][str(cols)] = {"left_out": "rhs and x exceed --host-bytes on the host"}
                continue
            print(f"{name}: {cols} columns", file=sys.stderr, flush=True)
            b = rs.standard_normal((cols, n, 6))
            r = _timed(e, lambda: e.pgo_solve_condensed_many(*g, LAM, b), a.reps)
            r["single_step_ms3_times_columns"] = float(single[3]) * cols
            B = np.ascontiguousarray(b.reshape(cols, -1).T)
            t = time.perf_counter(); lu[LAM].solve(B); r["splu_solve_ms"] = (time.perf_counter() - t) * 1e3
            row["solve_many"][str(cols)] = r
            del b, B
    e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
