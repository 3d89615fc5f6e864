#!/usr/bin/env python
"""The pose-graph solve (scl_pgo_optimize) on 1 000, 10 000 and 100 000 poses of a planted multi-loop trajectory: one JSON line.

The graph is tests/pgo_cases.py drifting_graph: odometry with drift (every measurement behind noise drawn from its own covariance),
loops at 3 % of the poses, one prior, started from the chained odometry.  Per size, with the default parameters: the wall time of
scl_pgo_optimize (inputs over PCIe, poses back), the device time of its two stages (scl_pgo_last_timing under scl_profile_enable(1):
linearisation + assembly, PCG + retraction), the LM and CG iteration counts, the stop reason and the final cost; and beside them the
checker's loop on the same graph (lm_numpy: scipy's sparse direct solve, the same accept / reject rule), capped at --checker-iterations
iterations: its time, its iterations and the cost it reached -- up to --checker-max poses: the loops are chords between far-apart poses,
and the fill-in of a sparse direct factorisation grows with their number (3 000 chords at 100 000 poses: more than 5 GB and an hour of
CPU time without an answer).

    python scripts/bench_pgo.py [--sizes 1000 10000 100000] [--reps 3] [--checker-iterations 10] [--checker-max 10000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pgo_cases as pg                                    # noqa: E402
from scl_slam_amd import PgoParams, ScanContextEngine     # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[1000, 10000, 100000])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--checker-iterations", type=int, default=10)
    ap.add_argument("--checker-max", type=int, default=10000)
    a = ap.parse_args()
    e = ScanContextEngine(initial_capacity=16)
    prm = PgoParams.defaults()
    out = {"bench": "pgo_optimize", "device": e.device_name(), "loop_fraction": 0.03, "reps": a.reps,
           "params": {k: getattr(prm, k) for k, _ in PgoParams._fields_}, "sizes": {}}
    for n in a.sizes:
        print(f"{n} poses: building the graph", file=sys.stderr, flush=True)
        g = pg.drifting_graph(n)
        print(f"{n} poses: {len(g.f_i)} factors, solving", file=sys.stderr, flush=True)
        e.pgo_optimize(*g, params=prm, want_chi2=False)                            # warm-up: allocations
        wall, lin, solve = [], [], []
        e.profile_enable(1)
        for _ in range(a.reps):
            t = time.perf_counter(); X, res, _ = e.pgo_optimize(*g, params=prm, want_chi2=False); wall.append((time.perf_counter() - t) * 1e3)
            p, q = e.pgo_last_timing(); lin.append(p); solve.append(q)
        e.profile_enable(0)
        host_ms, info = None, {"iterations": None, "stop_reason": None, "final_cost": None}
        if n <= a.checker_max:
            print(f"{n} poses: the checker's loop", file=sys.stderr, flush=True)
            t = time.perf_counter(); _, info = pg.lm_numpy(g, dict(pg.DEFAULTS, max_iterations=a.checker_iterations)); host_ms = (time.perf_counter() - t) * 1e3
        out["sizes"][str(n)] = {
            "factors": int(len(g.f_i)), "optimize_ms": float(np.median(wall)), "linearize_kernels_ms": float(np.median(lin)),
            "solve_kernels_ms": float(np.median(solve)), "lm_iterations": res.iterations, "accepted": res.accepted, "rejected": res.rejected,
            "cg_iterations": res.cg_iterations, "stop_reason": res.stop_reason, "initial_cost": res.initial_cost, "final_cost": res.final_cost,
            "gradient_max": res.gradient_max, "scipy_loop_ms": host_ms, "scipy_loop_iterations": info["iterations"],
            "scipy_loop_stop_reason": info["stop_reason"], "scipy_loop_final_cost": info["final_cost"]}
    e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
