#!/usr/bin/env python
"""The condensed direct step (scl_pgo_optimize_condensed) beside the PCG path (scl_pgo_optimize) on the same graphs, in the same
process and run: one JSON line.

The graphs are tests/pgo_cases.py drifting_graph at 1 000, 4 097 and 10 000 poses with loops at 3 % of the poses, at 30 000 and 100 000
poses with loops at 0.3 %, and a loop-free chain of 100 000 poses.  Every graph's junctions are counted first
(scl_pgo_count_junctions); one over the cap of 1 024 is reported as such and left out.  Per graph, with the default parameters, medians
of --reps runs: the wall time of each call (inputs over PCIe, poses back), the LM iterations, the stop and the final cost; under
scl_profile_enable(1) the device time of the condensed call's stages by HIP events (elimination, assembly of S, factorisation, the
triangular solves with the way back: scl_pgo_condensed_last_timing, each summed over the call's steps and divided by their number);
and the checker's loop (lm_numpy: scipy's sparse direct solve) up to --checker-max poses.  What is not measured is null.

    python scripts/bench_pgo_condensed.py [--reps 3] [--checker-max 10000] [--only NAME ...]
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
import pgo_condensed_cases as cc                          # noqa: E402
from scl_slam_amd import PgoParams, ScanContextEngine     # noqa: E402

GRAPHS = {
    "drifting1000": lambda: pg.drifting_graph(1000),
    "drifting4097": lambda: pg.drifting_graph(4097),
    "drifting10000": lambda: pg.drifting_graph(10000),
    "drifting30000_0.3pct": lambda: pg.drifting_graph(30000, loop_frac=0.003),
    "drifting100000_0.3pct": lambda: pg.drifting_graph(100000, loop_frac=0.003),
    "chain100000": lambda: cc.plain_chain(100000),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--checker-max", type=int, default=10000)
    ap.add_argument("--only", nargs="*", default=list(GRAPHS))
    a = ap.parse_args()
    e = ScanContextEngine(initial_capacity=16)
    prm = PgoParams.defaults()
    out = {"bench": "pgo_optimize_condensed", "device": e.device_name(), "reps": a.reps,
           "params": {k: getattr(prm, k) for k, _ in PgoParams._fields_}, "not_measured": ["hardware counters of the Cholesky's trailing update"],
           "graphs": {}}
    for name in a.only:
        print(f"{name}: building the graph", file=sys.stderr, flush=True)
        g = GRAPHS[name]()
        n = len(g.poses)
        nj, ns, longest = e.pgo_count_junctions(n, g.f_i, g.f_j, g.p_idx)
        row = {"poses": n, "factors": int(len(g.f_i)), "junctions": nj, "segments": ns, "longest_segment": longest}
        out["graphs"][name] = row
        if nj > cc.MAX_JUNCTIONS:
            row["left_out"] = "more than 1024 junctions"
            continue
        print(f"{name}: {nj} junctions, {ns} segments; the condensed solve", file=sys.stderr, flush=True)
        e.pgo_optimize_condensed(*g, params=prm, want_chi2=False)                  # warm-up: allocations
        wall, stages, solve = [], [], []
        e.profile_enable(1)
        for _ in range(a.reps):
            t = time.perf_counter(); X, res, _, failed = e.pgo_optimize_condensed(*g, params=prm, want_chi2=False)
            wall.append((time.perf_counter() - t) * 1e3)
            stages.append(np.array(e.pgo_condensed_last_timing()) / res.iterations); solve.append(e.pgo_last_timing())
        e.profile_enable(0)
        st = np.median(np.array(stages), axis=0)
        row["condensed"] = {"optimize_ms": float(np.median(wall)), "lm_iterations": res.iterations, "accepted": res.accepted, "rejected": res.rejected,
                            "failed_factorisations": failed, "stop_reason": res.stop_reason, "initial_cost": res.initial_cost,
                            "final_cost": res.final_cost, "gradient_max": res.gradient_max,
                            "linearize_kernels_ms": float(np.median([s[0] for s in solve])), "solve_kernels_ms": float(np.median([s[1] for s in solve])),
                            "per_step_ms": {"elimination": float(st[0]), "assembly": float(st[1]), "factorisation": float(st[2]),
                                            "solves_and_back_substitution": float(st[3])}}
        print(f"{name}: the PCG path", file=sys.stderr, flush=True)
        e.pgo_optimize(*g, params=prm, want_chi2=False)
        wall = []
        for _ in range(a.reps):
            t = time.perf_counter(); X, res, _ = e.pgo_optimize(*g, params=prm, want_chi2=False); wall.append((time.perf_counter() - t) * 1e3)
        row["pcg"] = {"optimize_ms": float(np.median(wall)), "lm_iterations": res.iterations, "cg_iterations": res.cg_iterations,
                      "stop_reason": res.stop_reason, "final_cost": res.final_cost}
        row["scipy_loop"] = None
        if n <= a.checker_max:
            print(f"{name}: the checker's loop", file=sys.stderr, flush=True)
            t = time.perf_counter(); _, info = pg.lm_numpy(g, pg.DEFAULTS); host_ms = (time.perf_counter() - t) * 1e3
            row["scipy_loop"] = {"ms": host_ms, "lm_iterations": info["iterations"], "stop_reason": info["stop_reason"], "final_cost": info["final_cost"]}
    e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
