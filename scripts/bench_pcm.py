#!/usr/bin/env python
"""Pairwise consistency of loop closures (scl_pcm_select) at N = 256, 1024 and 4096 loops, 60 % inliers: one JSON line.

Per N: the median wall time of scl_pcm_select, the median device time of its two stages (scl_pcm_last_timing under
scl_profile_enable(1): pre-pass + pair kernel + lower triangle, and clique kernel + finishing launch), and beside them the host's way:
the vectorised numpy restatement of the matrix (tests/pcm_cases.py d2_numpy), the greedy with numpy-kept counts (greedy_clique_fast)
and -- up to --greedy-max loops, above which it takes minutes to hours -- the plain Python greedy on the same graph.

    python scripts/bench_pcm.py [--reps 9] [--greedy-max 256]
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

import pcm_cases as pc                                    # noqa: E402
from scl_slam_amd import ScanContextEngine                # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--greedy-max", type=int, default=256)
    ap.add_argument("--sizes", type=int, nargs="*", default=[256, 1024, 4096])
    a = ap.parse_args()
    e = ScanContextEngine(initial_capacity=16)
    out = {"bench": "pcm_select", "device": e.device_name(), "threshold": pc.THRESHOLD, "inlier_fraction": 0.6, "reps": a.reps, "sizes": {}}
    for n in a.sizes:
        c, d2 = pc.case_and_d2("mixed", n)
        args = (c.poses_a, c.poses_b, c.idx_a, c.idx_b, c.z, c.cov, c.threshold)
        e.pcm_select(*args, odom_var=c.odom_var)                                   # warm-up: allocations
        wall, pairs, clique = [], [], []
        e.profile_enable(1)
        for _ in range(a.reps):
            t = time.perf_counter(); mem, seed, deg = e.pcm_select(*args, odom_var=c.odom_var); wall.append((time.perf_counter() - t) * 1e3)
            p, q = e.pcm_last_timing(); pairs.append(p); clique.append(q)
        e.profile_enable(0)
        t = time.perf_counter(); host = pc.d2_numpy(c); numpy_ms = (time.perf_counter() - t) * 1e3
        g = pc.graph(host, c.threshold)
        row = {"select_ms": float(np.median(wall)), "pairs_kernels_ms": float(np.median(pairs)), "clique_kernels_ms": float(np.median(clique)),
               "numpy_matrix_ms": numpy_ms, "members": int(len(mem)), "seed": int(seed), "density": float(g.mean()),
               "graph_equals_numpy": bool(np.array_equal(deg, g.sum(1)))}
        t = time.perf_counter(); want = pc.greedy_clique_fast(g); row["numpy_greedy_ms"] = (time.perf_counter() - t) * 1e3
        row["clique_equals_numpy_greedy"] = bool(want == (tuple(mem.tolist()), seed))
        if n <= a.greedy_max:
            t = time.perf_counter(); want = pc.greedy_clique(g); row["python_greedy_ms"] = (time.perf_counter() - t) * 1e3
            row["clique_equals_python"] = bool(want == (tuple(mem.tolist()), seed))
        out["sizes"][str(n)] = row
    e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
