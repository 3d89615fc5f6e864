"""Ranked search benchmark (include/scl_engine.h, THE RANKED SEARCH): prints one JSON line.

  10 k keyframes at 64x120, 16 queries per call, k = 25: wall time per sc_search call and (query, keyframe) pairs per second --
  and, in the same run, the same job the old way: sc_distance_matrix of the same queries over the same keyframes (every pair's
  distance and shift to the host) and a numpy sort of every row there.  Both answers are compared before anything is timed.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=10000)
    ap.add_argument("--rings", type=int, default=64)
    ap.add_argument("--sectors", type=int, default=120)
    ap.add_argument("--queries", type=int, default=16)
    ap.add_argument("--k", type=int, default=25)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    from scl_slam_amd import ScanContextEngine
    from scl_slam_amd.synth import synth_descriptors
    from sc_search_cases import ranked

    n, k = a.keyframes, a.k
    eng = ScanContextEngine(num_ring=a.rings, num_sector=a.sectors, num_exclude_recent=0, initial_capacity=n)
    eng.save_bulk(synth_descriptors(n, a.rings, a.sectors, seed=1002, revisit_frac=0.01))
    curs = np.full(a.queries, n, dtype=np.int32) - 1 - np.arange(a.queries, dtype=np.int32)    # the newest keyframes
    hi = int(curs.min())                                                                         # one range for all: what the matrix call takes

    def old_way():
        d, s = eng.sc_distance_matrix(curs, 0, hi)
        return [ranked(d[i], s[i], 0, hi, k) for i in range(len(curs))]

    def new_way():
        return eng.sc_search_range(curs, 0, hi, k)

    got, want = new_way(), old_way()
    for i in range(len(curs)):
        assert np.array_equal(got[0][i], want[i][0]) and np.array_equal(got[1][i], want[i][1]) and got[3][i] == want[i][3]
        assert np.array_equal(got[2][i].view(np.uint64), want[i][2].view(np.uint64))

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        t = []
        for _ in range(a.calls):
            t0 = time.perf_counter(); fn(); t.append(time.perf_counter() - t0)
        return np.array(t) * 1e6

    t_new, t_old = timed(new_way), timed(old_way)
    t_mat = timed(lambda: eng.sc_distance_matrix(curs, 0, hi))
    pairs = float(a.queries) * hi
    print(json.dumps({
        "metric": "sc_search_us_per_call", "grid": f"{a.rings}x{a.sectors}", "keyframes": n, "queries_per_call": a.queries, "k": k, "calls": a.calls,
        "sc_search_us_per_call": {"min": round(float(t_new.min()), 1), "median": round(float(np.median(t_new)), 1), "max": round(float(t_new.max()), 1)},
        "sc_search_pairs_per_s": round(pairs / (float(np.median(t_new)) * 1e-6), 1),
        "matrix_plus_host_sort_us_per_call": {"min": round(float(t_old.min()), 1), "median": round(float(np.median(t_old)), 1), "max": round(float(t_old.max()), 1)},
        "matrix_plus_host_sort_pairs_per_s": round(pairs / (float(np.median(t_old)) * 1e-6), 1),
        "matrix_alone_us_per_call": round(float(np.median(t_mat)), 1),
        "matrix_alone_pairs_per_s": round(pairs / (float(np.median(t_mat)) * 1e-6), 1),
    }))
    eng.close()


if __name__ == "__main__":
    main()
