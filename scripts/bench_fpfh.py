"""FPFH plugin benchmark (include/scl_fpfh.h): prints one JSON line.

  Inputs: synth_scan(120 000) clouds through the 0.4 m voxel filter (scl_voxel_grid), the cloud the reference's method receives
  (DM.h:185, 501, 996-1001); N is printed.  make_and_save_many over groups of 16 after a warm-up: device time of the kernel chain
  per scan (events around the chain, copies excluded), wall time per scan (host copies included), candidate distances of the
  neighbour search per point; detect_inter (the reference's mode) at 10 k keyframes; and the CPU checker's time per scan beside it
  (brute-force neighbours: a sanity figure, not the reference's time -- PCL is not built here).  The kernel split comes from a
  separate `rocprofv3 --kernel-trace --stats` run of this script.
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
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--leaf", type=float, default=0.4)
    ap.add_argument("--groups", type=int, default=8, help="timed launch groups of 16 scans")
    ap.add_argument("--keyframes", type=int, default=10000)
    ap.add_argument("--queries", type=int, default=200)
    ap.add_argument("--checker-scans", type=int, default=0, help="scans timed through the brute-force CPU checker (slow at ~96 k)")
    a = ap.parse_args()
    from scl_slam_amd import FpfhEngine, ScanContextEngine
    from scl_slam_amd.synth import synth_scan

    sc = ScanContextEngine()
    clouds = [np.ascontiguousarray(sc.voxel_grid(synth_scan(a.points, seed=700 + i, stride_floats=4), a.leaf)) for i in range(16)]
    sc.close()
    ns = [c.shape[0] for c in clouds]
    eng = FpfhEngine()
    eng.make_and_save_many(clouds, want_values=False)                   # warm-up: code objects, buffers
    p0, c0, us0 = eng.stats()
    t0 = time.perf_counter()
    for _ in range(a.groups):
        eng.make_and_save_many(clouds, want_values=False)
    wall = time.perf_counter() - t0
    p1, c1, us1 = eng.stats()
    scans = 16 * a.groups
    dev_us = (us1 - us0) / scans
    # detect_inter over 10 k stored keyframes (from the wire: 33 floats each), the reference's mode
    det = FpfhEngine()
    rs = np.random.RandomState(1)
    keys = (100.0 * rs.dirichlet(np.full(11, 0.7), size=(a.keyframes, 3)).reshape(a.keyframes, 33)).astype(np.float32)
    for k in range(a.keyframes):
        det.save_from_wire(keys[k], 0, k)
    for _ in range(10):
        det.detect_inter(a.keyframes - 1)
    t0 = time.perf_counter()
    for q in range(a.queries):
        det.detect_inter(a.keyframes - 1 - (q % 100))
    det_us = (time.perf_counter() - t0) / a.queries * 1e6
    from bench_plugin_detect import time_detect
    many = time_detect(det, "inter", a.keyframes, a.queries)             # the batch form at 16 and 256 queries, [min, median, max]
    chk_ms = None
    if a.checker_scans > 0:
        import fpfh_checker as fc
        t0 = time.perf_counter()
        for i in range(a.checker_scans):
            fc.describe(clouds[i])
        chk_ms = round((time.perf_counter() - t0) / a.checker_scans * 1e3, 1)
    print(json.dumps({
        "metric": "fpfh_make_and_save_many_us_per_scan", "raw_points": a.points, "leaf": a.leaf,
        "points_min": min(ns), "points_mean": round(float(np.mean(ns)), 1), "points_max": max(ns), "group": 16, "scans": scans,
        "device_us_per_scan": round(dev_us, 2), "wall_us_per_scan": round(wall / scans * 1e6, 2),
        "candidates_per_point": round((c1 - c0) / max(1, p1 - p0), 1),
        "detect_inter_us_at_keyframes": round(det_us, 2), "keyframes": a.keyframes,
        "detect_inter_many_us_per_query": {"16": many["detect_inter_many_us_per_query_at_16"], "256": many["detect_inter_many_us_per_query_at_256"]},
        "checker_ms_per_scan": chk_ms,
    }))
    eng.close(); det.close()


if __name__ == "__main__":
    main()
