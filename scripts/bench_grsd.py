"""GRSD plugin benchmark (include/scl_grsd.h): prints one JSON line.

  Inputs: 16 synthetic scans, once through the 0.4 m voxel filter (scl_voxel_grid; --filtered-points raw points each, ~20 k after
  the filter: the cloud the reference's method receives, DM.h:185, 501, 996-1001) and once raw (--raw-points, 120 000).  Per input
  and repetition (--reps, at least five), after a warm-up: make_and_save_many over --groups launch groups of 16; device time of the
  kernel chain per scan (events around the chain, copies excluded) and wall time per scan (host copies included), each reported as
  [min, median, max] over the repetitions.  Beside them the CPU checker's time on ONE core for one cloud of each input (brute
  force: the only CPU comparator available, not the reference's time -- PCL is not built here).  The kernel split comes from a
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


def _range(xs):
    return [round(float(min(xs)), 2), round(float(np.median(xs)), 2), round(float(max(xs)), 2)]


def measure(engine_cls, clouds, groups, reps):
    eng = engine_cls()
    eng.make_and_save_many(clouds, want_values=False)                   # warm-up: code objects, buffers
    dev, wall = [], []
    voxels = 0
    for _ in range(reps):
        p0, v0, us0 = eng.stats()
        t0 = time.perf_counter()
        for _ in range(groups):
            eng.make_and_save_many(clouds, want_values=False)
        w = time.perf_counter() - t0
        p1, v1, us1 = eng.stats()
        scans = len(clouds) * groups
        dev.append((us1 - us0) / scans); wall.append(w / scans * 1e6)
        voxels = (v1 - v0) / scans
    eng.close()
    return _range(dev), _range(wall), voxels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--filtered-points", type=int, default=25000, help="raw points of the scans that go through the filter")
    ap.add_argument("--raw-points", type=int, default=120000)
    ap.add_argument("--leaf", type=float, default=0.4)
    ap.add_argument("--groups", type=int, default=4, help="timed launch groups of 16 scans per repetition")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--keyframes", type=int, default=10000, help="stored keyframes of the detection timing")
    ap.add_argument("--checker", type=int, default=1, help="0: skip the CPU checker's one-core time")
    a = ap.parse_args()
    from scl_slam_amd import GrsdEngine, ScanContextEngine
    from scl_slam_amd.synth import synth_scan

    sc = ScanContextEngine()
    filtered = [np.ascontiguousarray(sc.voxel_grid(synth_scan(a.filtered_points, seed=700 + i, stride_floats=4), a.leaf)) for i in range(16)]
    sc.close()
    raw = [synth_scan(a.raw_points, seed=800 + i, stride_floats=4) for i in range(16)]
    out = {"metric": "grsd_make_and_save_many_us_per_scan", "group": 16, "scans_per_rep": 16 * a.groups, "reps": a.reps,
           "range": "[min, median, max] over the repetitions"}
    for name, clouds in (("filtered", filtered), ("raw", raw)):
        dev, wall, voxels = measure(GrsdEngine, clouds, a.groups, max(5, a.reps))
        ns = [c.shape[0] for c in clouds]
        out[name] = {"points_mean": round(float(np.mean(ns)), 1), "voxels_mean": round(float(voxels), 1), "device_us_per_scan": dev,
                     "wall_us_per_scan": wall}
        if a.checker:
            import grsd_checker as gc
            t0 = time.perf_counter()
            gc.describe(clouds[0], threads=1)
            out[name]["checker_one_core_ms_per_scan"] = round((time.perf_counter() - t0) * 1e3, 1)
    # detect_inter over --keyframes stored keyframes (from the wire: 21 floats each), the reference's mode: the single call and the
    # batch form at 16 and 256 queries, [min, median, max]
    from bench_plugin_detect import time_detect, wire_rows
    det = GrsdEngine()
    rows = wire_rows("grsd", a.keyframes)
    for k in range(a.keyframes):
        det.save_from_wire(rows[k], 0, k)
    many = time_detect(det, "inter", a.keyframes, 200, max(5, a.reps))
    det.close()
    out["keyframes"] = a.keyframes
    out["detect_inter_us_at_keyframes"] = many["detect_inter_us_per_query"]
    out["detect_inter_many_us_per_query"] = {"16": many["detect_inter_many_us_per_query_at_16"], "256": many["detect_inter_many_us_per_query_at_256"]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
