"""M2DP plugin benchmark (include/scl_m2dp.h): prints one JSON line.

  make_and_save_many over groups of 16 x 120 k-point synth_scan clouds: device time of the kernel chain per scan (events around
  the chain, copies excluded) and wall time per scan (host copies included); (point, plane) decisions per second of device
  time; the share of decisions that took the exact theta-edge path; detect_intra at 10 k keyframes; and the numpy checker's
  time per scan beside it (a sanity figure only: the reference's PCL / Eigen path is not built here).
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
    ap.add_argument("--groups", type=int, default=8, help="timed launch groups of 16 scans")
    ap.add_argument("--keyframes", type=int, default=10000)
    ap.add_argument("--queries", type=int, default=200)
    ap.add_argument("--checker-scans", type=int, default=1)
    a = ap.parse_args()
    from scl_slam_amd import M2dpEngine
    from scl_slam_amd.synth import synth_scan
    import m2dp_checker as mc

    clouds = [synth_scan(a.points, seed=700 + i) for i in range(16)]
    eng = M2dpEngine()
    eng.make_and_save_many(clouds, want_values=False)                   # warm-up: code objects, buffers
    d0, e0, us0 = eng.stats()
    t0 = time.perf_counter()
    for _ in range(a.groups):
        eng.make_and_save_many(clouds, want_values=False)
    wall = time.perf_counter() - t0
    d1, e1, us1 = eng.stats()
    scans = 16 * a.groups
    dev_us = (us1 - us0) / scans
    # detect_intra over 10 k stored keyframes (from the wire: 192 floats each)
    det = M2dpEngine(num_exclude_recent=30)
    rs = np.random.RandomState(1)
    sigs = np.abs(rs.standard_normal((a.keyframes, 192))).astype(np.float32)
    sigs /= np.linalg.norm(sigs, axis=1, keepdims=True)
    for k in range(a.keyframes):
        det.save_from_wire(sigs[k], 0, k)
    for _ in range(10):
        det.detect_intra(a.keyframes - 1)
    t0 = time.perf_counter()
    for q in range(a.queries):
        det.detect_intra(a.keyframes - 1 - (q % 100))
    det_us = (time.perf_counter() - t0) / a.queries * 1e6
    from bench_plugin_detect import time_detect
    many = time_detect(det, "intra", a.keyframes, a.queries)             # the batch form at 16 and 256 queries, [min, median, max]
    t0 = time.perf_counter()
    for i in range(a.checker_scans):
        mc.signature(clouds[i])
    chk_ms = (time.perf_counter() - t0) / a.checker_scans * 1e3
    print(json.dumps({
        "metric": "m2dp_make_and_save_many_us_per_scan", "points": a.points, "group": 16, "scans": scans,
        "device_us_per_scan": round(dev_us, 2), "wall_us_per_scan": round(wall / scans * 1e6, 2),
        "decisions_per_s": round((d1 - d0) / ((us1 - us0) * 1e-6), 1) if us1 > us0 else None,
        "exact_path_share": (e1 - e0) / max(1, d1 - d0),
        "detect_intra_us_at_keyframes": round(det_us, 2), "keyframes": a.keyframes,
        "detect_intra_many_us_per_query": {"16": many["detect_intra_many_us_per_query_at_16"], "256": many["detect_intra_many_us_per_query_at_256"]},
        "checker_ms_per_scan": round(chk_ms, 1),
    }))
    eng.close(); det.close()


if __name__ == "__main__":
    main()
