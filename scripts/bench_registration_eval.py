"""Batched registration scoring benchmark (include/scl_engine.h "BATCHED REGISTRATION SCORING"): prints one JSON line.

  bench.py's ICP problem (BASELINE configs[2]: one scan against 25 candidates of 100 k points, all in the keyframe store).  The
  transforms are the T of one guessed point-to-point loop ICP (identity guesses, 30 iterations), so the scored registrations are real.
  1. `eval_ms`: scl_loop_eval_batch_from_store, wall time of the whole call, --reps runs after a warm-up; their median is `eval_median_ms`.
  2. `route_ms`: the same figures by calls that exist without the scoring calls -- per candidate scl_transform_cloud, then
     scl_nn_correspondences (the source uploaded again, 8 bytes per source point downloaded), then numpy for the counts and the ten
     sums -- with the source and the candidates' submaps already on the host (fetching them is not timed).  --route-only runs on a
     build without the new calls: time it on the parent commit's build.
  `fitness` is the guessed ICP's, `mse_inliers` is sum d2 / n_inliers of the eval at the ICP's max_correspondence_dist: the ICP moves
  the source in two float steps (guess, then T_icp), the eval in one (T), so the two differ in rounding.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=25)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-dist", type=float, default=0.5)
    ap.add_argument("--route-only", action="store_true")
    ap.add_argument("--skip-route", action="store_true", help="the new call alone (for a kernel trace)")
    a = ap.parse_args()
    import bench
    from scl_slam_amd import ScanContextEngine

    n = a.candidates
    eng = ScanContextEngine()
    tgts, src0 = bench._icp_clouds(n, a.points)
    for c in range(n):
        eng.keyframe_put(0, c, tgts[c])
    eng.keyframe_put(0, n, src0)
    ident = np.eye(4, dtype=np.float32)
    keys = np.arange(n, dtype=np.int32)
    poses = np.tile(ident.reshape(1, 1, 16), (n, 1, 1))
    guesses = np.tile(ident.reshape(1, 4, 4), (n, 1, 1))
    pp = eng.icp_default_params(); pp.max_iterations = 30; pp.estimator = 0
    icp = eng.loop_icp_batch_from_store_guess(0, n, ident, keys, 0, poses, 0.05, guesses, pp)
    T = icp[0]
    out = {"device": eng.device_name(), "candidates": n, "points": a.points, "reps": a.reps, "max_dist": a.max_dist,
           "points_src": int(icp[5]), "points_tgt_mean": float(np.mean(icp[6]))}

    def timed(f):
        t0 = time.perf_counter()
        r = f()
        return (time.perf_counter() - t0) * 1e3, r

    # today's route, from clouds that are already on the host
    src = eng.submap_from_store(0, n, 0, ident[None], 0.05, a.points)
    subs = [eng.submap_from_store(0, int(k), 0, ident[None], 0.05, a.points) for k in keys]
    maxd2 = np.float32(a.max_dist * a.max_dist)

    def route():
        nv, ni, mo = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros((n, 10))
        for c in range(n):
            idx, d2 = eng.nn_correspondences(eng.transform_cloud(src, T[c]), subs[c])
            inl = (idx >= 0) & (d2 <= maxd2)
            q = subs[c][idx[inl], :3].astype(np.float64)
            x, y, z = q[:, 0], q[:, 1], q[:, 2]
            nv[c], ni[c] = int((idx >= 0).sum()), int(inl.sum())
            mo[c] = [x.sum(), y.sum(), z.sum(), (x * x).sum(), (y * y).sum(), (z * z).sum(), (x * y).sum(), (x * z).sum(), (y * z).sum(),
                     d2[inl].astype(np.float64).sum()]
        return nv, ni, mo

    if not a.skip_route:
        route()
        rt = [timed(route) for _ in range(a.reps)]
        out["route_ms"] = [round(t, 3) for t, _ in rt]
        out["route_median_ms"] = round(float(np.median(out["route_ms"])), 3)
        rnv, rni, rmo = rt[-1][1]
    if not a.route_only:
        def call():
            return eng.loop_eval_batch_from_store(0, n, ident, keys, 0, poses, 0.05, T, a.max_dist)

        call()
        ev = [timed(call) for _ in range(a.reps)]
        got = ev[-1][1]
        out["eval_ms"] = [round(t, 3) for t, _ in ev]
        out["eval_median_ms"] = round(float(np.median(out["eval_ms"])), 3)
        if not a.skip_route:
            out["counts_equal_route"] = bool(np.array_equal(got.n_valid, rnv) and np.array_equal(got.n_inliers, rni))
            out["sums_max_rel_diff_to_route"] = float(np.max(np.abs(got.moments - rmo) / np.maximum(np.abs(rmo), 1e-300)))
        out["overlap"] = [round(float(v), 4) for v in got.overlap]
        out["rmse"] = [round(float(v), 5) for v in got.rmse]
        wide = eng.loop_eval_batch_from_store(0, n, ident, keys, 0, poses, 0.05, T, pp.max_correspondence_dist)
        out["fitness"] = [float(v) for v in icp[2]]
        out["mse_inliers"] = [float(s / max(int(m), 1)) for s, m in zip(wide.moments[:, 9], wide.n_inliers)]
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
