"""Point-to-plane registration scoring benchmark (include/scl_engine.h "POINT-TO-PLANE REGISTRATION SCORING"): prints one JSON line.

  bench.py's ICP problem (BASELINE configs[2]: one scan against 25 candidates of 100 k points, all in the keyframe store), scored at
  the T of one guessed point-to-point loop ICP (identity guesses, 30 iterations), as scripts/bench_registration_eval.py scores it.
  1. `plane_ms`: scl_loop_eval_plane_batch_from_store, wall time of the whole call, --reps runs after a warm-up; `plane_median_ms`.
  2. `eval_ms`: scl_loop_eval_batch_from_store in the same process on the same inputs, interleaved with 1.; `eval_median_ms`.
  The difference is the normals' launch (one over all candidates), the cells' ordering and the heavier reduction.  `min_over_max_eig` is
  the smallest over the largest eigenvalue of every candidate's 6 x 6 matrix, `rmse_plane` its root mean square point-to-plane distance.
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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--max-dist", type=float, default=0.5)
    ap.add_argument("--normal-radius", type=float, default=1.0)
    ap.add_argument("--plane-only", action="store_true", help="the new call alone (for a kernel trace)")
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
           "normal_radius": a.normal_radius, "points_src": int(icp[5]), "points_tgt_mean": float(np.mean(icp[6]))}

    def timed(f):
        t0 = time.perf_counter()
        r = f()
        return (time.perf_counter() - t0) * 1e3, r

    def plane():
        return eng.loop_eval_plane_batch_from_store(0, n, ident, keys, 0, poses, 0.05, T, a.max_dist, a.normal_radius)

    def point():
        return eng.loop_eval_batch_from_store(0, n, ident, keys, 0, poses, 0.05, T, a.max_dist)

    plane()
    if not a.plane_only:
        point()
    pl, ev = [], []
    for _ in range(a.reps):
        pl.append(timed(plane))
        if not a.plane_only:
            ev.append(timed(point))
    got = pl[-1][1]
    out["plane_ms"] = [round(t, 3) for t, _ in pl]
    out["plane_median_ms"] = round(float(np.median(out["plane_ms"])), 3)
    if ev:
        ref = ev[-1][1]
        out["eval_ms"] = [round(t, 3) for t, _ in ev]
        out["eval_median_ms"] = round(float(np.median(out["eval_ms"])), 3)
        out["counts_and_d2_equal_eval"] = bool(np.array_equal(got.n_valid, ref.n_valid) and np.array_equal(got.n_inliers, ref.n_inliers)
                                               and np.array_equal(got.sums[:, 28].view(np.uint64), ref.moments[:, 9].view(np.uint64)))
    out["n_inliers"] = [int(v) for v in got.n_inliers]
    out["n_planar"] = [int(v) for v in got.n_planar]
    eig = [np.linalg.eigvalsh(got.information(c)) for c in range(n)]
    out["min_over_max_eig"] = [float(w[0] / w[-1]) if w[-1] > 0 else None for w in eig]
    out["rmse_plane"] = [round(got.rmse_plane(c), 5) for c in range(n)]
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
