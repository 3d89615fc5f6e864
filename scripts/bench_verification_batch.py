"""Batched geometric verification benchmark (include/scl_engine.h "THE BATCHED VERIFICATION"): prints one JSON line.

  One received scan against 25 candidates from the keyframe store, clouds sized as bench.py's configs[2] leg sizes them (100 k
  points per cloud, submaps of one keyframe, leaf 0.05 m), 1 000 hypotheses: ONE scl_geometric_verification_batch_from_store call
  against the loop of 25 scl_geometric_verification_from_store calls, the only way before the batch existed.  After a warm-up of
  both, --reps repetitions of each, alternating, wall time of the whole call (it ends in the host's wait for the device).  The
  batch counts as faster only if the two sets do not overlap.  On a build without the batch calls (--loop-only, or an older
  library) only the loop is timed.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def clouds(n_cand, n_pts):
    """bench.py's _icp_clouds: n_cand structured clouds and the scan = a moved, noisy copy of candidate 0 (the one true loop)"""
    from scl_slam_amd.synth import rigid_transform, synth_structured_cloud
    tgts = [synth_structured_cloud(n_pts, seed=100 + c, extent=60.0) for c in range(n_cand)]
    T = rigid_transform(0.004, -0.006, 0.02, 0.25, -0.15, 0.05)
    src = tgts[0].copy()
    p = tgts[0][:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    src[:, :3] = (p + 0.01 * np.random.RandomState(3).standard_normal(p.shape)).astype(np.float32)
    return tgts, src


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=25)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--hypotheses", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--leaf", type=float, default=0.05)
    ap.add_argument("--loop-only", action="store_true")
    ap.add_argument("--batch-only", action="store_true", help="one warm-up and --reps batch calls (for a kernel trace)")
    a = ap.parse_args()
    from scl_slam_amd import ScanContextEngine

    eng = ScanContextEngine()
    have_batch = hasattr(eng, "geometric_verification_batch_from_store") and not a.loop_only
    tgts, src = clouds(a.candidates, a.points)
    for c, t in enumerate(tgts):
        eng.keyframe_put(0, c, t)
    ident = np.eye(4, dtype=np.float32)
    keys = np.arange(a.candidates, dtype=np.int32)
    poses = np.tile(ident.reshape(1, 1, 16), (a.candidates, 1, 1))
    args = (a.hypotheses, 0.25, 0.45, 1)

    def loop():
        return [eng.geometric_verification_from_store(src, a.leaf, 0, int(k), 0, [ident], a.leaf, *args) for k in keys]

    def batch():
        return eng.geometric_verification_batch_from_store(src, a.leaf, 0, keys, 0, poses, a.leaf, *args)

    def timed(f):
        t0 = time.perf_counter()
        r = f()
        return (time.perf_counter() - t0) * 1e3, r

    out = {"metric": "geometric_verification_batch_from_store_ms", "device": eng.device_name(), "candidates": a.candidates,
           "points": a.points, "hypotheses": a.hypotheses, "leaf": a.leaf, "reps": a.reps}
    loop_ms, batch_ms = [], []
    if not a.batch_only:
        ref = loop()                                                    # warm-up (code objects, workspaces)
        out.update(points_src=int(ref[0][2]), points_tgt_mean=float(np.mean([r[3] for r in ref])),
                   successes=int(sum(r[1] for r in ref)), inliers=[int(r[5]) for r in ref])
    if have_batch:
        got = batch()                                                   # warm-up
        if not a.batch_only:
            out["bit_equal"] = bool(all(np.array_equal(got[0][c].view(np.uint32), r[0].view(np.uint32)) and
                                        (bool(got[1][c]), got[2], int(got[3][c]), int(got[4][c]), int(got[5][c])) == r[1:]
                                        for c, r in enumerate(ref)))
    for _ in range(a.reps):
        if not a.batch_only:
            loop_ms.append(timed(loop)[0])
        if have_batch:
            batch_ms.append(timed(batch)[0])
    rnd = lambda v: [round(x, 3) for x in v]
    if loop_ms:
        out.update(loop_ms=rnd(loop_ms), loop_ms_median=round(float(np.median(loop_ms)), 3))
    if batch_ms:
        out.update(batch_ms=rnd(batch_ms), batch_ms_median=round(float(np.median(batch_ms)), 3))
    if loop_ms and batch_ms:
        out.update(loop_over_batch=round(float(np.median(loop_ms) / np.median(batch_ms)), 3), faster=bool(max(batch_ms) < min(loop_ms)))
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
