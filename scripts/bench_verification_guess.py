"""Guessed batched geometric verification benchmark (include/scl_engine.h "THE BATCHED VERIFICATION WITH INITIAL GUESSES"): prints one
JSON line.

  The shape of scripts/bench_verification_batch.py: one received scan against 25 candidates from the keyframe store, 100 k points per
  cloud, submaps of one keyframe, leaf 0.05 m, 1 000 hypotheses.  ONE scl_geometric_verification_batch_from_store_guess call against ONE
  scl_geometric_verification_batch_from_store call: after a warm-up of both, --reps repetitions of each, alternating, wall time of the
  whole call.  The difference is the price of the per-candidate sources (one launch that writes 16 bytes x points x candidates, and
  the cold search, RANSAC and covariance reading them in place of one shared cloud).  --guess identity (default) moves nothing, so
  the two calls do the same arithmetic and their answers must agree (`bit_equal`); --guess inverse hands every candidate the
  inverse of the scan's true motion, so the searches start aligned.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=25)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--hypotheses", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--leaf", type=float, default=0.05)
    ap.add_argument("--guess", choices=("identity", "inverse"), default="identity")
    ap.add_argument("--guessed-only", action="store_true", help="one warm-up and --reps guessed calls (for a kernel trace)")
    a = ap.parse_args()
    from bench_verification_batch import clouds
    from scl_slam_amd import ScanContextEngine
    from scl_slam_amd.synth import rigid_transform

    eng = ScanContextEngine()
    tgts, src = clouds(a.candidates, a.points)
    for c, t in enumerate(tgts):
        eng.keyframe_put(0, c, t)
    ident = np.eye(4, dtype=np.float32)
    keys = np.arange(a.candidates, dtype=np.int32)
    poses = np.tile(ident.reshape(1, 1, 16), (a.candidates, 1, 1))
    G = ident if a.guess == "identity" else np.linalg.inv(rigid_transform(0.004, -0.006, 0.02, 0.25, -0.15, 0.05)).astype(np.float32)
    guesses = np.tile(G.reshape(1, 4, 4), (a.candidates, 1, 1))
    args = (a.hypotheses, 0.25, 0.45, 1)

    def plain():
        return eng.geometric_verification_batch_from_store(src, a.leaf, 0, keys, 0, poses, a.leaf, *args)

    def guessed():
        return eng.geometric_verification_batch_from_store_guess(src, a.leaf, 0, keys, 0, poses, a.leaf, guesses, *args)

    def timed(f):
        t0 = time.perf_counter()
        r = f()
        return (time.perf_counter() - t0) * 1e3, r

    out = {"metric": "geometric_verification_batch_from_store_guess_ms", "device": eng.device_name(), "candidates": a.candidates,
           "points": a.points, "hypotheses": a.hypotheses, "leaf": a.leaf, "reps": a.reps, "guess": a.guess}
    got = guessed()                                                   # warm-up (code objects, workspaces)
    out.update(points_src=int(got[2]), points_tgt_mean=float(np.mean(got[3])), successes=int(got[1].sum()), inliers=[int(x) for x in got[5]])
    if not a.guessed_only:
        ref = plain()                                                 # warm-up
        if a.guess == "identity":
            out["bit_equal"] = bool(np.array_equal(got[6].view(np.uint32), ref[0].view(np.uint32)) and np.array_equal(got[0], ref[0]) and
                                    all(np.array_equal(got[i], ref[i]) for i in (1, 3, 4, 5)) and got[2] == ref[2])
    plain_ms, guess_ms = [], []
    for _ in range(a.reps):
        if not a.guessed_only:
            plain_ms.append(timed(plain)[0])
        guess_ms.append(timed(guessed)[0])
    rnd = lambda v: [round(x, 3) for x in v]
    out.update(guessed_ms=rnd(guess_ms), guessed_ms_median=round(float(np.median(guess_ms)), 3))
    if plain_ms:
        out.update(batch_ms=rnd(plain_ms), batch_ms_median=round(float(np.median(plain_ms)), 3),
                   guessed_minus_batch_ms=round(float(np.median(guess_ms) - np.median(plain_ms)), 3),
                   guessed_over_batch=round(float(np.median(guess_ms) / np.median(plain_ms)), 3))
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
