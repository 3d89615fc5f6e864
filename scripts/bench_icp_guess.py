"""Guessed batched ICP benchmark (include/scl_engine.h "THE BATCHED ICP WITH INITIAL GUESSES"): prints one JSON line.

  Two measurements on bench.py's ICP problem (BASELINE configs[2]: one scan against 25 candidates of 100 k points, max 30
  iterations, both estimators):
  1. `unguessed`: bench.py --full's secondary `icp_verification` (bench.secondary_icp itself) --reps times: from the store and from
     host buffers, both estimators, and the reference's settings.  Run on this build and on the parent commit's, each in a process
     of its own (--unguessed-only works on a build without the guessed calls), it is the check that the unguessed path kept its
     launches.
  2. `guessed`: ONE scl_loop_icp_batch_from_store_guess call against ONE scl_loop_icp_batch_from_store call, after a warm-up of
     both, --reps repetitions of each, alternating, wall time of the whole call.  Identity guesses, so the two do the same
     arithmetic and their answers must agree (`bit_equal`); the difference is the price of the per-candidate sources and orders:
     one streaming pass and one sort of 25 x 100 k keys where the unguessed call sorts 100 k.
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
    ap.add_argument("--unguessed-only", action="store_true")
    a = ap.parse_args()
    import bench
    from scl_slam_amd import ScanContextEngine

    eng = ScanContextEngine()
    out = {"device": eng.device_name(), "candidates": a.candidates, "points": a.points, "reps": a.reps, "unguessed": {}}
    for _ in range(a.reps):
        r = bench.secondary_icp(eng, a.candidates, a.points)
        for est in ("point_to_plane", "point_to_point"):
            for mode in ("from_store", "host_buffers"):
                out["unguessed"].setdefault(f"{est}/{mode}", []).append(round(r[est][mode]["ms_per_query"], 3))
        out["unguessed"].setdefault("point_to_point_reference_settings", []).append(round(r["point_to_point_reference_settings"]["ms_per_query"], 3))
    if not a.unguessed_only:
        ident = np.eye(4, dtype=np.float32)
        keys = np.arange(a.candidates, dtype=np.int32)
        poses = np.tile(ident.reshape(1, 1, 16), (a.candidates, 1, 1))
        guesses = np.tile(ident.reshape(1, 4, 4), (a.candidates, 1, 1))
        out["guessed"] = {}
        for est, name in ((1, "point_to_plane"), (0, "point_to_point")):       # (secondary_icp left its 25 + 1 keyframes in the store)
            pp = eng.icp_default_params(); pp.max_iterations = 30; pp.estimator = est; pp.normal_radius = 1.0

            def plain():
                return eng.loop_icp_batch_from_store(0, a.candidates, ident, keys, 0, poses, 0.05, pp)

            def guessed():
                return eng.loop_icp_batch_from_store_guess(0, a.candidates, ident, keys, 0, poses, 0.05, guesses, pp)

            def timed(f):
                t0 = time.perf_counter()
                r = f()
                return (time.perf_counter() - t0) * 1e3, r

            p0, g0 = plain(), guessed()
            equal = bool(np.array_equal(p0[0].view(np.uint32), g0[1].view(np.uint32)) and np.array_equal(p0[1].view(np.uint32), g0[2].view(np.uint32))
                         and np.array_equal(p0[3], g0[4]))
            tp, tg = [], []
            for _ in range(a.reps):
                tp.append(round(timed(plain)[0], 3))
                tg.append(round(timed(guessed)[0], 3))
            out["guessed"][name] = {"unguessed_ms": tp, "guessed_ms": tg, "bit_equal": equal, "iterations_mean": float(np.mean(p0[3])),
                                    "points_src": int(p0[4])}
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
