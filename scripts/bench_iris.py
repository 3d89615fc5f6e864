"""LiDAR-Iris plugin timing at the defaults (80 x 360, 4 scales, compare()'s windows, 10 candidates): the single calls against the
batch forms, wall microseconds per keyframe / query as [min, median, max] over --reps repetitions, one JSON line.

  make_and_save singles against make_and_save_many at 16 and 256 scans (scans of --points points, a fresh engine per repetition);
  save_from_wire singles against save_from_wire_many at 16 and 256 vectors;
  detect_intra singles against detect_intra_many at 16 and 256 queries over a database of --keyframes keyframes.

The single calls timed here are the code the batch forms are compared with in tests/test_gpu_iris_batch.py.  Device times per kernel
come from a separate `rocprofv3 --kernel-trace --stats` run of this script."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCHES = (16, 256)


def _range(xs):
    return [round(float(min(xs)), 2), round(float(np.median(xs)), 2), round(float(max(xs)), 2)]


def _timed(fn, per):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) / per * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=2000)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--single-queries", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from scl_slam_amd.iris import IrisEngine
    from scl_slam_amd.synth import synth_scan
    rows, cols = 80, 360
    out = {"metric": "iris_plugin_us_per_keyframe", "keyframes": a.keyframes, "points": a.points, "reps": a.reps,
           "range": "[min, median, max] over the repetitions"}
    clouds = [synth_scan(a.points, seed=100 + k, max_range=85.0) for k in range(max(BATCHES))]
    warm = IrisEngine()
    wires = np.stack([warm.make_and_save(c, 0, k) for k, c in enumerate(clouds)])
    warm.make_and_save_many(clouds[:16], want_values=False)
    warm.save_from_wire_many(wires[:16])
    warm.close()

    # builders and wire ingest: a fresh engine per repetition, the timed region is the calls alone
    build = {"make_and_save_us": [], "save_from_wire_us": []}
    for size in BATCHES:
        build[f"make_and_save_many_us_at_{size}"] = []; build[f"save_from_wire_many_us_at_{size}"] = []
    for _ in range(a.reps):
        e = IrisEngine()
        build["make_and_save_us"].append(_timed(lambda: [e.make_and_save(c, 0, k) for k, c in enumerate(clouds[:64])], 64))
        e.close(); e = IrisEngine()
        build["save_from_wire_us"].append(_timed(lambda: [e.save_from_wire(wires[k], 0, k) for k in range(64)], 64))
        e.close()
        for size in BATCHES:
            calls = max(BATCHES) // size
            e = IrisEngine()
            build[f"make_and_save_many_us_at_{size}"].append(
                _timed(lambda: [e.make_and_save_many(clouds[c * size:(c + 1) * size]) for c in range(calls)], calls * size))
            e.close(); e = IrisEngine()
            build[f"save_from_wire_many_us_at_{size}"].append(
                _timed(lambda: [e.save_from_wire_many(wires[c * size:(c + 1) * size]) for c in range(calls)], calls * size))
            e.close()
    out.update({k: _range(v) for k, v in build.items()})

    # detection over a database of drawn images (a third of the cells seen) under smooth drawn row keys
    rs = np.random.RandomState(7)
    det = IrisEngine()
    per = rows * cols + rows
    for s in range(0, a.keyframes, 250):
        n = min(250, a.keyframes - s)
        v = np.empty((n, per), np.float32)
        v[:, :rows * cols] = rs.randint(1, 256, (n, rows * cols)) * (rs.rand(n, rows * cols) < 0.33)
        v[:, rows * cols:] = rs.uniform(0.0, 2.0, (n, rows))
        det.save_from_wire_many(v, indexs=np.arange(s, s + n))
    last = a.keyframes - 1
    for q in range(3):
        det.detect_intra(last - q)
    out["detect_intra_us_per_query"] = _range(
        [_timed(lambda: [det.detect_intra(last - (q % 100)) for q in range(a.single_queries)], a.single_queries) for _ in range(a.reps)])
    for size in BATCHES:
        curs = np.array([last - (q % 100) for q in range(size)], np.int32)
        det.detect_intra_many(curs[:16])
        out[f"detect_intra_many_us_per_query_at_{size}"] = _range([_timed(lambda: det.detect_intra_many(curs), size) for _ in range(a.reps)])
    det.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
