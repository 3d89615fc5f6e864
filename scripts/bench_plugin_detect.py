"""Detection timing of the vector plugins (M2DP, FPFH, GRSD) over a database filled from the wire: the single call and the batch
form (detect_*_many) at batch sizes 16 and 256, and the candidate lists (detect_*_topk) at k = 10 and 32 over the same batches, wall
microseconds per query as [min, median, max] over --reps repetitions.
scripts/bench_m2dp.py, bench_fpfh.py and bench_grsd.py take time_detect() from here; run alone it prints one JSON line per plugin
(--plugins).  --single-only: a library without the batch calls (an A/B against an older build); a library without the candidate lists is timed
without them.  The device time of
nn_l2_many_kernel comes from a separate `rocprofv3 --kernel-trace --stats` run of this script."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCHES = (16, 256)
TOPK = (10, 32)


def _range(xs):
    return [round(float(min(xs)), 2), round(float(np.median(xs)), 2), round(float(max(xs)), 2)]


def wire_rows(plugin, n, seed=1):
    rs = np.random.RandomState(seed)
    if plugin == "m2dp":
        rows = np.abs(rs.standard_normal((n, 192))).astype(np.float32)
        return rows / np.linalg.norm(rows, axis=1, keepdims=True)
    if plugin == "fpfh":
        return (100.0 * rs.dirichlet(np.full(11, 0.7), size=(n, 3)).reshape(n, 33)).astype(np.float32)
    return np.floor(rs.gamma(2.0, 1.0, size=(n, 21)) * 60.0).astype(np.float32)


def time_detect(det, form, keyframes, queries=200, reps=5, many=True):
    """det: an engine holding `keyframes` rows of one robot; form: "intra" or "inter".  {field: [min, median, max]} in us per query"""
    single, batched = getattr(det, "detect_" + form), getattr(det, f"detect_{form}_many", None)
    curs = {size: np.array([keyframes - 1 - (q % 100) for q in range(size)], np.int32) for size in BATCHES}
    for _ in range(10):
        single(keyframes - 1)
    out = {}
    us = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for q in range(queries):
            single(keyframes - 1 - (q % 100))
        us.append((time.perf_counter() - t0) / queries * 1e6)
    out[f"detect_{form}_us_per_query"] = _range(us)
    if not many:
        return out
    for size in BATCHES:
        calls = max(1, queries // size)
        for _ in range(3):
            batched(curs[size])
        us = []
        for _ in range(reps):
            t0 = time.perf_counter()
            for _ in range(calls):
                batched(curs[size])
            us.append((time.perf_counter() - t0) / (calls * size) * 1e6)
        out[f"detect_{form}_many_us_per_query_at_{size}"] = _range(us)
    topk = getattr(det, f"detect_{form}_topk", None)
    if topk is None:
        return out
    for k in TOPK:
        for size in BATCHES:
            calls = max(1, queries // size)
            for _ in range(3):
                topk(curs[size], k)
            us = []
            for _ in range(reps):
                t0 = time.perf_counter()
                for _ in range(calls):
                    topk(curs[size], k)
                us.append((time.perf_counter() - t0) / (calls * size) * 1e6)
            out[f"detect_{form}_topk{k}_us_per_query_at_{size}"] = _range(us)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plugins", default="m2dp,fpfh,grsd")
    ap.add_argument("--keyframes", type=int, default=10000)
    ap.add_argument("--queries", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--single-only", type=int, default=0)
    a = ap.parse_args()
    import scl_slam_amd
    for plugin in a.plugins.split(","):
        cls = {"m2dp": scl_slam_amd.M2dpEngine, "fpfh": scl_slam_amd.FpfhEngine, "grsd": getattr(scl_slam_amd, "GrsdEngine", None)}[plugin]
        det = cls(num_exclude_recent=30)
        rows = wire_rows(plugin, a.keyframes)
        for k in range(a.keyframes):
            det.save_from_wire(rows[k], 0, k)
        out = {"metric": f"{plugin}_detect_us_per_query", "keyframes": a.keyframes, "reps": a.reps, "queries_per_rep": a.queries,
               "range": "[min, median, max] over the repetitions"}
        for form in ("intra", "inter"):
            out.update(time_detect(det, form, a.keyframes, a.queries, a.reps, many=not a.single_only))
        print(json.dumps(out), flush=True)
        det.close()


if __name__ == "__main__":
    main()
