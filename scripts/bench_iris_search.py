"""LiDAR-Iris exhaustive ranked search benchmark (include/scl_iris.h "THE EXHAUSTIVE SEARCH"): prints one JSON line.

  At 80 x 360 (640 template rows, 20 words a column) and every --keyframes size: scl_iris_search_intra for one launch group of 16
  queries against the whole database, k = 32 -- wall time of the call around its one device synchronisation, [min, median, max] over
  --reps calls after --warmup; pairs per second; and the share of the integer-ALU ceiling.  A pair is cols * cols * words word steps
  (2.592 M); the compiled loop spends VALU_PER_STEP vector instructions on one (v_or, v_bitop3 for the xor and the and-not, two
  v_bcnt that add as they count), and the ceiling assumes one wave-wide vector instruction per SIMD every 4 cycles at 2.4 GHz on
  256 CUs x 4 SIMDs (MI355X_MICROARCH: vector-instruction issue cost of v_add-class operations).
  The yardstick is the only other route to the same answers: scl_iris_hamming_all_shifts(query, the whole set) for each of the 16
  queries, on the same handle and data, up to --yardstick-max keyframes.  The two routes' best candidates are compared.
  The images are random bytes at --fill density, stored from the wire: the kernels' work does not depend on the data.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VALU_PER_STEP = 4
CEILING_LANE_OPS = 256 * 4 * 16 * 2.4e9                     # lanes retired per second at one wave64 instruction per SIMD per 4 cycles


def spread(ts):
    ts = sorted(ts)
    return [round(ts[0] * 1e3, 3), round(ts[len(ts) // 2] * 1e3, 3), round(ts[-1] * 1e3, 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, nargs="+", default=[1000, 10000])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--yardstick-max", type=int, default=10000)
    ap.add_argument("--yardstick-reps", type=int, default=2)
    ap.add_argument("--fill", type=float, default=0.3)
    ap.add_argument("--k", type=int, default=32)
    a = ap.parse_args()
    from scl_slam_amd.iris import DETECT_GROUP, IrisEngine

    rows, cols = 80, 360
    eng = IrisEngine(rows=rows, cols=cols, num_exclude_recent=0, wire_decode=1)
    words = (eng.trows + 31) // 32
    steps_per_pair = cols * cols * words
    rs = np.random.RandomState(5)
    pool = np.zeros((250, rows * cols + rows), np.float32)
    pool[:, :rows * cols] = rs.randint(0, 256, (250, rows * cols)) * (rs.uniform(size=(250, rows * cols)) < a.fill)
    out = {"metric": "iris_search_ms_per_group_of_16", "rows": rows, "cols": cols, "k": a.k, "word_steps_per_pair": steps_per_pair,
           "valu_per_word_step": VALU_PER_STEP, "ceiling_lane_ops_per_s": CEILING_LANE_OPS, "sizes": {}}
    stored = 0
    for n in sorted(a.keyframes):
        while stored < n + DETECT_GROUP:                    # the queries are the 16 newest keyframes, each searching [0, its index)
            m = min(250, n + DETECT_GROUP - stored)
            eng.save_from_wire_many(pool[:m], indexs=np.arange(stored, stored + m))
            stored += m
        curs = np.arange(n, n + DETECT_GROUP, dtype=np.int32)
        for _ in range(a.warmup):
            got = eng.search_intra(curs, a.k)
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter(); eng.search_intra(curs, a.k); ts.append(time.perf_counter() - t0)
        pairs = float(sum(int(c) for c in curs))
        med = sorted(ts)[len(ts) // 2]
        res = {"search_ms": spread(ts), "pairs": pairs, "pairs_per_s": round(pairs / med, 1),
               "alu_ceiling_share": round(pairs / med * steps_per_pair * VALU_PER_STEP / CEILING_LANE_OPS, 4)}
        if n <= a.yardstick_max:
            def yard():
                return [eng.hamming_all_shifts(int(c), np.arange(int(c), dtype=np.int32)) for c in curs]
            eng.hamming_all_shifts(int(curs[0]), np.arange(64, dtype=np.int32))      # warm-up: code object, buffers
            ys = []
            for _ in range(a.yardstick_reps):
                t0 = time.perf_counter(); ref = yard(); ys.append(time.perf_counter() - t0)
            ymed = sorted(ys)[len(ys) // 2]
            agree = True
            for i, (d, b) in enumerate(ref):                # the first of the smallest scores against rank 0
                p = min((int(np.float32(x).view(np.uint32)), j) for j, x in enumerate(d) if not np.isnan(x))[1]
                agree &= bool(got[0][i, 0] == p and got[1][i, 0] == b[p] and np.float32(got[2][i, 0]).view(np.uint32) == np.float32(d[p]).view(np.uint32))
            res.update({"hamming_all_shifts_ms": spread(ys), "speedup": round(ymed / med, 2), "best_candidates_agree": agree})
        out["sizes"][str(n)] = res
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
