"""Generates tests/golden/fpfh_nn_golden.json with the REFERENCE's own vendored nanoflann in 33 dimensions, k = 1, as the FPFH
inter detection builds it (descriptor.h:399-412: KDTreeVectorOfVectorsAdaptor(33, ..., 10), KNNResultSet<float>(1)).

Run where oracle/_ref/libnanoflann_ref.so exists (oracle/Makefile compiles it from the reference tree):

    make -C oracle && python tests/golden/gen_fpfh_nn_golden.py

Inputs are regenerated from seeds by ``golden_keys`` / ``golden_queries`` (the tests import them); only the outputs are stored.
33 = 8 * 4 + 1, so every distance goes through nanoflann's tail term.  The "near" cases plant queries whose two nearest keys
differ in the last bits of the distance; exact ties are left out (nanoflann's tie order depends on how it walks the tree).
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracle_binding as ob  # noqa: E402

DIM = 33
# name, N keys, seed, n_queries, kind
CASES = [
    ("hist_200", 200, 31, 12, "hist"),
    ("hist_3000", 3000, 32, 12, "hist"),
    ("near_400", 400, 33, 16, "near"),
    ("tiny_2", 2, 34, 3, "hist"),
]


def golden_keys(N, seed, kind):
    """FPFH-like keys: three 11-bin histograms of 100 votes each (float32)"""
    rs = np.random.RandomState(seed)
    keys = np.empty((N, DIM), np.float32)
    for i in range(N):
        for f in range(3):
            p = rs.dirichlet(np.full(11, 0.7))
            keys[i, 11 * f:11 * f + 11] = (100.0 * p).astype(np.float32)
    return keys


def golden_queries(keys, seed, nq, kind):
    rs = np.random.RandomState(seed + 101)
    pick = rs.randint(0, keys.shape[0], size=nq)
    if kind == "near":
        # halfway between two keys plus a tiny push towards the first: the two candidates differ by a few ulps of d2
        other = rs.randint(0, keys.shape[0], size=nq)
        mid = 0.5 * (keys[pick].astype(np.float64) + keys[other].astype(np.float64))
        q = mid + 1e-5 * (keys[pick].astype(np.float64) - keys[other].astype(np.float64))
    else:
        q = keys[pick].astype(np.float64) + 0.5 * rs.standard_normal((nq, DIM))
    return np.ascontiguousarray(q, dtype=np.float32)


def main():
    L = ob.load_ref_nanoflann()
    if L is None:
        raise SystemExit("oracle/_ref/libnanoflann_ref.so missing: run `make -C oracle` where the reference tree exists")
    out = {"generator": "tests/golden/gen_fpfh_nn_golden.py", "source": "reference include/nanoflann.hpp driven in 33 dimensions, k = 1 "
           "(descriptor.h:399-412)", "cases": {}}
    for name, N, seed, nq, kind in CASES:
        keys = golden_keys(N, seed, kind)
        queries = golden_queries(keys, seed, nq, kind)
        res = []
        for q in queries:
            idx, d2, found = ob.ref_knn(L, keys, q, 1)
            res.append({"idx": int(idx[0]), "d2_bits": int(d2[:1].view(np.uint32)[0])})
        out["cases"][name] = {"N": N, "seed": seed, "nq": nq, "kind": kind, "results": res}
    with open(os.path.join(HERE, "fpfh_nn_golden.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("wrote fpfh_nn_golden.json with", len(CASES), "cases")


if __name__ == "__main__":
    main()
