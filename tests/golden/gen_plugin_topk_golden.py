"""Generates tests/golden/plugin_topk_golden.json with the REFERENCE's own vendored nanoflann (oracle/_ref/libnanoflann_ref.so,
ref_nanoflann_knn: KDTreeVectorOfVectorsAdaptor, KNNResultSet<float>(k)) in the three row widths of the vector plugins -- 192
(M2DP), 33 (FPFH), 21 (GRSD) -- with k = 10: the order of a candidate list.

Run where oracle/_ref/libnanoflann_ref.so exists (oracle/Makefile compiles it from the reference tree):

    make -C oracle && python tests/golden/gen_plugin_topk_golden.py

Inputs are regenerated from seeds by ``golden_keys`` / ``golden_queries`` (the tests import them); only the outputs are stored.
Among exactly equal distances nanoflann's order depends on how it walks its tree, so a query whose first k + 1 sums hold a tie is
left out ("tie": true, no result stored); the generator asserts that this happens to at most 10 % of the queries of any case.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]    # tests/ and the repository root

K = 10
MAX_LEFT_OUT = 0.10
# name, row width, N keys, seed, n_queries
CASES = [
    ("m2dp_700", 192, 700, 41, 24),
    ("fpfh_3000", 33, 3000, 42, 24),
    ("grsd_900", 21, 900, 43, 24),
    ("fpfh_7", 33, 7, 44, 6),                    # fewer keys than k: found = 7
]


def golden_keys(dim, N, seed):
    """rows shaped like the plugins' descriptors, every row drawn on its own (no planted copies)"""
    rs = np.random.RandomState(seed)
    if dim == 192:                               # M2DP: six prototypes, every row with noise
        protos = np.abs(rs.standard_normal((6, 192))) * 0.1
        rows = protos[rs.randint(6, size=N)] + rs.standard_normal((N, 192)) * 0.01
    elif dim == 33:                              # FPFH: three 11-bin histograms of 100 votes each
        rows = (100.0 * rs.dirichlet(np.full(11, 0.7), size=(N, 3))).reshape(N, 33)
    else:                                        # GRSD: transition counts, whole numbers
        scale = np.array([400, 60, 30, 10, 20, 300] + [25] * 15, np.float64)
        rows = np.floor(rs.gamma(2.0, 1.0, size=(N, 21)) * scale)
    return np.ascontiguousarray(rows, np.float32)


def golden_queries(keys, seed, nq):
    """keys with a perturbation of a tenth of the columns' spread: the query is no key itself"""
    rs = np.random.RandomState(seed + 101)
    pick = rs.randint(0, keys.shape[0], size=nq)
    q = keys[pick].astype(np.float64) + 0.1 * keys.std(axis=0) * rs.standard_normal((nq, keys.shape[1]))
    return np.ascontiguousarray(q, dtype=np.float32)


def main():
    import oracle_binding as ob
    from plugin_cases import sq_dist_rows
    L = ob.load_ref_nanoflann()
    if L is None:
        raise SystemExit("oracle/_ref/libnanoflann_ref.so missing: run `make -C oracle` where the reference tree exists")
    out = {"generator": "tests/golden/gen_plugin_topk_golden.py", "k": K,
           "source": "reference include/nanoflann.hpp driven in 192, 33 and 21 dimensions, KNNResultSet<float>(10)", "cases": {}}
    for name, dim, N, seed, nq in CASES:
        keys = golden_keys(dim, N, seed)
        res, left_out = [], 0
        for q in golden_queries(keys, seed, nq):
            s = np.sort(sq_dist_rows(q, keys))[:K + 1]
            if np.unique(s).size != s.size:
                res.append({"tie": True}); left_out += 1
                continue
            idx, d2, found = ob.ref_knn(L, keys, q, K)
            res.append({"found": int(found), "idx": [int(x) for x in idx[:found]], "d2_bits": [int(x) for x in d2[:found].view(np.uint32)]})
        assert left_out <= MAX_LEFT_OUT * nq, (name, left_out, nq)
        out["cases"][name] = {"dim": dim, "N": N, "seed": seed, "nq": nq, "left_out": left_out, "results": res}
    with open(os.path.join(HERE, "plugin_topk_golden.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("wrote plugin_topk_golden.json with", len(CASES), "cases,", sum(c["left_out"] for c in out["cases"].values()), "queries left out")


if __name__ == "__main__":
    main()
