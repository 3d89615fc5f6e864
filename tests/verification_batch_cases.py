"""One received scan and a named list of candidate clouds for the batched geometric verification (numpy only; the single-candidate
inputs are tests/verification_cases.py's, whose helpers this builds on).

tests/test_verification_batch_cases.py pins the list on the CPU checker (oracle/icp_oracle.c), tests/test_gpu_verification_batch.py
holds scl_geometric_verification_batch(_from_store) to the single calls, bit for bit, and to the checker on it.  The list mixes
candidates that verify, candidates that fail in different ways (so that no two neighbours share their counts: a batch that hands
candidate c the answer of candidate c + 1 cannot pass), candidates on the edges of the reduction's partition and of the early
exits, and one candidate twice."""
import numpy as np

import verification_cases as vc
from scl_slam_amd.synth import rigid_transform, synth_structured_cloud

ITERATIONS = (1, 7, 8, 9, 257, 300)                                  # around kHypPerBlock = 8 and the pick kernel's 256-thread trip
THRESHOLD, RATIO, SEED = 0.25, 0.45, 3
N_NONFINITE = 5

_cache = {}


def _yawed(cloud, degrees):
    out = cloud.copy()
    out[:, :3] = (cloud[:, :3].astype(np.float64) @ rigid_transform(0.0, 0.0, np.radians(degrees), 0, 0, 0)[:3, :3].T).astype(np.float32)
    return out


def target():
    """the place the received scan was taken at: verification_cases' matching target"""
    if "target" not in _cache:
        _cache["target"] = synth_structured_cloud(4000, seed=31)
    return _cache["target"]


def source():
    """the received scan: verification_cases' matching source (every second target point, moved a little, 3 mm of noise) with
    N_NONFINITE rows made non-finite -> (cloud, those rows)"""
    if "source" not in _cache:
        T = rigid_transform(0.0, 0.0, 0.002, 0.02, -0.01, 0.0)
        _cache["source"] = vc.with_nonfinite(vc._moved_copy(target(), T, 2, 0.003, 1), N_NONFINITE)
    return _cache["source"]


def finite_source():
    """what the checker is run on (vc.CHECKER_ON_FINITE_ROWS: its four outputs on a cloud are those on the cloud's finite rows)"""
    src = source()[0]
    return src[np.isfinite(src[:, :3]).all(1)]


def candidates():
    """[(name, cloud)] in the order the batch takes them"""
    if "candidates" not in _cache:
        tgt = target()
        rs = np.random.RandomState(5)
        half = tgt.copy()
        half[::4, 0] += 60.0                                          # source i is target row 2 i: the partners of every second source
        cs = [("matching", tgt),
              ("permuted", tgt[rs.permutation(len(tgt))]),
              ("yaw_3", _yawed(tgt, 3.0)), ("yaw_20", _yawed(tgt, 20.0)), ("yaw_90", _yawed(tgt, 90.0)),
              ("other_place", synth_structured_cloud(3000, seed=77)),
              ("half_moved", half),
              ("first_257", tgt[:257]), ("first_256", tgt[:256]), ("first_3", tgt[:3]), ("first_1", tgt[:1]),
              ("empty", tgt[:0]),
              ("matching_again", tgt.copy())]
        _cache["candidates"] = [(n, np.ascontiguousarray(c)) for n, c in cs]
    return _cache["candidates"]


def names():
    return [n for n, _ in candidates()]


def clouds():
    return [c for _, c in candidates()]
