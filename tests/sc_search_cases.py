"""The checker of the ranked search (include/scl_engine.h, THE RANKED SEARCH): from a row of SC distances and shifts, the list
scl_sc_search_range must return.  tests/test_sc_search_cases.py pins it with hand-written rows; the GPU tests feed it the CPU
checker's rows (OracleDB.distance_batch) and the engine's own (sc_distance_matrix)."""
import numpy as np

NO_DIST = 10000000.0          # the engine's "no winner" distance: a pair is listed only below it


def ranked(d, s, lo, hi, k, base=0):
    """d[p], s[p]: fp64 distance and shift of the query against keyframe base + p.  The list over the keyframes lo .. hi-1:
    (ids int32 [k], shifts int32 [k], dists float64 [k], n_found) -- the k smallest distances among the entries with d < 1e7 (NaN
    fails that by itself), ascending by (distance, position) through a stable sort, so that equal distances (-0.0 and 0.0 too) keep
    their position order; behind n_found: id -1, shift 0, distance 1e7."""
    d = np.asarray(d, dtype=np.float64)
    s = np.asarray(s, dtype=np.int32)
    pos = np.arange(max(lo - base, 0), max(hi - base, 0))
    with np.errstate(invalid="ignore"):
        pos = pos[d[pos] < NO_DIST]
    pos = pos[np.argsort(d[pos], kind="stable")][:k]
    ids = np.full(k, -1, dtype=np.int32); shifts = np.zeros(k, dtype=np.int32); dists = np.full(k, NO_DIST, dtype=np.float64)
    ids[:pos.size] = base + pos; shifts[:pos.size] = s[pos]; dists[:pos.size] = d[pos]
    return ids, shifts, dists, int(pos.size)


def assert_lists_equal(got, want, what=""):
    """bit for bit: ids and shifts equal, the doubles by their uint64 views, n_found equal"""
    g_ids, g_shifts, g_dists, g_found = got
    w_ids, w_shifts, w_dists, w_found = want
    assert int(g_found) == int(w_found), f"{what}: n_found {g_found} != {w_found}"
    assert np.array_equal(np.asarray(g_ids), w_ids), f"{what}: ids {g_ids} != {w_ids}"
    assert np.array_equal(np.asarray(g_shifts), w_shifts), f"{what}: shifts {g_shifts} != {w_shifts}"
    assert np.array_equal(np.ascontiguousarray(g_dists).view(np.uint64), np.ascontiguousarray(w_dists).view(np.uint64)), f"{what}: dists {g_dists} != {w_dists}"
