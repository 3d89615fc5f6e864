"""The checker of the per-robot ranked searches (include/scl_engine.h, THE RANKED SEARCH PER ROBOT: scl_sc_search_intra,
scl_sc_search_inter): which keyframes a query may list, by the VALUE of each keyframe's (robot, index), and the list over such a
subset of a row of SC distances.  tests/test_sc_search_robot_cases.py pins it with hand-written rows; the GPU tests feed it the CPU
checker's rows (OracleDB.distance_batch).  Also the robot layout those tests share."""
import numpy as np

from sc_search_cases import NO_DIST

ANY_OTHER_ROBOT = -1          # SCL_SC_ANY_OTHER_ROBOT


def eligible(robots, indexs, cur, mode, robot_pre=ANY_OTHER_ROBOT, exclude=0):
    """The search set of query slot `cur` as a boolean array over the slots.  With (r, x) = (robots[cur], indexs[cur]):
    mode "intra": robot == r and index < x - exclude, the bound formed in 64 bits (Python integers);
    mode "inter", robot_pre == -1: robot != r;  robot_pre >= 0: robot == robot_pre (which must not be r).
    Slot order plays no part."""
    robots = np.asarray(robots).astype(np.int64)
    indexs = np.asarray(indexs).astype(np.int64)
    r, x = int(robots[cur]), int(indexs[cur])
    if mode == "intra":
        bound = x - int(exclude)                                          # a Python integer: no wrap-around
        return (robots == r) & np.array([int(v) < bound for v in indexs], dtype=bool)
    assert mode == "inter", mode
    if robot_pre == ANY_OTHER_ROBOT:
        return robots != r
    assert 0 <= robot_pre <= 127 and robot_pre != r, (robot_pre, r)
    return robots == robot_pre


def ranked_eligible(d, s, mask, k):
    """d[p], s[p]: fp64 distance and shift of the query against slot p; mask[p]: slot p is in the search set.  The list:
    (ids int32 [k], shifts int32 [k], dists float64 [k], n_found) -- the k smallest distances among the masked entries with d < 1e7
    (NaN fails that by itself), ascending by (distance, slot) through a stable sort; behind n_found: id -1, shift 0, distance 1e7."""
    d = np.asarray(d, dtype=np.float64)
    s = np.asarray(s, dtype=np.int32)
    pos = np.flatnonzero(np.asarray(mask, dtype=bool)[:d.size])
    with np.errstate(invalid="ignore"):
        pos = pos[d[pos] < NO_DIST]
    pos = pos[np.argsort(d[pos], kind="stable")][:k]
    ids = np.full(k, -1, dtype=np.int32); shifts = np.zeros(k, dtype=np.int32); dists = np.full(k, NO_DIST, dtype=np.float64)
    ids[:pos.size] = pos; shifts[:pos.size] = s[pos]; dists[:pos.size] = d[pos]
    return ids, shifts, dists, int(pos.size)


# ---- the layout of the GPU tests -------------------------------------------------------------------------------------------------------
TILE2 = (128, 192)            # one whole 64-slot tile of the selection: all robot 2
COPIES = (63, 64, 130)        # copies of the LAST keyframe's descriptor, on robots 0, 1, 2: both sides of a tile border
COPY_ROBOTS = (0, 1, 2)
ZERO_AT, NAN_AT = 20, 21      # an all-zero keyframe and one with a NaN cell, both robot 1
SWAP_AT, DUP_AT = 7, 9        # robot 0's 8th and 9th keyframes carry each other's index; robot 1's 10th repeats the 9th's index


def layout(n, seed=2024):
    """(robots int8 [n], indexs int32 [n]) of a database of n slots: robots 0, 1, 2 in runs of 1-5 slots, the planted slots above
    forced, every robot's indexes counting up in slot order but for one swapped pair (robot 0) and one duplicate (robot 1)."""
    rng = np.random.default_rng(seed)
    robots = np.empty(n, dtype=np.int8)
    p, last = 0, -1
    while p < n:
        r = int(rng.integers(0, 3))
        if r == last:
            r = (r + 1 + int(rng.integers(0, 2))) % 3
        run = int(rng.integers(1, 6))
        robots[p:p + run] = r
        p += run; last = r
    robots[TILE2[0]:TILE2[1]] = 2
    for q, r in zip(COPIES, COPY_ROBOTS):
        if q < n:
            robots[q] = r
    for q in (ZERO_AT, NAN_AT):
        if q < n:
            robots[q] = 1
    indexs = np.zeros(n, dtype=np.int32)
    for r in range(3):
        own = np.flatnonzero(robots == r)
        indexs[own] = np.arange(own.size)
    zero, one = np.flatnonzero(robots == 0), np.flatnonzero(robots == 1)
    if zero.size > SWAP_AT + 1:
        a, b = zero[SWAP_AT], zero[SWAP_AT + 1]
        indexs[a], indexs[b] = indexs[b], indexs[a]
    if one.size > DUP_AT:
        indexs[one[DUP_AT]] = indexs[one[DUP_AT - 1]]
    return robots, indexs
