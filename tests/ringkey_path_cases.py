"""The cases of tests/test_gpu_ringkey_paths.py: key tables, ranges and queries that put the ring-key search on every path its
dispatch can take, and the path each case is meant to take -- restated here from the constants, so that a reviewer can check a
case against the sources without running anything.  tests/test_ringkey_path_cases.py pins all of it on the CPU checker alone.

The dispatch (ringkey_topk.hip, topk_merge.hpp, engine.hip's topk_enqueue_locked), n = hi - lo slots, k neighbours, R rings:
  1. n <= 256 * 256: ringkey_lists_kernel, 256 slots per workgroup, ceil(n / 256) lists;  more: ringkey_lists_chunked_kernel,
     1 024 slots per chunk, min(256, ceil(n / 1024)) lists, the workgroups stride over the chunks from 262 145 slots on
  2. R / 4 <= 16 and R % 4 == 0 (lists kernel only): the straight-line metric;  else ringkey_metric (always in the chunked kernel)
  3. k <= 8 (lists kernel only): DPP wave minima, the first wave ranks 4k keys;  else every thread counts the keys below its own
  4. lists * k <= 3 072: the threshold merge (topk_merge_pack_kernel);  more: topk_merge_rounds_kernel (+ topk_pack_kernel)
  5. distances wanted, k <= 16, a supported grid (20 x 60, 64 x 120): lists * k <= 1 024: sc_cand_exact merges the lists itself;
     more: launch_topk_merge (rule 4) first
  6. distances wanted, k > 16 (or another grid): merge (rule 4), launch_sc_distance, launch_topk_pack

Keys are planted the way test_gpu_topk.engine_with_ringkeys does (constant rows, S = 8).  A PLANTED neighbourhood is a cluster
of its own: centre c (every ring the same multiple of 8, far from the walk's 0 .. 12 and from every other centre), the query is the
centre, and the key of rank j is the centre with (j + 1) / 64 added to ring j % R -- squared distance ((j + 1) / 64)^2 exactly, so
the order of the planted slots is known by construction and the checker only confirms it."""
import functools
from collections import namedtuple

import numpy as np

# ---- the constants of the dispatch, restated (test_ringkey_path_cases.py compares them with the sources) ----
THREADS = 256            # kTopkThreads: slots per workgroup of ringkey_lists_kernel
MAX_BLOCKS = 256         # kTopkMaxBlocks
CHUNK = 1024             # kTopkChunk = kTopkThreads * kTopkPerThread
MAX_K = 64               # kTopkMaxK
MERGE_LDS = 3072         # kTopkMergeLds
CAND_MAX_KEYS = 1024     # kCandMergeMaxKeys
CAND_MAX_K = 16          # topk_enqueue_locked: k <= 16 goes to sc_cand_exact
DPP_MAX_K = 8            # ringkey_lists_kernel: k <= 8
STRAIGHT_MAX_GROUPS = 16
MAX_RINGS = 256          # scl_create: num_ring <= 256 (sq[256] in both scan kernels)
S_PLANT = 8
FLT_EPSILON = float(np.finfo(np.float32).eps)


def route(n, R, k, consumer="bare", grid_supported=False):
    """The path of one search over n slots.  consumer: "bare" (scl_ringkey_topk and the unfused detect_full) or "dist"
    (topk_with_distance, detect_intra, detect_inter)."""
    r = dict(scan=None, lists=0, metric=None, rank=None, merge=None, cand=None, tail=None)
    if n > 0:
        if n <= THREADS * MAX_BLOCKS:
            r["scan"], r["lists"] = "lists", (n + THREADS - 1) // THREADS
            r["metric"] = "straight" if (R // 4 <= STRAIGHT_MAX_GROUPS and R % 4 == 0) else "general"
            r["rank"] = "dpp" if k <= DPP_MAX_K else "count"
        else:
            chunks = (n + CHUNK - 1) // CHUNK
            r["scan"], r["lists"] = ("chunked-stride" if chunks > MAX_BLOCKS else "chunked"), min(chunks, MAX_BLOCKS)
            r["metric"] = "general"
    keys = r["lists"] * k
    merge = "threshold" if keys <= MERGE_LDS else "rounds"
    if consumer == "dist" and n > 0:
        if k <= CAND_MAX_K and grid_supported:
            r["cand"] = "cand-fused" if keys <= CAND_MAX_KEYS else "cand-merge-first"
            r["merge"] = None if r["cand"] == "cand-fused" else merge
        else:
            r["merge"], r["tail"] = merge, "dist-pack"
    else:
        r["merge"] = merge
    return r


def threshold_mq(L, k):
    """m, q of topk_merge_lists"""
    m = (k + L - 1) // L
    return m, (k + m - 1) // m


def walk_keys(N, R, seed):
    """a slow random walk reflected into 0 .. 12 (what golden_keys' "walk" draws, without its loop over N)"""
    rs = np.random.RandomState(seed)
    x = rs.uniform(0.5, 4.0, size=R) + np.cumsum(0.08 * rs.standard_normal((N, R)), axis=0)
    y = np.mod(x, 24.0)
    return np.ascontiguousarray(np.where(y > 12.0, 24.0 - y, y), dtype=np.float32)


def noisy(key, seed):
    return np.ascontiguousarray(key.astype(np.float64) + 0.05 * np.random.RandomState(seed).standard_normal(key.shape), dtype=np.float32)


class Planter:
    """plants clusters into a key table; no slot is planted twice"""

    def __init__(self, keys, first_centre=32.0, step=8.0):
        self.keys, self.used, self.centre, self.step = keys, np.zeros(keys.shape[0], bool), first_centre, step

    def take(self, a, b, count, seed=0):
        """up to `count` free slots of [a, b), spread, ascending"""
        free = np.flatnonzero(~self.used[a:b]) + a
        if free.size > count:
            free = np.sort(np.random.RandomState(seed + a).choice(free, size=count, replace=False))
        self.used[free] = True
        return [int(x) for x in free]

    def cluster(self, slots_by_rank):
        """slots_by_rank[j] becomes the j-th nearest key of the returned query"""
        R = self.keys.shape[1]
        assert len(slots_by_rank) <= MAX_K and len(set(slots_by_rank)) == len(slots_by_rank)
        centre = self.centre
        self.centre += self.step
        assert centre < 2048.0                            # (j + 1) / 64 stays exact beside the centre
        for j, s in enumerate(slots_by_rank):
            self.used[s] = True
            self.keys[s] = centre
            self.keys[s, j % R] = np.float32(centre + (j + 1) / 64.0)
        return np.full(R, centre, np.float32)


def interleave(a, b):
    """a[0], b[0], a[1], b[1], ... then what is left of the longer one"""
    out = []
    for i in range(max(len(a), len(b))):
        out += a[i:i + 1] + b[i:i + 1]
    return out


# id: names the path; db: which key table; queries: [("slot", i) | ("key", array) | ("planted", array: a cluster's centre)]; eps: the
# engine's knn_exclude_eps; prop(rel_idx, found, k): the placement, asserted on the CHECKER's indices (relative to lo) for the planted
# queries (every query: prop_all); why: the arithmetic that puts the case on its path
Case = namedtuple("Case", "id db lo hi ks queries eps consumer prop prop_all why")


def case(id, db, lo, hi, ks, queries, prop=None, why="", eps=0.0, consumer="bare", prop_all=False):
    assert prop is None or prop_all or any(kind == "planted" for kind, _ in queries)
    return Case(id, db, lo, hi, tuple(ks), queries, eps, consumer, prop, prop_all, why)


# =====================================================================================================================
# 1. range size: the two scan kernels and the stride.  R = 4: the smallest multiple of four (scl_create takes 1 .. 256)
# =====================================================================================================================
RANGE_R = 4
RANGE_N = 262144 + 1025
RANGE_SIZES = (65535, 65536, 65537, 66560, 66561, 262144, 262145, 263169)
RANGE_LOS = (0, 1023)
RANGE_KS = (1, 3, 8, 9, 64)


@functools.lru_cache(maxsize=None)
def range_world():
    keys = walk_keys(RANGE_N, RANGE_R, 11)
    pl = Planter(keys)
    cases = []
    for n in RANGE_SIZES:
        for lo in RANGE_LOS:
            hi = lo + n
            if hi > RANGE_N:
                continue                                   # 263 169 slots are the whole table: lo = 0 only
            rt = route(n, RANGE_R, 1)
            unit = THREADS if rt["scan"] == "lists" else CHUNK
            units = (n + unit - 1) // unit
            tag = f"{rt['scan']}-n{n}-lo{lo}"
            why = f"{n} slots: {units} x {unit}, {rt['lists']} lists"
            rs = np.random.RandomState(n + lo)
            cases.append(case(f"{tag}-random", "range", lo, hi, RANGE_KS,
                              [("slot", int(rs.randint(0, RANGE_N))), ("key", noisy(keys[int(rs.randint(lo, hi))], n + lo))], why=why))
            if rt["scan"] == "chunked-stride":
                # (c) workgroup w scans chunk w and chunk w + 256: the ranks alternate between the two, so the list srun that the
                # workgroup carries from its first chunk into its second decides the answer
                for w in range(units - MAX_BLOCKS):
                    a2 = lo + (w + MAX_BLOCKS) * CHUNK
                    second = pl.take(a2, min(a2 + CHUNK, hi), MAX_K // 2, seed=1)
                    if not second:
                        continue
                    first = pl.take(lo + w * CHUNK, lo + (w + 1) * CHUNK, MAX_K - len(second), seed=2)
                    q = pl.cluster(interleave(second, first))

                    def prop(rel, found, k, w=w):
                        chunks = {int(x) // CHUNK for x in rel[:found]}
                        return found == k and chunks == ({w + MAX_BLOCKS} if k == 1 else {w, w + MAX_BLOCKS})
                    cases.append(case(f"{tag}-wg{w}-split-over-its-two-chunks", "range", lo, hi, RANGE_KS, [("planted", q)], prop,
                                      why + f"; workgroup {w} has chunks {w} and {w + MAX_BLOCKS} ({min(a2 + CHUNK, hi) - a2} slots)"))
            # (b) the nearest keys in the last unit (chunk, or workgroup of the lists kernel), ragged unless n is a multiple
            a = lo + (units - 1) * unit
            last = pl.take(a, hi, MAX_K, seed=3)
            if last:
                before = pl.take(a - unit, a, MAX_K - len(last), seed=4)
                q = pl.cluster(last + before)

                def prop(rel, found, k, first_rel=a - lo, n_last=len(last)):
                    return found == k and all(int(x) >= first_rel for x in rel[:min(k, n_last)])
                cases.append(case(f"{tag}-nearest-in-last-{'chunk' if unit == CHUNK else 'workgroup'}", "range", lo, hi, RANGE_KS, [("planted", q)], prop,
                                  why + f"; the last one holds {hi - a} slots, {len(last)} of them planted"))
    return keys, cases


# =====================================================================================================================
# 2. ring counts off the fast path
# =====================================================================================================================
METRIC_RS = (1, 3, 4, 22, 60, 64, 68, 100, 130, 255, 256)
METRIC_N = 700                       # three workgroups
METRIC_KS = (3, 25)
METRIC_BIG = (68, 66000)             # the general metric inside the chunked kernel
METRIC_REFUSED_R = 257               # scl_create returns SCL_ERR_INVALID_ARG: nothing is allocated, nothing launches


@functools.lru_cache(maxsize=None)
def metric_world(R, N):
    keys = walk_keys(N, R, 1000 + R)
    rt = route(N, R, 3)
    tag = f"metric-{rt['metric']}-R{R}-{rt['scan']}-N{N}"
    why = f"R = {R}: {R // 4} ring groups, tail {R % 4}"
    rs = np.random.RandomState(R)
    cases = []
    for lo, hi in ((0, N), (17, N - 3)):
        cases.append(case(f"{tag}-lo{lo}", ("metric", R, N), lo, hi, METRIC_KS,
                          [("slot", int(rs.randint(0, N))), ("key", noisy(keys[int(rs.randint(lo, hi))], R + lo))], why=why))
    return keys, cases


def metric_worlds():
    return [(R, METRIC_N) for R in METRIC_RS] + [METRIC_BIG]


# =====================================================================================================================
# 3. both rank paths of the lists kernel with fewer valid keys than k
# =====================================================================================================================
SHORT_R = 20
SHORT_N = 1100
SHORT_SIZES = (0, 1, 2, 5, 63, 64, 65, 255, 256, 257, 513)
SHORT_KS = (1, 2, 7, 8, 9, 16, 64)
BLOCK = (513, 813)                   # 300 consecutive slots: copies of one key ("copies" table), inf / NaN keys ("holes" table)
TIE_SLOTS = (3, 77, 130, 200, 255) + tuple(range(256, 322, 2)) + (511,) + (512,)     # 5 + 34 + 1: workgroups 0, 1 and 2 of [0, 513)
TIE_CENTRE = 50.0


@functools.lru_cache(maxsize=None)
def short_world():
    """three tables: "short" (the plain walk), "copies" (300 copies of one key, searched with knn_exclude_eps = FLT_EPSILON),
    "holes" (300 keys of inf / NaN / -inf, and 40 slots at one and the same squared distance from TIE_CENTRE)"""
    plain = walk_keys(SHORT_N, SHORT_R, 33)
    copies = plain.copy()
    copies[BLOCK[0]:BLOCK[1]] = plain[600]
    holes = plain.copy()
    holes[BLOCK[0]:BLOCK[1]:3] = np.inf
    holes[BLOCK[0] + 1:BLOCK[1]:3] = np.nan
    holes[BLOCK[0] + 2:BLOCK[1]:3] = -np.inf
    assert len(TIE_SLOTS) == 40
    for j, s in enumerate(TIE_SLOTS):                       # +-1/4 on one ring: (1/4)^2 whatever the ring and the sign
        holes[s] = TIE_CENTRE
        holes[s, j % SHORT_R] = TIE_CENTRE + (0.25 if (j // SHORT_R) % 2 == 0 else -0.25)
    cases = []
    for n in SHORT_SIZES:
        lo = 300
        for name, ks in (("dpp", [k for k in SHORT_KS if k <= DPP_MAX_K]), ("count", [k for k in SHORT_KS if k > DPP_MAX_K])):
            cases.append(case(f"rank-{name}-n{n}" if n else f"empty-range-{name}", "short", lo, lo + n, ks,
                              [("slot", 5), ("key", noisy(plain[lo + n // 2], n))],
                              (lambda rel, found, k, n=n: found == min(k, n)),
                              f"{n} slots: {(n + 255) // 256} lists, the last with {n - (n - 1) // 256 * 256 if n else 0} keys", prop_all=True))
    for n in (257, 513):
        for k in SHORT_KS:
            for name, c in (("1-copy", 1), ("k-1-copies", k - 1), ("every-copy", min(n, BLOCK[1] - BLOCK[0]))):
                lo = BLOCK[0] + c - n                       # the range ends c slots into the block
                cases.append(case(f"rank-{'dpp' if k <= DPP_MAX_K else 'count'}-exclude-{name}-n{n}-k{k}", "copies", lo, lo + n, [k], [("slot", 600)],
                                  (lambda rel, found, k, n=n, c=c: found == min(k, n - c)),
                                  f"{n} slots, {c} of them copies of the query's key: {n - c} valid keys", eps=FLT_EPSILON, prop_all=True))
    # the block in FRONT of valid keys: [513, 1026) = a workgroup of holes, 44 holes + 212 keys, 1 key; [557, 814) = 256 holes, 1 key
    for lo, n, valid in ((BLOCK[0], 513, 213), (BLOCK[1] - 256, 257, 1)):
        for name, ks in (("dpp", [k for k in SHORT_KS if k <= DPP_MAX_K]), ("count", [k for k in SHORT_KS if k > DPP_MAX_K])):
            cases.append(case(f"rank-{name}-holes-first-list-empty-n{n}", "holes", lo, lo + n, ks, [("slot", 5), ("key", noisy(plain[900], n))],
                              (lambda rel, found, k, valid=valid: found == min(k, valid)), f"{n} slots, {n - valid} of them inf / NaN: {valid} valid keys", prop_all=True))
    for lo, n, ties in ((0, 513, 40), (256, 257, 35)):
        want = [s - lo for s in TIE_SLOTS if lo <= s < lo + n]
        assert len(want) == ties
        for name, ks in (("dpp", [k for k in SHORT_KS if k <= DPP_MAX_K]), ("count", [k for k in SHORT_KS if k > DPP_MAX_K])):
            cases.append(case(f"rank-{name}-{ties}-equal-distances-n{n}", "holes", lo, lo + n, ks, [("key", np.full(SHORT_R, TIE_CENTRE, np.float32))],
                              (lambda rel, found, k, want=want: found == k and [int(x) for x in rel[:min(k, len(want))]] == want[:k]),
                              f"{ties} slots at squared distance 1/16 over {(n + 255) // 256} workgroups: ascending index decides", prop_all=True))
    return dict(short=plain, copies=copies, holes=holes), cases


# =====================================================================================================================
# 4. the merges on both sides of 3 072 keys, and the threshold rule inside the first
# =====================================================================================================================
MERGE_R = 20
MERGE_N = 261200                     # 255 chunks and 80 slots: 256 lists from the chunked kernel
Z48 = 200000                         # 48 workgroups of holes with a few keys left: fewer than q lists have an m-th key
Z100 = Z48 + 48 * THREADS            # 100 workgroups of holes
MERGE_BOUNDS = ((64, 48), (64, 49), (25, 122), (25, 123), (13, 236), (13, 237))     # (k, lists): lists * k on both sides of 3 072
THRESHOLD_SHAPES = ((1, 64), (2, 64), (3, 64), (5, 64), (48, 64), (100, 25))        # (L, k): m = 64, 32, 22, 13, 2, 1
ROUNDS_L = 100                       # k = 64: 6 400 list entries, the loop over `base` runs 7 times
ALTERNATING = (64, 3)


def _lists_of(rel, found):
    return [int(x) // THREADS for x in rel[:found]]


@functools.lru_cache(maxsize=None)
def merge_world():
    keys = walk_keys(MERGE_N, MERGE_R, 44)
    keep = np.zeros(MERGE_N, bool)
    for j in range(2, 17):                                   # Z48: lists 2 .. 16 keep 5 keys, 17 .. 36 keep 1, the other 13 none
        keep[Z48 + j * THREADS + np.array([7, 60, 100, 180, 250])] = True
    for j in range(17, 37):
        keep[Z48 + j * THREADS + 33] = True
    for j in range(3, 23):                                   # Z100: lists 3 .. 22 keep 3 keys
        keep[Z100 + j * THREADS + np.array([1, 128, 255])] = True
    holes = np.arange(Z48, Z100 + 100 * THREADS)
    keys[holes[~keep[holes]]] = np.inf
    pl = Planter(keys)
    pl.used[Z48:Z100 + 100 * THREADS] = True
    cases = []
    lo_of = iter(range(37, 10 ** 6, 1531))

    def two_random(lo, hi, seed):
        rs = np.random.RandomState(seed)
        return [("slot", int(rs.randint(0, Z48))), ("key", noisy(keys[int(rs.randint(lo, min(hi, Z48)))], seed))]

    def first_and_last(lo, n, unit):
        units = (n + unit - 1) // unit
        a = lo + (units - 1) * unit
        return pl.cluster(interleave(pl.take(lo, lo + unit, MAX_K // 2, 5), pl.take(a, lo + n, MAX_K // 2, 6)))

    # -- both sides of 3 072, lists kernel and chunked kernel
    for k, L in MERGE_BOUNDS:
        lo, n = next(lo_of), (L - 1) * THREADS + (1 if L % 2 else THREADS)       # 12 288 / 12 289, 31 232 / 31 233, 60 416 / 60 417 slots
        rt = route(n, MERGE_R, k)
        assert rt["lists"] == L
        q = first_and_last(lo, n, THREADS)
        cases.append(case(f"{rt['merge']}-merge-k{k}-{L}-lists", "merge", lo, lo + n, [k], two_random(lo, lo + n, L) + [("planted", q)],
                          why=f"{n} slots = {L} lists x {k} = {L * k} keys"))
    for k in (12, 13):
        rt = route(MERGE_N, MERGE_R, k)
        assert rt["lists"] == MAX_BLOCKS and rt["scan"] == "chunked"
        q = first_and_last(0, MERGE_N, CHUNK)
        cases.append(case(f"chunked-{rt['merge']}-merge-k{k}-256-lists", "merge", 0, MERGE_N, [k], two_random(0, MERGE_N, k) + [("planted", q)],
                          why=f"{MERGE_N} slots = 256 chunks -> 256 lists x {k} = {256 * k} keys"))
    # -- the threshold rule: m = ceil(k / L) keys of each list, q = ceil(k / m) lists
    for L, k in THRESHOLD_SHAPES:
        m, q = threshold_mq(L, k)
        tag = f"threshold-L{L}-k{k}-m{m}"
        why = f"{L} lists x {k} = {L * k} keys, m = {m}, q = {q}"
        lo, n = next(lo_of), L * THREADS
        j = L // 2
        c = pl.cluster(pl.take(lo + j * THREADS, lo + (j + 1) * THREADS, k, 7))
        cases.append(case(f"{tag}-all-in-one-list", "merge", lo, lo + n, [k], [("planted", c)],
                          (lambda rel, found, k, j=j: found == k and set(_lists_of(rel, found)) == {j}), why))
        lo = next(lo_of)
        per = [pl.take(lo + i * THREADS, lo + (i + 1) * THREADS, m, 8) for i in range(q)]
        ranks = [per[r % q][r // q] for r in range(min(q * m, MAX_K))]
        c = pl.cluster(ranks)

        def prop(rel, found, k, m=m, q=q):
            ls = _lists_of(rel, found)
            return found == k and set(ls) == set(range(q)) and max(ls.count(i) for i in range(q)) == m
        cases.append(case(f"{tag}-m-in-each-of-the-first-q-lists", "merge", lo, lo + n, [k], [("planted", c)], prop, why))
        # fewer than q lists have an m-th key: tau is "no key" and every valid key is a candidate
        if L <= 5:
            lo = next(lo_of)
            n_short = (L - 1) * THREADS + (m - 1)                                  # the last list holds m - 1 keys
            per = [pl.take(lo + i * THREADS, min(lo + (i + 1) * THREADS, lo + n_short), m, 9) for i in range(L)]
            ranks = [per[r % L][r // L] for r in range(L * m) if r // L < len(per[r % L])][:MAX_K]
            c = pl.cluster(ranks)
            cases.append(case(f"{tag}-short-last-list-tau-is-no-key", "merge", lo, lo + n_short, [k], [("planted", c)],
                              (lambda rel, found, k, n_short=n_short: found == min(k, n_short)), why + f"; {n_short} slots: the last list has {m - 1} keys"))
        else:
            lo, valid, kept = (Z48, 95, Z48 + 2 * THREADS + 7) if L == 48 else (Z100, 60, Z100 + 3 * THREADS + 1)
            cases.append(case(f"{tag}-mostly-holes-tau-is-no-key", "merge", lo, lo + n, [k], [("slot", 5), ("key", noisy(keys[kept], L))],
                              (lambda rel, found, k, valid=valid: found == min(k, valid)), why + f"; holes but for {valid} keys, the first lists empty",
                              prop_all=True))
    # -- the rounds merge over seven passes of 1 024 entries, nearest keys in the first and the last block of lists
    lo, n = next(lo_of), ROUNDS_L * THREADS
    c = first_and_last(lo, n, THREADS)
    cases.append(case("rounds-merge-k64-100-lists-nearest-in-first-and-last-list", "merge", lo, lo + n, [64], two_random(lo, lo + n, 100) + [("planted", c)],
                      (lambda rel, found, k: found == k and set(_lists_of(rel, found)) == {0, ROUNDS_L - 1}),
                      f"{n} slots = 100 lists x 64 = 6 400 keys: ceil(6 400 / 1 024) = 7 passes of the loop over base"))
    return keys, cases


def rounds_case():
    return [c for c in merge_world()[1] if c.id.startswith("rounds-merge-k64-100-lists")][0]


# =====================================================================================================================
# 5. the consumers on a supported grid: 20 x 60, synth_descriptors
# =====================================================================================================================
GRID_R, GRID_S = 20, 60
GRID_N = 53000
CAND_BOUNDS = ((16, 64), (16, 65), (8, 128), (8, 129), (5, 204), (5, 205))         # (k, lists): lists * k on both sides of 1 024
DIST_PACK = ((17, 12289), (64, 12289), (17, 46081), (64, 52900))      # (k, slots): k > 16; 49 x 17 = 833, 49 x 64 = 3 136, 181 x 17 = 3 077, 207 x 64
DETECT_K = 16
DETECT_CURS = (16484, 16485)         # cur - 100 = 16 384 (64 lists) and 16 385 (65 lists)
FULL_RANGES = ((0, 40000), (20000, 20013))
FULL_KS = (4, 5)                     # kTailTop = 4: the fused epilogue;  5: the stand-alone scan on the second stream


def grid_cases():
    """(id, lo, hi, k) of the topk_with_distance calls"""
    out = []
    for k, L in CAND_BOUNDS:
        n = (L - 1) * THREADS + (1 if L % 2 else THREADS)                         # 16 384 / 16 385, 32 768 / 32 769, 52 224 / 52 225
        rt = route(n, GRID_R, k, "dist", True)
        assert rt["lists"] == L
        out.append((f"{rt['cand']}-k{k}-{L}-lists", 300, 300 + n, k))
    rt = route(GRID_N - 100, GRID_R, DETECT_K, "dist", True)                     # 207 lists x 16 = 3 312 keys: the rounds merge in front of the kernel
    out.append((f"{rt['cand']}-{rt['merge']}-merge-k{DETECT_K}-{rt['lists']}-lists", 0, GRID_N - 100, DETECT_K))
    for k, n in DIST_PACK:
        rt = route(n, GRID_R, k, "dist", True)
        out.append((f"{rt['merge']}-merge-{rt['tail']}-k{k}-n{n}", 0, n, k))
    return out


def all_routes():
    """every (route, id) of the file: the union the CPU test looks through for both sides of each rule"""
    out = []
    for c in range_world()[1] + short_world()[1] + merge_world()[1]:
        R = RANGE_R if c.db == "range" else SHORT_R
        out += [(route(c.hi - c.lo, R, k, c.consumer), c.id) for k in c.ks]
    for R, N in metric_worlds():
        for c in metric_world(R, N)[1]:
            out += [(route(c.hi - c.lo, R, k), c.id) for k in c.ks]
    out += [(route(hi - lo, GRID_R, k, "dist", True), id) for id, lo, hi, k in grid_cases()]
    out += [(route(cur - 100, GRID_R, DETECT_K, "dist", True), f"detect-{cur}") for cur in DETECT_CURS]
    out += [(route(hi - lo, GRID_R, 5), "full-5") for lo, hi in FULL_RANGES]
    return out
