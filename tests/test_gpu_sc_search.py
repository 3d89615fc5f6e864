"""The ranked search of the Scan Context engine (include/scl_engine.h, THE RANKED SEARCH: scl_sc_search, scl_sc_search_range) on
the device against the checker of tests/sc_search_cases.py applied to the CPU checker's rows (OracleDB.distance_batch): every
comparison bit for bit -- ids and shifts equal, the doubles by their uint64 views.

One database per grid, built once and shared (20x60: the plain matrix path, 4 rows per launch; 64x120: the screened path with
sc_matrix, 16 rows; 80x180: its two lanes; 22x50: the generic kernel), with what a list must get right planted in it: copies of
one keyframe on both sides of a tile border (ties), all-zero keyframes and keyframes with a NaN or an inf cell (never listed or
listed as the checker says).  The checker's rows are computed once per (grid, query) and cached."""
import numpy as np
import pytest

import oracle_binding as ob
from sc_search_cases import NO_DIST, ranked, assert_lists_equal
from scl_slam_amd import ScanContextEngine, SclError
from scl_slam_amd.synth import synth_descriptors

pytestmark = pytest.mark.gpu

GRIDS = {"20x60": (20, 60, 300), "64x120": (64, 120, 260), "80x180": (80, 180, 60), "22x50": (22, 50, 40)}
EXCLUDE = 10                      # num_exclude_recent of every engine here: the small databases keep a search set
ZERO_A, NAN_AT, INF_AT, ZERO_B = 20, 21, 22, 23
COPIES = (10, 63, 64, 130)        # the keyframes that are copies of the last one (grids with more than 130 keyframes)
KS = (1, 2, 25, 32)


def make_descs(R, S, n, seed):
    descs = synth_descriptors(n, R, S, seed=seed, revisit_frac=0.05)
    descs[ZERO_A] = 0.0; descs[ZERO_B] = 0.0
    descs[NAN_AT][1, 2] = np.nan
    descs[INF_AT][2, 3] = np.inf
    if n > COPIES[-1]:
        for p in COPIES:
            descs[p] = descs[n - 1]
    return descs


class World:
    """a grid's database on the engine and in the CPU checker; the checker also holds the staged query as keyframe n"""

    def __init__(self, name):
        self.R, self.S, self.n = GRIDS[name]
        self.descs = make_descs(self.R, self.S, self.n, seed=500 + self.R)
        self.ext = synth_descriptors(1, self.R, self.S, seed=993)[0]
        self.eng = self.engine()
        self.eng.stage_query(self.ext)
        self.db = ob.OracleDB(ob.make_config(R=self.R, S=self.S))
        self.db.save_bulk(self.descs); self.db.save_bulk(self.ext[None])
        self._rows = {}

    def engine(self, **kw):
        eng = ScanContextEngine(num_ring=self.R, num_sector=self.S, num_exclude_recent=EXCLUDE, initial_capacity=64, **kw)
        eng.save_bulk(self.descs)
        return eng

    def row(self, q):
        """the checker's distances and shifts of query q (-1: the staged one) against the keyframes 0 .. n-1"""
        q = self.n if q < 0 else int(q)
        if q not in self._rows:
            with np.errstate(all="ignore"):
                self._rows[q] = self.db.distance_batch(q, n=self.n, fast=True)
        return self._rows[q]

    def expect(self, q, lo, hi, k):
        d, s = self.row(q)
        return ranked(d, s, lo, hi, k)

    def check(self, queries, lo, hi, k, what):
        """one sc_search_range call against the checker, list by list; returns the engine's answer"""
        queries = np.asarray(queries, dtype=np.int32)
        lo = np.broadcast_to(np.asarray(lo, dtype=np.int32), queries.shape); hi = np.broadcast_to(np.asarray(hi, dtype=np.int32), queries.shape)
        got = self.eng.sc_search_range(queries, lo, hi, k)
        assert got[0].shape == got[1].shape == got[2].shape == (len(queries), k) and got[3].shape == (len(queries),)
        for i, q in enumerate(queries):
            assert_lists_equal((got[0][i], got[1][i], got[2][i], got[3][i]), self.expect(q, int(lo[i]), int(hi[i]), k),
                               f"{what}: query {q} over [{lo[i]}, {hi[i]}) at k = {k}")
        return got

    def close(self):
        self.eng.close(); self.db.close()


@pytest.fixture(scope="module")
def worlds():
    made = {}

    def get(name):
        if name not in made:
            made[name] = World(name)
        return made[name]

    yield get
    for w in made.values():
        w.close()


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("grid", list(GRIDS))
def test_set_sizes_and_per_query_ranges(worlds, grid, k):
    """Ranges of 0, 1, k-1, k, k+1, 63, 64, 65 and 255-257 keyframes (those the database holds), every one at its own place, in ONE
    call with full ranges and empty ones between them and a staged query: 19 queries and more, so that every path runs several
    groups (two on the screened grids) whose matrices cover the union of their queries' ranges."""
    w = worlds(grid)
    n = w.n
    lengths = sorted({m for m in (0, 1, k - 1, k, k + 1, 63, 64, 65, 255, 256, 257) if 0 <= m <= n})
    pool = [n - 1, 0, n // 2, -1, n - 2, 7]
    queries, lo, hi = [], [], []
    for j, m in enumerate(lengths):
        queries.append(pool[j % len(pool)]); lo.append((11 * j + 3) % (n - m + 1)); hi.append(lo[-1] + m)
    for j in range(max(8, 19 - len(queries))):                        # full ranges, an empty one in the middle of them, the ends
        queries.append(pool[(j + 2) % len(pool)]); lo.append((0, 0, n, 1, 0, n - 1, 0, 5)[j % 8]); hi.append((n, n, n, n - 1, n, n, 0, 5)[j % 8])
    got = w.check(queries, lo, hi, k, grid)
    full = [i for i in range(len(queries)) if hi[i] - lo[i] == n]
    assert full and all(got[3][i] == min(k, int(np.sum(w.row(queries[i])[0] < NO_DIST))) for i in full)
    empty = [i for i in range(len(queries)) if hi[i] == lo[i]]
    assert len(empty) >= 2 and all(got[3][i] == 0 and (got[0][i] == -1).all() and (got[1][i] == 0).all() and (got[2][i] == NO_DIST).all() for i in empty)


def test_more_tiles_than_one_merge_round_and_growth_past_earlier_buffers():
    """20x60, 4 224 keyframes, k = 32: 66 tiles of 32 keys are more than the merge holds beside the best so far (2 048 - 32), so it
    runs two rounds.  The same engine searched first with 300 keyframes: the later search needs larger matrix halves, work buffers
    and database arrays than the earlier one left."""
    R, S, n, k = 20, 60, 4224, 32
    descs = synth_descriptors(n, R, S, seed=77, revisit_frac=0.02)
    descs[4000] = descs[n - 1]; descs[64] = descs[n - 1]               # equal distances 62 tiles apart
    eng = ScanContextEngine(num_ring=R, num_sector=S, num_exclude_recent=EXCLUDE, initial_capacity=64)
    db = ob.OracleDB(ob.make_config(R=R, S=S)); db.save_bulk(descs)
    eng.save_bulk(descs[:300])
    queries = np.array([299, 5, 150], dtype=np.int32)
    got = eng.sc_search_range(queries, 0, 300, k)
    for i, q in enumerate(queries):
        d, s = db.distance_batch(int(q), n=300, fast=True)
        assert_lists_equal((got[0][i], got[1][i], got[2][i], got[3][i]), ranked(d, s, 0, 300, k), f"300 keyframes, query {q}")
    eng.save_bulk(descs[300:])
    queries = np.array([n - 1, 0, 2111], dtype=np.int32)
    lo = np.array([0, 0, 1], dtype=np.int32); hi = np.array([n, n, n - 1], dtype=np.int32)
    got = eng.sc_search_range(queries, lo, hi, k)
    for i, q in enumerate(queries):
        d, s = db.distance_batch(int(q), n=n, fast=True)
        want = ranked(d, s, int(lo[i]), int(hi[i]), k)
        assert want[3] == k
        assert_lists_equal((got[0][i], got[1][i], got[2][i], got[3][i]), want, f"{n} keyframes, query {q}")
    assert got[0][0][:3].tolist() == [64, 4000, n - 1] and (got[2][0][:3] == got[2][0][0]).all()   # the copies, in position order
    eng.close(); db.close()


@pytest.mark.parametrize("grid", ["20x60", "64x120"])
def test_ties_go_to_the_lower_keyframe(worlds, grid):
    """Keyframes 10, 63, 64 and 130 are copies of the last keyframe, which is the query: the checker scores them exactly 0.0, and
    the list names them in position order whatever k cuts off and wherever the range starts."""
    w = worlds(grid)
    n = w.n
    d, s = w.row(n - 1)
    assert all(d[p] == 0.0 for p in COPIES + (n - 1,)), d[list(COPIES)]
    for k in (1, 2, 3, 4, 5, 25):
        want = w.expect(n - 1, 0, n, k)
        if k >= 3:
            assert np.sum(want[2] == want[2][0]) >= 3                  # the expected list itself holds the tie
        got = w.check([n - 1], 0, n, k, grid)
        assert got[0][0][:min(k, 5)].tolist() == [10, 63, 64, 130, n - 1][:k] and (got[2][0][:min(k, 5)] == 0.0).all()
    got = w.check([n - 1, n - 1, n - 1], [63, 64, 11], [n, 131, 130], 4, grid)
    assert got[0][0].tolist() == [63, 64, 130, n - 1] and got[0][1][:2].tolist() == [64, 130] and got[0][2][:2].tolist() == [63, 64]


@pytest.mark.parametrize("grid", list(GRIDS))
def test_unlisted_pairs_and_short_lists(worlds, grid):
    """All-zero keyframes score exactly 1e7 in the checker and are never listed; a keyframe with a NaN or an inf cell is listed
    only where the checker's distance is below 1e7.  A range with fewer listable pairs than k: n_found < k and the fillers."""
    w = worlds(grid)
    n, k = w.n, 5
    lo, hi = ZERO_A - 1, ZERO_B + 2                                        # six keyframes, two of them all-zero
    for q in (n - 1, 0, -1, NAN_AT, INF_AT, ZERO_A):
        d, s = w.row(q)
        assert d[ZERO_A] == NO_DIST and d[ZERO_B] == NO_DIST and s[ZERO_A] == 0
        listable = int(np.sum(d[lo:hi] < NO_DIST))
        assert listable < k
        got = w.check([q], lo, hi, k, grid)
        assert got[3][0] == listable < k
        assert (got[0][0][listable:] == -1).all() and (got[1][0][listable:] == 0).all() and (got[2][0][listable:] == NO_DIST).all()
        assert ZERO_A not in got[0][0] and ZERO_B not in got[0][0]
        assert not np.isnan(got[2][0]).any() and (got[2][0][:listable] < NO_DIST).all()
    # the all-zero keyframe as the query lists nothing at all
    got = w.check([ZERO_A], 0, n, 32, grid)
    assert got[3][0] == 0


@pytest.mark.parametrize("grid", list(GRIDS))
def test_cross_checks_on_the_device(worlds, grid):
    """Entry 0 is detect_full_range's winner; every list is the checker's selection from sc_distance_matrix's own row; sc_search is
    sc_search_range over [0, cur - num_exclude_recent).  (The full-database passes come first: on the screened grids a
    sc_distance_matrix call leaves its screening minima in the buffer sets it used, and a full-database pass through those sets
    then selects against them -- which is why a search puts them back, test_full_database_passes_after_searches.)"""
    w = worlds(grid)
    n, eng = w.n, w.eng
    queries = np.array([n - 1, n // 2, 3, -1, n - 2], dtype=np.int32)
    lo = np.array([0, 2, 0, 1, ZERO_A], dtype=np.int32); hi = np.array([n, n - 3, n, n, ZERO_A + 1], dtype=np.int32)
    lists = {k: eng.sc_search_range(queries, lo, hi, k) for k in (1, 7)}
    for k, (ids, shifts, dists, found) in lists.items():
        for i, q in enumerate(queries):
            nn, sh, d = eng.detect_full_range(int(q), int(lo[i]), int(hi[i]))
            assert (nn, sh) == (ids[i][0], shifts[i][0]) and np.float64(d).view(np.uint64) == dists[i][:1].view(np.uint64)[0], (grid, q)
    for k, (ids, shifts, dists, found) in lists.items():
        for i, q in enumerate(queries):
            dm, sm = eng.sc_distance_matrix([int(q)], int(lo[i]), int(hi[i]))
            assert_lists_equal((ids[i], shifts[i], dists[i], found[i]), ranked(dm[0], sm[0], int(lo[i]), int(hi[i]), k, base=int(lo[i])), f"{grid}: matrix row of {q}")
    assert ids[4][0] == -1 and found[4] == 0                              # (the one keyframe of that range is all-zero)
    curs = np.array([n - 1, EXCLUDE + 1, EXCLUDE, 0, n // 2, EXCLUDE + 2], dtype=np.int32)
    for k in (1, 25):
        a = eng.sc_search(curs, k)
        b = eng.sc_search_range(curs, 0, np.maximum(curs - EXCLUDE, 0), k)
        for x, y in zip(a, b):
            assert np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x, y.view(np.uint64) if y.dtype == np.float64 else y)
        assert a[3][2] == 0 and a[3][3] == 0 and a[3][1] <= 1            # empty search sets, and one of keyframe 0 alone
        for i, cur in enumerate(curs):
            assert_lists_equal((a[0][i], a[1][i], a[2][i], a[3][i]), w.expect(cur, 0, max(int(cur) - EXCLUDE, 0), k), f"{grid}: sc_search {cur}")


def _sentinels(nq, k):
    return (np.full((nq, max(k, 1)), -7, dtype=np.int32), np.full((nq, max(k, 1)), -7, dtype=np.int32), np.full((nq, max(k, 1)), -7.0), np.full(nq, -7, dtype=np.int32))


@pytest.mark.parametrize("grid", list(GRIDS))
def test_searches_leave_no_trace_and_errors_write_nothing(worlds, grid):
    """Two fresh engines go through the same sequence of sc_distance_matrix, detect_intra and detect_inter calls (detect_inter keeps
    the periodic tree's counter) twice; one of them searches in between -- and fails in every way a search can.  Their answers
    agree call by call."""
    w = worlds(grid)
    n = w.n
    a, b = w.engine(tree_making_period=3), w.engine(tree_making_period=3)
    curs = [n - 1, n // 2, EXCLUDE + 3, n - 2, n - 3]

    def answers(eng):
        out = [eng.sc_distance_matrix([n - 1, 2], 1, n - 1)]
        out += [eng.detect_intra(c) for c in curs] + [eng.detect_inter(c) for c in curs] + [eng.detect_full(c) for c in curs[:2]]
        return out

    def same(x, y):
        if isinstance(x, tuple):
            return len(x) == len(y) and all(same(p, q) for p, q in zip(x, y))
        x, y = np.asarray(x), np.asarray(y)
        if x.dtype.kind == "f":
            x, y = x.astype(np.float64).view(np.uint64), y.astype(np.float64).view(np.uint64)
        return np.array_equal(x, y)

    first_a, first_b = answers(a), answers(b)
    assert all(same(x, y) for x, y in zip(first_a, first_b))
    for k in (1, 25, 32):
        got = a.sc_search(np.arange(n - 1, n - 20, -1), k)
        want = w.expect(n - 1, 0, n - 1 - EXCLUDE, k)
        assert_lists_equal((got[0][0], got[1][0], got[2][0], got[3][0]), want, f"{grid}: fresh engine")
        a.sc_search_range([n - 1, 0, 5], [0, 3, 2], [n, n - 2, 2], k)
    # errors: status, and the sentinel-filled arrays as they were
    with pytest.raises(SclError) as ei:                                  # nothing staged on this engine
        a.sc_search_range([n - 1, -1], 0, n, 3, out=_sentinels(2, 3))
    assert ei.value.status == -1
    for args, status in ((([n - 1, 0], 0, n, 0), -1), (([n - 1, 0], 0, n, 33), -1), (([0, n], 0, n, 3), -4), (([0, 1], 0, [n, n + 1], 3), -4),
                         (([0, 1], [0, 5], [n, 4], 3), -4), (([0, 1], [-1, 0], n, 3), -4), (([0, -400000], 0, n, 3), -4)):
        out = _sentinels(2, args[3])
        with pytest.raises(SclError) as ei:
            a.sc_search_range(*args, out=out)
        assert ei.value.status == status, args
        assert (out[0] == -7).all() and (out[1] == -7).all() and (out[2] == -7.0).all() and (out[3] == -7).all(), args
    for curs_bad, k, status in (([n - 1, n], 3, -4), ([n - 1, -1], 3, -4), ([n - 1], 0, -1), ([n - 1], 33, -1)):
        out = _sentinels(len(curs_bad), k)
        with pytest.raises(SclError) as ei:
            a.sc_search(curs_bad, k, out=out)
        assert ei.value.status == status, (curs_bad, k)
        assert (out[0] == -7).all() and (out[1] == -7).all() and (out[2] == -7.0).all() and (out[3] == -7).all()
    assert a.sc_search([], 5)[0].shape == (0, 5) and a.sc_search_range([], 0, 0, 5)[3].shape == (0,)
    second_a, second_b = answers(a), answers(b)
    assert all(same(x, y) for x, y in zip(second_a, second_b))
    a.close(); b.close()


@pytest.mark.parametrize("grid", list(GRIDS))
def test_full_database_passes_after_searches(worlds, grid):
    """A search runs the screening launches of the screened grids, which leave every row's smallest screened distance in its buffer
    set; the full-database passes select their survivors against that word.  After searches whose queries have smaller minima than
    the passes that follow (full ranges, then ranges that leave the best keyframes out), detect_full, detect_full_range and
    detect_full_stream answer what a twin engine that never searched answers, and what the checker's row says."""
    w = worlds(grid)
    n = w.n
    a, b = w.engine(), w.engine()
    a.stage_query(w.ext); b.stage_query(w.ext)
    passes = [(-1, 1, n), (-1, ZERO_B + 1, n), (n - 1, 0, n - 1), (n - 1, 11, min(63, n - 1)), (n // 2, 0, n // 2), (0, 1, n), (3, ZERO_B + 1, n - 2)]
    for k in (1, 25):
        a.sc_search_range([q for q, _, _ in passes] + [n - 2] * 12, 0, n, k)        # 19 rows over the whole database: every buffer set a pass may take
        for q, lo, hi in passes:
            got, twin = a.detect_full_range(q, lo, hi), b.detect_full_range(q, lo, hi)
            want = w.expect(q, lo, hi, 1)
            assert got[:2] == twin[:2] == (want[0][0], want[1][0]) and np.float64(got[2]).view(np.uint64) == np.float64(twin[2]).view(np.uint64) == want[2].view(np.uint64)[0], (grid, q, lo, hi)
        a.sc_search(np.arange(n - 1, n - 18, -1), k)
        qs = np.array([q for q, _, _ in passes[2:]], dtype=np.int32); los = np.array([l for _, l, _ in passes[2:]], dtype=np.int32); his = np.array([h for _, _, h in passes[2:]], dtype=np.int32)
        x, y = a.detect_full_stream(qs, los, his, 16, 2), b.detect_full_stream(qs, los, his, 16, 2)
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and np.array_equal(x[2].view(np.uint64), y[2].view(np.uint64))
        assert a.detect_full(n - 1) == b.detect_full(n - 1)
    a.close(); b.close()


@pytest.mark.parametrize("G", [2, 3])
def test_sharded_lists_equal_the_single_engine(G):
    """One database over G shards (all on device 0, host merge): per query one search per shard over the shard's slots of the global
    range, merged by (distance, global key) -- the single engine's lists, bit for bit; ties between shards included."""
    R, S, n = 64, 120, 200
    descs = make_descs(R, S, n, seed=640)
    one = ScanContextEngine(num_ring=R, num_sector=S, num_exclude_recent=EXCLUDE, initial_capacity=64)
    sh = ScanContextEngine(num_ring=R, num_sector=S, num_exclude_recent=EXCLUDE, initial_capacity=64, devices=[0] * G, exchange=1)
    assert sh.shard_info() == (G, 1)
    one.save_bulk(descs); sh.save_bulk(descs)
    ext = synth_descriptors(1, R, S, seed=994)[0]
    one.stage_query(ext); sh.stage_query(ext)
    queries = np.array([n - 1, 0, 1, 2, n - 2, 100, -1, 57, n - 1], dtype=np.int32)     # the oldest and the newest keyframes of every shard
    lo = np.array([0, 0, 3, 0, 1, 99, 0, 57, 64], dtype=np.int32); hi = np.array([n, n, n - 4, 0, n, 102, n, 58, 131], dtype=np.int32)
    for k in (1, 4, 25, 32):
        a = one.sc_search_range(queries, lo, hi, k); b = sh.sc_search_range(queries, lo, hi, k)
        for i in range(len(queries)):
            assert_lists_equal((b[0][i], b[1][i], b[2][i], b[3][i]), (a[0][i], a[1][i], a[2][i], a[3][i]), f"G = {G}, k = {k}, query {queries[i]}")
    assert a[0][0][:5].tolist() == [10, 63, 64, 130, n - 1]
    curs = np.array([n - 1, EXCLUDE, 0, 150, EXCLUDE + G + 1], dtype=np.int32)
    a = one.sc_search(curs, 25); b = sh.sc_search(curs, 25)
    for i in range(len(curs)):
        assert_lists_equal((b[0][i], b[1][i], b[2][i], b[3][i]), (a[0][i], a[1][i], a[2][i], a[3][i]), f"G = {G}, sc_search {curs[i]}")
    for args, status in ((([0, n], 0, n, 3), -4), (([0, 1], 0, [n, n + 1], 3), -4), (([0, 1], 0, n, 33), -1)):
        out = _sentinels(2, 3)
        with pytest.raises(SclError) as ei:
            sh.sc_search_range(*args, out=out)
        assert ei.value.status == status and (out[0] == -7).all() and (out[3] == -7).all()
    one.close(); sh.close()


def test_sharded_query_that_has_left_the_mirror():
    """Every shard keeps the query-side rows of the newest 1 024 keyframes of the others; an older query keyframe is copied to a
    staging row of the shards that do not own it when it is asked for.  Two shards, 2 200 keyframes: old and recent queries in one
    call, over short ranges."""
    R, S, G, n = 64, 120, 2, 2200
    base = synth_descriptors(220, R, S, seed=641, revisit_frac=0.05)
    descs = np.concatenate([np.roll(base, 7 * j, axis=2) for j in range(10)])           # the same places under ten headings
    one = ScanContextEngine(num_ring=R, num_sector=S, num_exclude_recent=EXCLUDE, initial_capacity=256)
    sh = ScanContextEngine(num_ring=R, num_sector=S, num_exclude_recent=EXCLUDE, initial_capacity=256, devices=[0] * G, exchange=1)
    one.save_bulk(descs); sh.save_bulk(descs)
    queries = np.array([0, 1, 101, n - 1, n - 2, 151, 150, 1000], dtype=np.int32)   # keyframes below 152 have 1 024 newer ones on their shard
    lo = np.array([0, 90, 2000, 0, 30, 435, 1, 2100], dtype=np.int32); hi = lo + np.array([130, 129, 131, 64, 65, 10, 127, 100], dtype=np.int32)
    a = one.sc_search_range(queries, lo, hi, 25); b = sh.sc_search_range(queries, lo, hi, 25)
    for i in range(len(queries)):
        assert_lists_equal((b[0][i], b[1][i], b[2][i], b[3][i]), (a[0][i], a[1][i], a[2][i], a[3][i]), f"query {queries[i]}")
    assert (a[3] > 0).all()
    one.close(); sh.close()
