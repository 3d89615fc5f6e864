"""The per-robot ranked searches of the Scan Context engine (include/scl_engine.h, THE RANKED SEARCH PER ROBOT: scl_sc_search_intra,
scl_sc_search_inter) on the device against the checker of tests/sc_search_robot_cases.py applied to the CPU checker's rows
(OracleDB.distance_batch): every comparison bit for bit -- ids and shifts equal, the doubles by their uint64 views.

One database per grid, built once and shared (20x60: the plain matrix path, 4 rows per launch; 64x120: the screened path, 16 rows;
80x180: its two lanes; 22x50: the generic kernel), three robots interleaved as sc_search_robot_cases.layout says.  The checker's rows
are computed once per (grid, query) and cached."""
import numpy as np
import pytest

import oracle_binding as ob
from sc_search_cases import NO_DIST, assert_lists_equal
from sc_search_robot_cases import COPIES, DUP_AT, NAN_AT, SWAP_AT, TILE2, ZERO_AT, eligible, layout, ranked_eligible
from scl_slam_amd import ScanContextEngine, SclError
from scl_slam_amd.synth import rigid_transform, synth_descriptors, synth_scan

pytestmark = pytest.mark.gpu

GRIDS = {"20x60": (20, 60, 300), "64x120": (64, 120, 260), "80x180": (80, 180, 60), "22x50": (22, 50, 40)}
EXCLUDE = 10                      # num_exclude_recent of every engine here: the small databases keep a search set
KS = (1, 2, 25, 32)
INVALID_ARG, OUT_OF_RANGE = -1, -4


def make_descs(R, S, n, seed):
    descs = synth_descriptors(n, R, S, seed=seed, revisit_frac=0.05)
    descs[ZERO_AT] = 0.0
    descs[NAN_AT][1, 2] = np.nan
    if n > COPIES[-1]:
        for p in COPIES:
            descs[p] = descs[n - 1]
    return descs


def new_engine(R, S, descs, robots=None, indexs=None, **kw):
    eng = ScanContextEngine(num_ring=R, num_sector=S, num_exclude_recent=EXCLUDE, initial_capacity=64, **kw)
    if len(descs):
        eng.save_bulk(descs, robots, indexs)
    return eng


def row_of(got, i):
    return got[0][i], got[1][i], got[2][i], got[3][i]


def same_answer(a, b, what):
    for i in range(len(a[3])):
        assert_lists_equal(row_of(a, i), row_of(b, i), f"{what}: query {i}")


def mixed_queries(robots, indexs, count=19):
    """`count` query slots whose robots alternate 0, 1, 2, 0, ...: per robot its newest and its oldest keyframe (an empty intra set), the
    keyframes whose intra bound falls between the out-of-order pair and just behind the duplicate, then the rest from the newest on"""
    pools = []
    for r in range(3):
        own = np.flatnonzero(robots == r)
        first = [int(own[-1]), int(own[0])]
        for want in (SWAP_AT + 1 + EXCLUDE, DUP_AT + EXCLUDE):
            first += [int(s) for s in own[indexs[own] == want][:1] if int(s) not in first]
        pools.append(first + [int(s) for s in own[::-1] if int(s) not in first])
    out, i = [], 0
    while len(out) < count and i < 3 * len(robots):
        if i // 3 < len(pools[i % 3]):
            out.append(pools[i % 3][i // 3])
        i += 1
    return np.array(out, dtype=np.int32)


class World:
    """a grid's database on the engine and in the CPU checker"""

    def __init__(self, name):
        self.name = name
        self.R, self.S, self.n = GRIDS[name]
        self.descs = make_descs(self.R, self.S, self.n, seed=700 + self.R)
        self.robots, self.indexs = layout(self.n)
        self.eng = self.engine()
        self.db = ob.OracleDB(ob.make_config(R=self.R, S=self.S))
        self.db.save_bulk(self.descs)
        self._rows = {}

    def engine(self, **kw):
        return new_engine(self.R, self.S, self.descs, self.robots, self.indexs, **kw)

    def row(self, q):
        q = int(q)
        if q not in self._rows:
            with np.errstate(all="ignore"):
                self._rows[q] = self.db.distance_batch(q, n=self.n, fast=True)
        return self._rows[q]

    def expect(self, q, mode, robot_pre, k):
        d, s = self.row(q)
        return ranked_eligible(d, s, eligible(self.robots, self.indexs, int(q), mode, robot_pre, EXCLUDE), k)

    def searches(self, eng, queries, k):
        """every list the two calls give for `queries`: {(mode, robot_pre): (queries asked, answer)}; a named robot is asked by the
        queries of the other robots"""
        out = {("intra", None): (queries, eng.sc_search_intra(queries, k)), ("inter", -1): (queries, eng.sc_search_inter(queries, k))}
        for b in range(3):
            sub = queries[self.robots[queries] != b]
            out[("inter", b)] = (sub, eng.sc_search_inter(sub, k, robot_pre=b))
        return out

    def check(self, answers, k):
        for (mode, pre), (qs, got) in answers.items():
            assert got[0].shape == got[1].shape == got[2].shape == (len(qs), k) and got[3].shape == (len(qs),)
            for i, q in enumerate(qs):
                assert_lists_equal(row_of(got, i), self.expect(q, mode, pre, k), f"{self.name}: {mode} robot_pre {pre} query {q} at k = {k}")

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


# ---- 1. against the checker ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("grid", list(GRIDS))
def test_both_calls_against_the_checker(worlds, grid, k):
    """ONE call of 19 queries whose robots alternate, so every launch group mixes rules; intra, inter over every other robot and inter
    over each named robot (asked by the queries of the others)."""
    w = worlds(grid)
    queries = mixed_queries(w.robots, w.indexs)
    assert len(queries) == 19 and (np.diff(w.robots[queries[:9]].astype(int)) != 0).all()
    answers = w.searches(w.eng, queries, k)
    w.check(answers, k)
    assert answers[("intra", None)][1][3].min() == 0 and answers[("intra", None)][1][3].max() > 0      # the oldest keyframes search empty sets
    if w.n > 200:                                                         # full lists, and the planted index anomalies were asked for
        assert (answers[("inter", -1)][1][3] == k).all()
        zero, one = np.flatnonzero(w.robots == 0), np.flatnonzero(w.robots == 1)
        q0 = zero[w.indexs[zero] == SWAP_AT + 1 + EXCLUDE][0]; q1 = one[w.indexs[one] == DUP_AT + EXCLUDE][0]
        assert q0 in queries and q1 in queries
        m0 = eligible(w.robots, w.indexs, q0, "intra", exclude=EXCLUDE); m1 = eligible(w.robots, w.indexs, q1, "intra", exclude=EXCLUDE)
        assert not m0[zero[SWAP_AT]] and m0[zero[SWAP_AT + 1]]            # the later slot is in, the earlier one out
        assert m1[one[DUP_AT]] and m1[one[DUP_AT - 1]]


# ---- 2. twins: no checker at all -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", ["20x60", "64x120"])
def test_twins_of_the_slot_range_searches(worlds, grid):
    """A one-robot engine with index = slot: sc_search_intra is sc_search.  An engine whose robots sit in contiguous blocks:
    sc_search_inter(robot_pre = b) is sc_search_range over block b."""
    w = worlds(grid)
    n = w.n
    one = new_engine(w.R, w.S, w.descs)
    curs = np.array([n - 1, EXCLUDE + 1, EXCLUDE, 0, n // 2, 130 + EXCLUDE + 1, 64 + EXCLUDE, n - 2, 5, n - 3, 77, 200, 1, 199, 65, 129, 191, 192, n - 4], dtype=np.int32)
    for k in KS:
        same_answer(one.sc_search_intra(curs, k), one.sc_search(curs, k), f"{grid}: one robot, k = {k}")
    one.close()
    bounds = [0, 100, 190, n]
    robots = np.repeat(np.arange(3, dtype=np.int8), np.diff(bounds))
    indexs = np.concatenate([np.arange(b - a, dtype=np.int32) for a, b in zip(bounds[:-1], bounds[1:])])
    blocks = new_engine(w.R, w.S, w.descs, robots, indexs)
    for b in range(3):
        sub = curs[robots[curs] != b]
        for k in KS:
            same_answer(blocks.sc_search_inter(sub, k, robot_pre=b), blocks.sc_search_range(sub, bounds[b], bounds[b + 1], k), f"{grid}: block {b}, k = {k}")
    blocks.close()


# ---- 3. eligible-set sizes -------------------------------------------------------------------------------------------------------------
def test_eligible_set_sizes_and_the_fillers():
    """Databases of 70 keyframes in which robot 1 owns exactly 0, 1, k-1, k, k+1 keyframes, scattered: n_found and the fillers."""
    R, S, n = 20, 60, 70
    descs = synth_descriptors(n, R, S, seed=731, revisit_frac=0.05)
    db = ob.OracleDB(ob.make_config(R=R, S=S)); db.save_bulk(descs)
    d, s = db.distance_batch(n - 1, n=n, fast=True)
    assert (d[:n - 1] < NO_DIST).all()                                    # every pair listable: the set's size is the list's
    for k in (2, 25):
        for m in sorted({0, 1, k - 1, k, k + 1}):
            robots = np.zeros(n, dtype=np.int8)
            owned = (np.arange(m) * (n - 2) // max(m, 1) + 1) if m else np.array([], dtype=int)      # slots 1 .. n-2, never the query's
            assert len(set(owned.tolist())) == m
            robots[owned] = 1
            indexs = np.zeros(n, dtype=np.int32)
            for r in (0, 1):
                indexs[robots == r] = np.arange(int(np.sum(robots == r)))
            eng = new_engine(R, S, descs, robots, indexs)
            for pre in (1, -1):
                got = eng.sc_search_inter([n - 1], k, robot_pre=pre)
                want = ranked_eligible(d, s, eligible(robots, indexs, n - 1, "inter", pre), k)
                assert want[3] == min(k, m)
                assert_lists_equal(row_of(got, 0), want, f"robot 1 owns {m}, k = {k}, robot_pre {pre}")
                f = min(k, m)
                assert got[3][0] == f and (got[0][0][f:] == -1).all() and (got[1][0][f:] == 0).all() and (got[2][0][f:] == NO_DIST).all()
                assert set(got[0][0][:f].tolist()) <= set(owned.tolist())
            if m:                                                         # the newest of robot 1 asks for its own m - 1 - EXCLUDE older ones
                q = int(owned[-1])
                dq, sq = db.distance_batch(q, n=n, fast=True)
                got = eng.sc_search_intra([q], k)
                want = ranked_eligible(dq, sq, eligible(robots, indexs, q, "intra", exclude=EXCLUDE), k)
                assert want[3] == min(k, max(m - 1 - EXCLUDE, 0))
                assert_lists_equal(row_of(got, 0), want, f"robot 1 owns {m}, k = {k}, intra")
            eng.close()
    db.close()


# ---- 4. database sizes -----------------------------------------------------------------------------------------------------------------
def test_database_sizes_around_the_tiles():
    """Databases of 1, 63, 64, 65, 255, 256 and 257 slots, robots alternating slot by slot inside every tile but tile 2, which is all
    robot 2: for a query of robot 0 or 1 (intra, or inter over the other of the two) that tile holds no eligible entry between tiles
    that do."""
    R, S, N, k = 20, 60, 257, 25
    descs = synth_descriptors(N, R, S, seed=741, revisit_frac=0.05)
    robots = (np.arange(N) % 3).astype(np.int8)
    robots[TILE2[0]:TILE2[1]] = 2
    indexs = np.zeros(N, dtype=np.int32)
    for r in range(3):
        indexs[robots == r] = np.arange(int(np.sum(robots == r)))
    db = ob.OracleDB(ob.make_config(R=R, S=S)); db.save_bulk(descs)
    for n in (1, 63, 64, 65, 255, 256, 257):
        eng = new_engine(R, S, descs[:n], robots[:n], indexs[:n])
        queries = np.array(sorted({n - 1, max(n - 2, 0), max(n - 3, 0), 0, n // 2}), dtype=np.int32)
        assert n < 3 or set(robots[queries].tolist()) == {0, 1, 2}
        rows = {int(q): db.distance_batch(int(q), n=n, fast=True) for q in queries}
        calls = [("intra", None, queries, eng.sc_search_intra(queries, k)), ("inter", -1, queries, eng.sc_search_inter(queries, k))]
        for b in range(3):
            sub = queries[robots[queries] != b]
            calls.append(("inter", b, sub, eng.sc_search_inter(sub, k, robot_pre=b)))
        for mode, pre, qs, got in calls:
            assert got[3].shape == (len(qs),)
            for i, q in enumerate(qs):
                mask = eligible(robots[:n], indexs[:n], int(q), mode, pre, EXCLUDE)
                if n >= 255 and q >= n - 3 and robots[q] != 2 and (mode == "intra" or pre in (0, 1)):
                    assert not mask[TILE2[0]:TILE2[1]].any() and mask[64:128].any() and mask[192:n].any()
                assert_lists_equal(row_of(got, i), ranked_eligible(*rows[int(q)], mask, k), f"{n} slots: {mode} robot_pre {pre} query {q}")
        eng.close()
    db.close()


# ---- 5. ties and unlistable keyframes --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", ["20x60", "64x120"])
def test_ties_go_to_the_lower_eligible_slot(worlds, grid):
    """Slots 63, 64 and 130 (robots 0, 1, 2) are copies of the last keyframe, which is the query: distance exactly 0.0.  The lists name
    the copies on eligible robots in slot order and leave the one on an ineligible robot out."""
    w = worlds(grid)
    n, q = w.n, w.n - 1
    r = int(w.robots[q])
    d, s = w.row(q)
    assert all(d[p] == 0.0 for p in COPIES)
    others = [p for p in COPIES if w.robots[p] != r]
    own = [p for p in COPIES if w.robots[p] == r]
    assert len(others) == 2 and len(own) == 1 and eligible(w.robots, w.indexs, q, "intra", exclude=EXCLUDE)[own[0]]
    for k in (1, 2, 3, 32):
        got = w.eng.sc_search_inter([q], k)
        assert_lists_equal(row_of(got, 0), w.expect(q, "inter", -1, k), f"{grid}: k = {k}")
        assert got[0][0][:2].tolist() == others[:k] and (got[2][0][:min(k, 2)] == 0.0).all()
        assert own[0] not in got[0][0] and q not in got[0][0]
        for b in range(3):
            if b == r:
                continue
            got = w.eng.sc_search_inter([q], k, robot_pre=b)
            assert_lists_equal(row_of(got, 0), w.expect(q, "inter", b, k), f"{grid}: robot_pre {b}, k = {k}")
            assert w.robots[got[0][0][0]] == b and got[0][0][0] in others and got[2][0][0] == 0.0
            assert not (set(got[0][0].tolist()) & (set(COPIES) - {int(got[0][0][0])}))
        got = w.eng.sc_search_intra([q], k)
        assert_lists_equal(row_of(got, 0), w.expect(q, "intra", None, k), f"{grid}: intra, k = {k}")
        assert got[0][0][0] == own[0] and got[2][0][0] == 0.0 and not (set(got[0][0].tolist()) & set(others))


@pytest.mark.parametrize("grid", ["20x60", "64x120", "22x50"])
def test_the_all_zero_keyframe_is_never_listed_and_the_nan_keyframe_only_where_the_checker_scores_it(worlds, grid):
    """Both sit in robot 1.  The all-zero keyframe scores exactly 1e7 in the checker and is never listed; the keyframe with a NaN cell
    is listed only where the checker's distance is below 1e7 (which depends on the query), and no list holds a NaN.  On 22x50 robot 1
    owns fewer keyframes than k = 32: n_found is what is listable, the fillers behind it."""
    w = worlds(grid)
    own1 = np.flatnonzero(w.robots == 1)
    queries = np.array([s for s in (w.n - 1, w.n - 2, w.n - 3, w.n - 4, w.n - 5, 0, 1, 2) if w.robots[s] != 1][:4], dtype=np.int32)
    assert len(queries) >= 2
    for k in (5, 32):
        for pre in (1, -1):
            got = w.eng.sc_search_inter(queries, k, robot_pre=pre)
            for i, q in enumerate(queries):
                d, s = w.row(q)
                assert d[ZERO_AT] == NO_DIST
                assert_lists_equal(row_of(got, i), w.expect(q, "inter", pre, k), f"{grid}: query {q}, robot_pre {pre}, k = {k}")
                assert ZERO_AT not in got[0][i] and (NAN_AT not in got[0][i] or d[NAN_AT] < NO_DIST) and not np.isnan(got[2][i]).any()
                if pre == 1 and own1.size <= k:
                    listable = int(np.sum(d[own1] < NO_DIST))
                    assert got[3][i] == listable <= own1.size - 1 and (got[0][i][listable:] == -1).all() and (got[2][i][listable:] == NO_DIST).all()
    q1 = int(own1[-1])                                                    # a query of robot 1 itself: intra
    got = w.eng.sc_search_intra([q1, ZERO_AT], 32)
    assert_lists_equal(row_of(got, 0), w.expect(q1, "intra", None, 32), f"{grid}: intra of robot 1")
    assert ZERO_AT not in got[0][0] and not np.isnan(got[2][0]).any() and got[3][1] == 0        # the all-zero keyframe as a query lists nothing


# ---- 6. the device copy of (robot, index) ----------------------------------------------------------------------------------------------
def test_the_mirror_follows_appends_growth_and_a_reload(tmp_path):
    """Search -> append 1 -> search -> append 200 (64 -> 128 -> 256 slots of capacity) -> search: every search equals a fresh engine built
    in one piece; then db_dump -> db_load into a new engine -> the same lists."""
    R, S, N, k = 20, 60, 251, 25
    descs = make_descs(R, S, N, seed=761)
    robots, indexs = layout(N)
    eng = new_engine(R, S, descs[:50], robots[:50], indexs[:50])

    def lists(e, n):
        qs = mixed_queries(robots[:n], indexs[:n], count=12)
        out = [e.sc_search_intra(qs, k), e.sc_search_inter(qs, k)]
        for b in range(3):
            out.append(e.sc_search_inter(qs[robots[qs] != b], k, robot_pre=b))
        return out

    def against_a_fresh_engine(n):
        fresh = new_engine(R, S, descs[:n], robots[:n], indexs[:n])
        a, b = lists(eng, n), lists(fresh, n)
        fresh.close()
        for x, y in zip(a, b):
            same_answer(x, y, f"{n} keyframes")
        return a

    against_a_fresh_engine(50)
    eng.save_bulk(descs[50:51], robots[50:51], indexs[50:51])
    against_a_fresh_engine(51)
    eng.save_bulk(descs[51:], robots[51:], indexs[51:])
    last = against_a_fresh_engine(N)
    assert any((x[3] > 0).any() for x in last)
    path = str(tmp_path / "team.scdb")
    eng.db_dump(path)
    loaded = ScanContextEngine(num_ring=R, num_sector=S, num_exclude_recent=EXCLUDE, initial_capacity=64)
    assert loaded.db_load(path) == N and loaded.get_index(N - 1) == (int(robots[N - 1]), int(indexs[N - 1]))
    for x, y in zip(lists(loaded, N), last):
        same_answer(x, y, "reloaded")
    loaded.close(); eng.close()


# ---- 7. the matrix range is narrowed to the eligible span ------------------------------------------------------------------------------
def test_the_matrix_runs_over_the_eligible_span_only(worlds):
    """20x60, robots in contiguous blocks [0, 100), [100, 190), [190, 300): the profile's pair count grows by the span's length, not by
    the database's, and the lists are the checker's."""
    w = worlds("20x60")
    n = w.n
    bounds = [0, 100, 190, n]
    robots = np.repeat(np.arange(3, dtype=np.int8), np.diff(bounds))
    indexs = np.concatenate([np.arange(b - a, dtype=np.int32) for a, b in zip(bounds[:-1], bounds[1:])])
    eng = new_engine(w.R, w.S, w.descs, robots, indexs)
    eng.profile_enable(1)
    q, k = n - 1, 25
    d, s = w.row(q)

    def pairs_of(call):
        before = eng.profile()["sc_distance_pairs"]
        got = call()
        return got, eng.profile()["sc_distance_pairs"] - before

    got, pairs = pairs_of(lambda: eng.sc_search_inter([q], k, robot_pre=1))
    assert_lists_equal(row_of(got, 0), ranked_eligible(d, s, eligible(robots, indexs, q, "inter", 1), k), "block 1")
    print("pairs scored for block 1:", pairs)
    assert pairs == 90
    got, pairs = pairs_of(lambda: eng.sc_search_inter([q], k, robot_pre=0))
    assert_lists_equal(row_of(got, 0), ranked_eligible(d, s, eligible(robots, indexs, q, "inter", 0), k), "block 0")
    assert pairs == 100
    got, pairs = pairs_of(lambda: eng.sc_search_intra([q], k))            # robot 2's keyframes 0 .. 109 - 1 - EXCLUDE - 1
    assert_lists_equal(row_of(got, 0), ranked_eligible(d, s, eligible(robots, indexs, q, "intra", exclude=EXCLUDE), k), "intra")
    assert pairs == n - 190 - 1 - EXCLUDE
    got, pairs = pairs_of(lambda: eng.sc_search_inter([q], k))            # every other robot: blocks 0 and 1
    assert_lists_equal(row_of(got, 0), ranked_eligible(d, s, eligible(robots, indexs, q, "inter"), k), "blocks 0 and 1")
    assert pairs == 190
    got, pairs = pairs_of(lambda: eng.sc_search_intra([190], k))          # nothing eligible: nothing scored
    assert got[3][0] == 0 and pairs == 0
    eng.close()


# ---- 8. no trace; errors write nothing -------------------------------------------------------------------------------------------------
def _sentinels(nq, k):
    return (np.full((nq, max(k, 1)), -7, dtype=np.int32), np.full((nq, max(k, 1)), -7, dtype=np.int32), np.full((nq, max(k, 1)), -7.0), np.full(nq, -7, dtype=np.int32))


@pytest.mark.parametrize("grid", ["20x60", "64x120"])
def test_searches_leave_no_trace_and_errors_write_nothing(worlds, grid):
    """Two fresh engines go through the same detect_full, detect_inter (which keeps the periodic tree's counter), sc_search and
    sc_search_range calls twice; one of them runs both per-robot searches in between -- and fails in every way they can."""
    w = worlds(grid)
    n = w.n
    a, b = w.engine(tree_making_period=3), w.engine(tree_making_period=3)
    curs = [n - 1, n // 2, EXCLUDE + 3, n - 2, n - 3]

    def answers(eng):
        out = [eng.detect_full(c) for c in curs] + [eng.detect_inter(c) for c in curs]
        return out + [eng.sc_search(curs, 7), eng.sc_search_range(curs, 0, n, 7)]

    def same(x, y):
        if isinstance(x, tuple):
            return len(x) == len(y) and all(same(p, q) for p, q in zip(x, y))
        x, y = np.asarray(x), np.asarray(y)
        if x.dtype.kind == "f":
            x, y = x.astype(np.float64).view(np.uint64), y.astype(np.float64).view(np.uint64)
        return np.array_equal(x, y)

    assert all(same(x, y) for x, y in zip(answers(a), answers(b)))
    queries = mixed_queries(w.robots, w.indexs)
    for k in (1, 25):
        w.check(w.searches(a, queries, k), k)
    q = n - 1
    r = int(w.robots[q])
    other = np.flatnonzero(w.robots != r)[-1]
    errors = [(lambda out: a.sc_search_inter([other, q], 3, robot_pre=r, out=out), 2, 3, INVALID_ARG),      # robot_pre is the robot of ONE query
              (lambda out: a.sc_search_inter([q], 3, robot_pre=128, out=out), 1, 3, INVALID_ARG),
              (lambda out: a.sc_search_inter([q], 3, robot_pre=-2, out=out), 1, 3, INVALID_ARG),
              (lambda out: a.sc_search_inter([q, n], 3, out=out), 2, 3, OUT_OF_RANGE),
              (lambda out: a.sc_search_intra([q, n], 3, out=out), 2, 3, OUT_OF_RANGE),
              (lambda out: a.sc_search_intra([-1, q], 3, out=out), 2, 3, OUT_OF_RANGE),
              (lambda out: a.sc_search_intra([q], 0, out=out), 1, 0, INVALID_ARG),
              (lambda out: a.sc_search_intra([q], 33, out=out), 1, 33, INVALID_ARG),
              (lambda out: a.sc_search_inter([q], 0, out=out), 1, 0, INVALID_ARG),
              (lambda out: a.sc_search_inter([q], 33, out=out), 1, 33, INVALID_ARG)]
    for call, nq, k, status in errors:
        out = _sentinels(nq, k)
        with pytest.raises(SclError) as ei:
            call(out)
        assert ei.value.status == status, (nq, k, status)
        assert (out[0] == -7).all() and (out[1] == -7).all() and (out[2] == -7.0).all() and (out[3] == -7).all()
        got = a.sc_search_inter([q], 3)                                  # the next call is unaffected
        assert_lists_equal(row_of(got, 0), w.expect(q, "inter", -1, 3), f"{grid}: after an error")
    assert a.sc_search_intra([], 5)[0].shape == (0, 5) and a.sc_search_inter([], 5)[3].shape == (0,)
    assert all(same(x, y) for x, y in zip(answers(a), answers(b)))
    a.close(); b.close()


# ---- 9. shards ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [2, 3])
@pytest.mark.parametrize("grid", ["20x60", "64x120"])
def test_sharded_lists_equal_the_single_engine(worlds, grid, G):
    """One database over G shards (all on device 0, host merge): every list of the first test, bit for bit, and the errors."""
    w = worlds(grid)
    sh = w.engine(devices=[0] * G, exchange=1)
    assert sh.shard_info() == (G, 1)
    queries = mixed_queries(w.robots, w.indexs)
    for k in KS:
        one, many = w.searches(w.eng, queries, k), w.searches(sh, queries, k)
        for key in one:
            same_answer(many[key][1], one[key][1], f"{grid}, G = {G}, k = {k}, {key}")
    q = w.n - 1
    for call, status in ((lambda out: sh.sc_search_inter([q], 3, robot_pre=int(w.robots[q]), out=out), INVALID_ARG),
                         (lambda out: sh.sc_search_inter([q], 3, robot_pre=128, out=out), INVALID_ARG),
                         (lambda out: sh.sc_search_intra([w.n], 3, out=out), OUT_OF_RANGE)):
        out = _sentinels(1, 3)
        with pytest.raises(SclError) as ei:
            call(out)
        assert ei.value.status == status and (out[0] == -7).all() and (out[3] == -7).all()
    sh.close()


@pytest.mark.parametrize("G", [2, 3])
@pytest.mark.parametrize("grid", ["20x60", "64x120"])
def test_sharded_default_indexes_are_global_slots(worlds, grid, G):
    """A one-robot database appended ONE keyframe at a time without robots or indexes (then a bulk of the rest, also without): every
    keyframe's index is its global slot on the shards too, so on G shards sc_search_intra is sc_search and both are the one engine's."""
    w = worlds(grid)
    n, single = 150, 97
    one = new_engine(w.R, w.S, w.descs[:n])
    sh = new_engine(w.R, w.S, w.descs[:0], devices=[0] * G, exchange=1)
    for i in range(single):
        sh.save_bulk(w.descs[i:i + 1])
    sh.save_bulk(w.descs[single:n])
    assert [sh.get_index(s) for s in (0, 1, 50, single - 1, single, n - 1)] == [(0, s) for s in (0, 1, 50, single - 1, single, n - 1)]
    curs = np.array([n - 1, 50, EXCLUDE + 1, EXCLUDE, 0, 60, 61, single, single - 1, single + EXCLUDE, 2 * EXCLUDE + G, n - 2, 75, 31, 30, 29, 140, 101, 11], dtype=np.int32)
    for k in (1, 25, 32):
        want = one.sc_search(curs, k)
        same_answer(one.sc_search_intra(curs, k), want, f"{grid}: one engine, k = {k}")
        same_answer(sh.sc_search(curs, k), want, f"{grid}: G = {G}, sc_search, k = {k}")
        same_answer(sh.sc_search_intra(curs, k), want, f"{grid}: G = {G}, sc_search_intra, k = {k}")
        for i, cur in enumerate(curs):
            listed = want[0][i][:want[3][i]]
            assert (listed < cur - EXCLUDE).all()
    assert want[3].max() == 32 and want[3].min() == 0
    one.close(); sh.close()


# ---- 10. end to end: search per robot -> get_index -> guess -> verification ------------------------------------------------------------
SECTORS_TURNED = 7                                                    # 42 degrees on the 20 x 60 grid: a whole number of sectors
IDENT = np.eye(4, dtype=np.float32)
THR, RATIO, SEED = 0.25, 0.45, 3


def test_inter_search_guess_verification_end_to_end():
    """Two robots on the 20 x 60 grid whose keyframes ALTERNATE slot by slot.  Robot 0's keyframe 1 is a scan at pose_pre in its world
    frame (with 2 cm of noise on every point: another scan of the place); robot 1 stood still at that place with the sensor turned by 7
    sectors, so its own earlier keyframes are the best matches of the one received last.  sc_search_range over everything lists them first -- candidates the store of robot 0 cannot
    verify; sc_search_inter(robot_pre = 0) lists robot 0's keyframes, get_index turns them into its keys, scl_loop_guess_from_shift
    turns the shift and the two poses into the guess, and the store form verifies the planted revisit."""
    cloud = synth_scan(20000, seed=7)
    Rz = rigid_transform(0.0, 0.0, np.radians(SECTORS_TURNED * 6.0), 0, 0, 0)
    turned = cloud.copy()
    turned[:, :3] = (cloud[:, :3].astype(np.float64) @ Rz[:3, :3].T).astype(np.float32)
    seen = cloud.copy()
    seen[:, :3] += np.random.default_rng(5).normal(0.0, 0.02, (len(cloud), 3)).astype(np.float32)
    cfg = ob.make_config(R=20, S=60)
    d_seen, want_shift = ob.distance(cfg, ob.make_scancontext(cfg, turned), ob.make_scancontext(cfg, seen))
    assert want_shift == SECTORS_TURNED and 0.0 < d_seen < 0.01         # a near match, but not the sender's own scan
    pose_pre = np.float32([14.0, -6.5, 0.4, 0.02, -0.015, 1.1])
    pose_cur = np.float32([-35.0, 22.0, -0.3, -0.01, 0.025, -2.3])
    e = ScanContextEngine(num_ring=20, num_sector=60)
    try:
        M_pre, M_cur = e.pose_to_matrix(*[float(v) for v in pose_pre]), e.pose_to_matrix(*[float(v) for v in pose_cur])
        own = (synth_scan(20000, seed=11), seen, synth_scan(20000, seed=12))
        for k in range(3):                                            # slot 2k: robot 0's keyframe k (descriptor and cloud); slot 2k + 1: robot 1's
            e.make_and_save(own[k], 0, k)
            e.keyframe_put(0, k, own[k])
            e.make_and_save(turned, 1, k)
        cur = 5                                                       # the received keyframe: robot 1's newest
        assert [e.get_index(s) for s in range(6)] == [(0, 0), (1, 0), (0, 1), (1, 1), (0, 2), (1, 2)]
        ids, shifts, dists, found = e.sc_search_range([cur], 0, cur, 2)
        print("by slot range", ids, shifts, dists, found)
        assert e.get_index(int(ids[0, 0]))[0] == 1                    # the sender's own keyframe comes first: the failure
        top = e.sc_search_range([cur], 0, cur, 1)
        assert [i for i in top[0][0] if i >= 0 and e.get_index(int(i))[0] == 0] == []     # over-fetching 1 and filtering leaves nothing
        ids, shifts, dists, found = e.sc_search_inter([cur], 2, robot_pre=0)
        print("robot 0 only", ids, shifts, dists, found)
        assert found[0] == 2 and ids[0, 0] == 2 and shifts[0, 0] == want_shift
        assert all(e.get_index(int(i))[0] == 0 for i in ids[0])
        keys = [int(e.get_index(int(i))[1]) for i in ids[0]]
        assert keys[0] == 1
        received = e.transform_cloud(turned, M_cur)                   # what the other robot sends
        received[::400, 0] = np.nan                                   # rows the voxel filter drops
        G = np.stack([e.loop_guess_from_shift(int(shifts[0, j]), 60, pose_cur, pose_pre if keys[j] == 1 else np.zeros(6)) for j in range(2)])
        windows = np.stack([M_pre if key == 1 else IDENT for key in keys]).reshape(2, 1, 4, 4)
        args = (received, 0.1, 0, keys, 0, windows, 0.1)
        got = e.geometric_verification_batch_from_store_guess(*args, G, 300, THR, RATIO, SEED)
        print("guessed", got[1], got[2], got[3], got[4], got[5])
        assert got[1][0] and got[2] >= 300                            # the planted revisit verifies
        assert not got[1][1]                                          # the other place stays unverified
        assert np.abs(got[6][0] - IDENT).max() < 0.05                 # the fit is the residual; T is the whole motion
        back = received[np.isfinite(received[:, 0]), :3].astype(np.float64) @ got[0][0, :3, :3].astype(np.float64).T + got[0][0, :3, 3]
        there = e.transform_cloud(cloud, M_pre)[np.isfinite(received[:, 0]), :3]
        assert np.linalg.norm(back - there, axis=1).max() < 0.05
    finally:
        e.close()
