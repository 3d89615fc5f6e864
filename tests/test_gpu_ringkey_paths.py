"""The ring-key search on every path its dispatch can take, against the CPU checker: oracle_binding.knn (nanoflann's metric order,
ties by ascending index, exclude_eps) for the neighbours and OracleDB.distance_batch for their SC distances.  Every comparison is
exact: indices, the bits of d2 (uint32) and of dist (uint64), shifts, found, and (-1, FLT_MAX) behind found.  No tolerances.

The cases, the path each is meant to take and the arithmetic that puts it there are in tests/ringkey_path_cases.py (pinned on the
checker alone by tests/test_ringkey_path_cases.py); every test id names its path.  Every database is built once per module.
Section 5 keeps the issue's 53 000 keyframes of the 20 x 60 grid: synth_descriptors, the checker's save_bulk and ringkeys take 4 s
together on the CPU, the three engines' save_bulk well under a second each."""
import numpy as np
import pytest

import oracle_binding as ob
import ringkey_path_cases as rc
from scl_slam_amd import ScanContextEngine
from scl_slam_amd.engine import SclError
from scl_slam_amd.synth import synth_descriptors

pytestmark = pytest.mark.gpu
S = rc.S_PLANT


def planted_engine(keys, eps=0.0):
    """test_gpu_topk.engine_with_ringkeys: constant rows, so the ring key of a keyframe is the planted value (32 R bytes each)"""
    N, R = keys.shape
    eng = ScanContextEngine(num_ring=R, num_sector=S, num_candidates=3, knn_exclude_eps=eps, initial_capacity=N + 8)
    eng.save_bulk(np.repeat(keys[:, :, None], S, axis=2))
    for i in (0, N // 2, N - 1):
        assert np.array_equal(eng.get_ringkey(i), keys[i], equal_nan=True)
    return eng


def same_bits(a, b):
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    return a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def check_bare(eng, keys, c, k, kind, val):
    if kind == "slot":
        qarg, qkey = val, keys[val]
    else:
        eng.stage_query(np.repeat(val[:, None], S, axis=1))
        qarg, qkey = -1, val
    idx, d2, found = eng.ringkey_topk(qarg, c.lo, c.hi, k)
    o_idx, o_d2, o_found = ob.knn(keys[c.lo:c.hi], qkey, k, exclude_eps=c.eps)
    want = np.where(o_idx >= 0, o_idx + c.lo, -1).astype(np.int32)
    where = (c.id, k, kind)
    assert found == o_found, where
    assert np.array_equal(idx, want), (where, idx, want)
    assert same_bits(d2, o_d2), (where, d2, o_d2)
    assert np.all(idx[found:] == -1) and np.all(d2[found:] == np.finfo(np.float32).max), where
    if c.prop is not None and (c.prop_all or kind == "planted"):
        assert c.prop(o_idx, o_found, k), where               # the placement the case was built for (the CPU test pins it too)


def run_case(eng, keys, c):
    for k in c.ks:
        for kind, val in c.queries:
            check_bare(eng, keys, c, k, kind, val)


# ---- 1. range size: ringkey_lists_kernel, ringkey_lists_chunked_kernel, and the stride over the chunks ----
@pytest.fixture(scope="module")
def range_db():
    keys, _ = rc.range_world()
    eng = planted_engine(keys)
    yield eng, keys
    eng.close()


@pytest.mark.parametrize("c", rc.range_world()[1], ids=lambda c: c.id)
def test_range_sizes_on_both_scan_kernels(range_db, c):
    run_case(*range_db, c)


# ---- 2. ring counts off the fast path ----
@pytest.mark.parametrize("R,N", rc.metric_worlds(), ids=[f"metric-{rc.route(N, R, 3)['metric']}-R{R}-{rc.route(N, R, 3)['scan']}-N{N}" for R, N in rc.metric_worlds()])
def test_ring_counts(R, N):
    keys, cases = rc.metric_world(R, N)
    eng = planted_engine(keys)
    for i in range(0, N, max(1, N // 7)):
        assert np.array_equal(eng.get_ringkey(i), keys[i])
    for c in cases:
        print(c.id, c.why)
        run_case(eng, keys, c)
    eng.close()


def test_ring_count_257_is_refused_at_creation():
    """scl_create: num_ring > 256 is SCL_ERR_INVALID_ARG (-1) before anything is allocated -- both scan kernels hold the query's ring
    key in sq[256], and launch_ringkey_lists would refuse R > 256 as well, but no engine of that shape ever exists"""
    with pytest.raises(SclError) as ei:
        ScanContextEngine(num_ring=rc.METRIC_REFUSED_R, num_sector=S)
    assert ei.value.status == -1
    ScanContextEngine(num_ring=rc.MAX_RINGS, num_sector=S).close()


# ---- 3. both rank paths of the lists kernel with fewer valid keys than k ----
@pytest.fixture(scope="module")
def short_dbs():
    tables, _ = rc.short_world()
    engs = {name: planted_engine(keys, eps=rc.FLT_EPSILON if name == "copies" else 0.0) for name, keys in tables.items()}
    a, b = rc.BLOCK
    for i in (a, a + 1, a + 2, b - 1):
        assert np.array_equal(engs["holes"].get_ringkey(i), tables["holes"][i], equal_nan=True)
    yield engs, tables
    for e in engs.values():
        e.close()


@pytest.mark.parametrize("c", rc.short_world()[1], ids=lambda c: c.id)
def test_fewer_valid_keys_than_k(short_dbs, c):
    engs, tables = short_dbs
    run_case(engs[c.db], tables[c.db], c)


# ---- 4. the merges on both sides of 3 072 keys, and the threshold rule inside the first ----
@pytest.fixture(scope="module")
def merge_db():
    keys, _ = rc.merge_world()
    eng = planted_engine(keys)
    assert np.array_equal(eng.get_ringkey(rc.Z48), keys[rc.Z48]) and np.all(np.isinf(keys[rc.Z48]))
    yield eng, keys
    eng.close()


@pytest.mark.parametrize("c", rc.merge_world()[1], ids=lambda c: c.id)
def test_merges(merge_db, c):
    run_case(*merge_db, c)


def test_rounds_merge_alternating_with_k3_never_returns_the_previous_calls_block(merge_db):
    """k = 64 over 100 lists (rounds merge, then topk_pack_kernel fills the pinned block) alternating with k = 3 over the same
    lists (threshold merge, which writes the block itself): neither may read the other's block"""
    eng, keys = merge_db
    c = rc.rounds_case()
    for rep in range(6):
        for k in rc.ALTERNATING:
            kind, val = c.queries[rep % len(c.queries)]
            check_bare(eng, keys, c, k, kind, val)


# ---- 5. the consumers on a supported grid (20 x 60) ----
class Grid:
    pass


@pytest.fixture(scope="module")
def grid():
    """one engine with num_candidates = 16 (tree_making_period = 1: detect_inter searches [0, n - 100) on every call) beside the
    checker's database; detect_inter is run while the two hold 16 484 and 16 485 keyframes, then the rest is saved"""
    g = Grid()
    R, Sg, n = rc.GRID_R, rc.GRID_S, rc.GRID_N
    g.descs = synth_descriptors(n, R, Sg, seed=5, revisit_frac=0.01)
    g.eng = ScanContextEngine(num_ring=R, num_sector=Sg, num_candidates=rc.DETECT_K, tree_making_period=1, initial_capacity=n + 8)
    g.db = ob.OracleDB(ob.make_config(R=R, S=Sg, k=rc.DETECT_K, tree_period=1))
    g.inter = []
    at = 0
    for cur in rc.DETECT_CURS:                               # n = cur: the search set of detect_inter is [0, cur - 100)
        g.eng.save_bulk(g.descs[at:cur]); g.db.save_bulk(g.descs[at:cur]); at = cur
        try:                                                 # (an error is the test's to report, not every test's on this fixture)
            got = g.eng.detect_inter(cur - 1)
        except SclError as exc:
            got = exc
        g.inter.append((cur, got, g.db.detect_inter(cur - 1)))
    g.eng.save_bulk(g.descs[at:]); g.db.save_bulk(g.descs[at:])
    g.keys = g.db.ringkeys()
    yield g
    g.eng.close(); g.db.close()


def check_with_distance(g, q, lo, hi, k, where):
    idx, d2, dist, shift, found = g.eng.topk_with_distance(q, lo, hi, k)
    o_idx, o_d2, o_found = ob.knn(g.keys[lo:hi], g.keys[q], k)
    want = np.where(o_idx >= 0, o_idx + lo, -1).astype(np.int32)
    assert found == o_found == k, where
    assert np.array_equal(idx, want), (where, idx, want)
    assert same_bits(d2, o_d2), where
    o_dist, o_shift = g.db.distance_batch(q, cand=want)
    assert same_bits(dist, o_dist) and np.array_equal(shift, o_shift), (where, dist, o_dist, shift, o_shift)


@pytest.mark.parametrize("id,lo,hi,k", rc.grid_cases(), ids=lambda v: v if isinstance(v, str) else None)
def test_topk_with_distance_on_both_sides_of_the_candidates_limit(grid, id, lo, hi, k):
    for q in (rc.GRID_N - 1, 7, (lo + hi) // 2):
        check_with_distance(grid, q, lo, hi, k, (id, q))


def test_alternating_k_through_both_forms_of_the_candidates_kernel(grid):
    """k = 16 over 65 lists (merge first), k = 3 over the same range (merged by the kernel), k = 64 (rounds merge, distances, pack):
    one pinned block, three layouts"""
    for rep in range(4):
        for k in (16, 3, 64, 16, 5):
            check_with_distance(grid, 40000 + 13 * rep + k, 300, 300 + 16385, k, (rep, k))


def _same_detection(a, o):
    return a[0] == o[0] and np.float32(a[1]) == np.float32(o[1]) and same_bits(np.float64(a[2]), np.float64(o[2]))


@pytest.mark.parametrize("i", range(len(rc.DETECT_CURS)), ids=[f"{rc.route(c - 100, rc.GRID_R, rc.DETECT_K, 'dist', True)['cand']}-{c - 100}-slots" for c in rc.DETECT_CURS])
def test_detections_with_16_candidates_on_both_sides_of_the_limit(grid, i):
    """cur - 100 = 16 384: 64 lists x 16 = 1 024 keys, merged by the candidates' kernel; 16 385: 65 lists, 1 040 keys, merged first"""
    cur = rc.DETECT_CURS[i]
    a = grid.eng.detect_intra(cur); o = grid.db.detect_intra(cur)
    assert _same_detection(a, o[:3]), (cur, a, o)
    n, a, o = grid.inter[i]
    assert n == cur and not isinstance(a, Exception), (cur, a)
    assert _same_detection(a, o), (cur, a, o)


def test_detections_with_16_candidates_over_the_whole_database(grid):
    """52 900 slots: 207 lists x 16 = 3 312 keys -- the rounds merge in front of the candidates' kernel"""
    assert rc.route(rc.GRID_N - 100, rc.GRID_R, rc.DETECT_K, "dist", True)["merge"] == "rounds"
    for cur in (rc.GRID_N - 1, rc.GRID_N - 2):
        a = grid.eng.detect_intra(cur); o = grid.db.detect_intra(cur)
        assert _same_detection(a, o[:3]), (cur, a, o)
        a = grid.eng.detect_inter(cur); o = grid.db.detect_inter(cur)
        assert _same_detection(a, o), (cur, a, o)


def test_full_pass_delivers_the_same_lists_fused_and_stand_alone(grid):
    """detect_full_range, then last_topk: num_candidates = 4 is reduced by the SC-distance kernel's epilogue (kTailTop = 4), 5 by the
    stand-alone scan on the second stream (157 lists over 40 000 slots: more workgroups than CUs beside the SC kernel; 1 list over
    13).  Both equal the checker's lists, and the first four of the five are the four."""
    R, Sg = rc.GRID_R, rc.GRID_S
    n = max(hi for _, hi in rc.FULL_RANGES)
    engs = {}
    for k in rc.FULL_KS:
        engs[k] = ScanContextEngine(num_ring=R, num_sector=Sg, num_candidates=k, initial_capacity=n + 72)
        engs[k].save_bulk(grid.descs[:n + 64])
    for lo, hi in rc.FULL_RANGES:
        for q in (n + 10, 11):
            got = {}
            for k in rc.FULL_KS:
                nn, sh, d = engs[k].detect_full_range(q, lo, hi)
                idx, d2 = engs[k].last_topk(k)
                o_idx, o_d2, o_found = ob.knn(grid.keys[lo:hi], grid.keys[q], k)
                assert o_found == k
                assert np.array_equal(idx, o_idx + lo) and same_bits(d2, o_d2), (lo, hi, q, k, idx, o_idx + lo)
                got[k] = (idx, d2, nn, sh, d)
            a, b = got[rc.FULL_KS[0]], got[rc.FULL_KS[1]]
            assert np.array_equal(a[0], b[0][:4]) and same_bits(a[1], b[1][:4])
            assert a[2:4] == b[2:4] and same_bits(np.float64(a[4]), np.float64(b[4]))
            if hi - lo <= 64:                                # the winner against the checker where that is cheap
                dist, shift = grid.db.distance_batch(q, cand=np.arange(lo, hi, dtype=np.int32))
                j = int(np.lexsort((np.arange(hi - lo), dist))[0])
                assert (a[2], a[3]) == (lo + j, int(shift[j])) and same_bits(np.float64(a[4]), dist[j:j + 1][0])
    for e in engs.values():
        e.close()
