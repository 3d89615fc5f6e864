"""Pairwise consistency of loop closures on the GPU (include/scl_engine.h "PAIRWISE CONSISTENCY OF LOOP CLOSURES") against the checkers
of tests/pcm_cases.py: the d2 matrix within TAU of the 40-digit definition, the graph and the degrees bit for bit, the clique equal to
the contract's greedy on hand-made and random graphs, scl_pcm_select equal to clique-of-consistency, state and errors."""
from ctypes import POINTER, byref, c_double, c_int, c_uint64

import numpy as np
import pytest

import icp_guess_cases as gc
import pcm_cases as pc
import registration_eval_cases as rc
from scl_slam_amd import ScanContextEngine, SclError
from scl_slam_amd.synth import rigid_transform, synth_scan
from scl_slam_amd.engine import pcm_bool_to_words, pcm_words_to_bool

pytestmark = pytest.mark.gpu
INVALID_ARG = -1
GRAPH_SIZES = (1, 63, 64, 65, 127, 128, 129, 1000, 4095, 4096)


@pytest.fixture(scope="module")
def eng():
    e = ScanContextEngine(initial_capacity=16)
    yield e
    e.close()


def _run(e, c, threshold=None, odom="case", want_d2=True):
    return e.pcm_consistency(c.poses_a, c.poses_b, c.idx_a, c.idx_b, c.z, c.cov, c.threshold if threshold is None else threshold,
                             odom_var=c.odom_var if isinstance(odom, str) else odom, want_d2=want_d2)


def _select(e, c, threshold=None):
    return e.pcm_select(c.poses_a, c.poses_b, c.idx_a, c.idx_b, c.z, c.cov, c.threshold if threshold is None else threshold, odom_var=c.odom_var)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _check_graph_shape(r, n):
    W = (n + 63) // 64
    assert r.words.shape == (n, W) and not r.adj.diagonal().any()
    if n % 64:
        assert not (r.words[:, W - 1] >> np.uint64(n % 64)).any()               # no bit at or beyond n
    assert np.array_equal(r.adj, r.adj.T) and np.array_equal(r.degree, r.adj.sum(1))


@pytest.mark.parametrize("family", sorted(pc.FAMILIES))
@pytest.mark.parametrize("n", pc.SMALL_N)
def test_matrix_graph_and_select_against_the_exact_checker(eng, family, n):
    c, exact = pc.case_and_d2(family, n)
    r = _run(eng, c)
    assert np.array_equal(np.isinf(r.d2), np.isinf(exact))
    fin = np.isfinite(exact)
    dev = np.abs(r.d2 - exact)[fin] / np.maximum(1.0, exact[fin])
    print(family, n, "largest deviation from d2_exact:", dev.max(), "TAU:", pc.TAU[family])
    assert (dev <= pc.TAU[family]).all()
    assert np.array_equal(_bits(r.d2), _bits(r.d2.T)) and not r.d2.diagonal().any()
    g = pc.graph(exact, c.threshold)
    assert np.array_equal(r.adj, g) and np.array_equal(r.degree, g.sum(1))
    _check_graph_shape(r, n)
    again = _run(eng, c)
    assert np.array_equal(_bits(again.d2), _bits(r.d2)) and np.array_equal(again.words, r.words)
    # the clique of that graph, three ways
    want = pc.greedy_clique(g)
    mem, seed, deg = _select(eng, c)
    assert (tuple(mem.tolist()), seed) == want and np.array_equal(deg, r.degree)
    mem2, seed2 = eng.pcm_max_clique(r.words)
    assert (tuple(mem2.tolist()), seed2) == want
    if family == "planted":
        assert tuple(mem.tolist()) == tuple(np.flatnonzero(c.inlier).tolist())


@pytest.fixture(scope="module")
def large():
    """the two largest mixed cases and their numpy graphs, made once (the numpy pass over 8.4 M pairs is the slow part)"""
    return {n: pc.case_and_d2("mixed", n) for n in (4095, 4096)}


@pytest.mark.parametrize("n", GRAPH_SIZES)
def test_graph_sizes_against_the_numpy_graph(eng, large, n):
    c, d2 = large[n] if n in large else pc.case_and_d2("mixed", n)
    assert c.gap >= pc.KNIFE_EDGE
    r = _run(eng, c, want_d2=(n == 4096))
    g = pc.graph(d2, c.threshold)
    assert np.array_equal(r.adj, g) and np.array_equal(r.degree, g.sum(1))
    _check_graph_shape(r, n)
    if n == 4096:
        rs = np.random.RandomState(9)
        I = rs.randint(0, n, 500); J = rs.randint(0, n, 500)
        keep = I != J
        I, J = I[keep], J[keep]
        assert (np.abs(r.d2[I, J] - d2[I, J]) <= pc.TAU["mixed"] * np.maximum(1.0, d2[I, J])).all()
        assert np.array_equal(_bits(r.d2[I, J]), _bits(r.d2[J, I]))
    mem, seed, deg = _select(eng, c)                         # select = clique of consistency, at every size
    mem2, seed2 = eng.pcm_max_clique(r.words)
    assert np.array_equal(mem, mem2) and seed == seed2 and np.array_equal(deg, r.degree) and pc.is_clique(g, mem)
    if n <= 1000:                                            # (the checker takes a minute on the two largest: scripts/bench_pcm.py compares there)
        assert (tuple(mem.tolist()), seed) == pc.greedy_clique_fast(g)
    if n <= 129:
        assert (tuple(mem.tolist()), seed) == pc.greedy_clique(g)


def test_workspace_keeps_nothing_between_calls(eng, large):
    c_big, d2_big = large[4096]
    c_small, d2_small = pc.case_and_d2("mixed", 65)
    first = _run(eng, c_big, want_d2=False)
    sel_first = _select(eng, c_big)
    small = _run(eng, c_small)
    assert np.array_equal(small.adj, pc.graph(d2_small, c_small.threshold))
    mem, seed, _ = _select(eng, c_small)
    assert (tuple(mem.tolist()), seed) == pc.greedy_clique(small.adj)
    again = _run(eng, c_big, want_d2=False)
    assert np.array_equal(again.words, first.words) and np.array_equal(again.degree, first.degree)
    sel_again = _select(eng, c_big)
    assert np.array_equal(sel_again[0], sel_first[0]) and sel_again[1] == sel_first[1]
    assert pc.is_clique(first.adj, sel_first[0]) and len(sel_first[0]) >= 2
    mem2, seed2 = eng.pcm_max_clique(first.words)
    assert np.array_equal(mem2, sel_first[0]) and seed2 == sel_first[1]


# ---- odd inputs -----------------------------------------------------------------------------------------------------------------------

def test_intra_robot_loops_with_aliased_trajectories(eng):
    c, exact = pc.make_case(1.0, 30, seed=4242, same=True)
    assert c.poses_a is c.poses_b
    r = _run(eng, c)
    fin = np.isfinite(exact)
    assert (np.abs(r.d2 - exact)[fin] <= pc.TAU["mixed"] * np.maximum(1.0, exact[fin])).all()
    assert np.array_equal(r.adj, pc.graph(exact, c.threshold))


def test_duplicates_half_turns_and_unnormalised_quaternions(eng):
    c, _ = pc.case_and_d2("mixed", 40)
    z = c.z.copy(); ia = c.idx_a.copy(); ib = c.idx_b.copy(); cov = c.cov.copy()
    z[1] = z[0]; ia[1] = ia[0]; ib[1] = ib[0]                                    # a duplicate loop
    z[2, 3:] = [0.6, 0.0, 0.8, 0.0]                                              # an exact half turn: w = 0
    z[3, 3:] *= 2.0; z[4, 3:] *= -1.0; z[5, 3:] *= -0.5                          # norm 2, w < 0, both
    d = c._replace(z=z, idx_a=ia, idx_b=ib, cov=cov)
    exact = pc.d2_exact(d)
    r = _run(eng, d)
    fin = np.isfinite(exact)
    assert np.array_equal(np.isinf(r.d2), ~fin)
    assert (np.abs(r.d2 - exact)[fin] <= pc.TAU["mixed"] * np.maximum(1.0, exact[fin])).all()
    assert r.d2[0, 1] <= 1e-20 and r.adj[0, 1]                                  # the cycle of a loop with its copy: the identity up to rounding
    assert not (np.abs(exact - c.threshold) <= pc.KNIFE_EDGE * c.threshold).any()
    assert np.array_equal(r.adj, pc.graph(exact, c.threshold))
    # the same loops with the quaternions as they were give the same rotation: rows 3, 4, 5 within TAU of the plain case's
    plain = _run(eng, c)
    keep = np.ones(40, bool); keep[:3] = False
    sub = np.ix_(keep, keep)
    assert np.allclose(r.d2[sub], plain.d2[sub], rtol=pc.TAU["mixed"] * 2, atol=pc.TAU["mixed"] * 2)


def test_no_odometry_variance_is_zeros(eng):
    c, _ = pc.case_and_d2("mixed", 40)
    a = _run(eng, c, odom=None); b = _run(eng, c, odom=np.zeros(6))
    assert np.array_equal(_bits(a.d2), _bits(b.d2)) and np.array_equal(a.words, b.words)


def test_zero_covariances_are_infinitely_far(eng):
    c, _ = pc.case_and_d2("mixed", 3)
    cov = c.cov.copy(); cov[0] = 0.0; cov[1] = 0.0
    r = _run(eng, c._replace(cov=cov), odom=None, threshold=1e300)
    assert np.isinf(r.d2[0, 1]) and not r.adj[0, 1] and r.adj[0, 2] and r.adj[1, 2]


def test_thresholds_zero_everything_and_exactly_one_pairs_d2(eng):
    c, exact = pc.case_and_d2("mixed", 40)
    assert not _run(eng, c, threshold=0.0).adj.any()
    full = _run(eng, c, threshold=1e300)
    assert np.array_equal(full.adj, ~np.eye(40, dtype=bool)) and (full.degree == 39).all()
    mem, seed = eng.pcm_max_clique(full.words)
    assert mem.tolist() == list(range(40)) and seed == 0
    v = float(full.d2[3, 17])
    r = _run(eng, c, threshold=v)
    assert r.adj[3, 17] and r.adj[17, 3]                                         # equality is kept
    assert np.array_equal(r.adj, (full.d2 <= v) & ~np.eye(40, dtype=bool))
    assert not _run(eng, c, threshold=np.nextafter(v, 0.0)).adj[3, 17]


# ---- the clique on hand-made graphs -------------------------------------------------------------------------------------------------

def _clique_twice(e, a):
    first = e.pcm_max_clique(a)
    second = e.pcm_max_clique(pcm_bool_to_words(a))
    assert np.array_equal(first[0], second[0]) and first[1] == second[1]
    assert pc.is_clique(a, first[0])
    return tuple(first[0].tolist()), first[1]


@pytest.mark.parametrize("name", sorted(pc.HAND_GRAPHS))
def test_clique_on_the_graphs_with_written_answers(eng, name):
    n, edges, members, seed = pc.HAND_GRAPHS[name]
    a = pc.graph_from_edges(n, edges)
    assert _clique_twice(eng, a) == (members, seed)
    if n <= 24:
        assert len(members) <= pc.max_clique_brute(a)


def test_clique_on_complete_empty_path_and_disjoint_graphs(eng):
    for n in (64, 65):
        assert _clique_twice(eng, ~np.eye(n, dtype=bool)) == (tuple(range(n)), 0)
    assert _clique_twice(eng, np.zeros((4096, 4096), bool)) == ((0,), 0)
    path = pc.graph_from_edges(200, [(i, i + 1) for i in range(199)])
    assert _clique_twice(eng, path) == ((0, 1), 0)
    # two disjoint 30-cliques, the vertices of the second listed first in index order: equal sizes, the lower seed's wins
    first, second = list(range(30, 60)), list(range(0, 30))
    a = pc.graph_from_edges(60, [(i, j) for grp in (first, second) for i in grp for j in grp if i < j])
    assert _clique_twice(eng, a) == (tuple(range(30)), 0)
    a = pc.graph_from_edges(130, [(i, j) for i in range(62, 67) for j in range(i + 1, 67)])
    assert _clique_twice(eng, a) == ((62, 63, 64, 65, 66), 62)


@pytest.mark.parametrize("n,density", [(100, 0.05), (100, 0.5), (100, 0.95), (1000, 0.05), (1000, 0.5), (1000, 0.95), (20, 0.5), (24, 0.7)])
def test_clique_on_random_graphs(eng, n, density):
    rs = np.random.RandomState(int(n * 100 + density * 100))
    a = np.triu(rs.rand(n, n) < density, 1); a = a | a.T
    got = _clique_twice(eng, a)
    assert got == pc.greedy_clique_fast(a)                                      # members, seed: the seed skipping does not show
    if n <= 100:
        assert got == pc.greedy_clique(a)
    if n <= 24:
        assert len(got[0]) <= pc.max_clique_brute(a)


def test_clique_planted_in_noise_at_the_limit(eng):
    n = 4096
    rs = np.random.RandomState(11)
    a = np.triu(rs.rand(n, n) < 0.01, 1)
    members = np.sort(rs.permutation(n)[:40])
    a[np.ix_(members, members)] = True
    a = np.triu(a, 1); a = a | a.T
    got = _clique_twice(eng, a)
    assert got == pc.greedy_clique_fast(a) and set(members.tolist()) <= set(got[0])


# ---- state and errors ------------------------------------------------------------------------------------------------------------------

def test_no_loops(eng):
    c, _ = pc.case_and_d2("mixed", 3)
    e = np.zeros((0,))
    mem, seed, deg = eng.pcm_select(c.poses_a, c.poses_b, np.zeros(0, np.int32), np.zeros(0, np.int32), e.reshape(0, 7), e.reshape(0, 36), 7.8)
    assert len(mem) == 0 and seed == -1 and len(deg) == 0
    mem, seed = eng.pcm_max_clique(np.zeros((0, 0), bool))
    assert len(mem) == 0 and seed == -1
    r = eng.pcm_consistency(c.poses_a, c.poses_b, np.zeros(0, np.int32), np.zeros(0, np.int32), e.reshape(0, 7), e.reshape(0, 36), 7.8)
    assert len(r) == 0


def _raw(e, c, n=None, n_a=None, n_b=None, threshold=None, odom=None, null=(), outs=("d2", "adj", "degree")):
    """scl_pcm_consistency and scl_pcm_select on raw pointers; returns (status of both, whether every output kept its sentinel)"""
    lib = e._lib
    N = len(c.idx_a)
    dp = lambda a: None if a is None else np.ascontiguousarray(a, np.float64).ctypes.data_as(POINTER(c_double))
    ip = lambda a: np.ascontiguousarray(a, np.int32).ctypes.data_as(POINTER(c_int))
    hold = {"poses_a": np.ascontiguousarray(c.poses_a), "poses_b": np.ascontiguousarray(c.poses_b), "z": np.ascontiguousarray(c.z),
            "cov": np.ascontiguousarray(c.cov), "idx_a": np.ascontiguousarray(c.idx_a, np.int32), "idx_b": np.ascontiguousarray(c.idx_b, np.int32)}
    arg = {k: (None if k in null else (ip(v) if k.startswith("idx") else dp(v))) for k, v in hold.items()}
    ov = None if odom is None else np.ascontiguousarray(odom, np.float64)
    d2 = np.full((N, N), 7.0); adj = np.full((N, (N + 63) // 64), 7, np.uint64); deg = np.full(N, 7, np.int32)
    mem = np.full(N, 7, np.int32); nm = c_int(7); seed = c_int(7)
    common = (e._h, arg["poses_a"], len(c.poses_a) if n_a is None else n_a, arg["poses_b"], len(c.poses_b) if n_b is None else n_b,
              arg["idx_a"], arg["idx_b"], arg["z"], arg["cov"], N if n is None else n, dp(ov), c.threshold if threshold is None else threshold)
    rc1 = lib.scl_pcm_consistency(*common, dp(d2) if "d2" in outs else None, adj.ctypes.data_as(POINTER(c_uint64)) if "adj" in outs else None,
                                  ip(deg) if "degree" in outs else None)
    rc2 = lib.scl_pcm_select(*common, None if "members" in null else ip(mem), None if "n_members" in null else byref(nm),
                             None if "seed" in null else byref(seed), ip(deg))
    untouched = (d2 == 7.0).all() and (adj == 7).all() and (deg == 7).all() and (mem == 7).all() and nm.value == 7 and seed.value == 7
    return rc1, rc2, untouched


def test_errors_write_nothing(eng):
    c, _ = pc.case_and_d2("mixed", 40)
    assert _raw(eng, c)[:2] == (0, 0)

    def bad(field, row, col, value):
        a = np.array(getattr(c, field), np.float64).copy()
        a.reshape(len(a), -1)[row, col] = value
        return c._replace(**{field: a})
    idx = c.idx_a.copy(); idx[7] = len(c.poses_a)
    idxn = c.idx_b.copy(); idxn[0] = -1
    q0 = c.z.copy(); q0[5, 3:] *= 0.49
    q4 = c.poses_a.copy(); q4[int(c.idx_a[0]), 3:] *= 2.01
    refused = [
        dict(n=-1), dict(n_a=-1), dict(n_b=-1), dict(null=("poses_a",)), dict(null=("poses_b",)), dict(null=("idx_a",)), dict(null=("idx_b",)),
        dict(null=("z",)), dict(null=("cov",)), dict(threshold=float("nan")), dict(threshold=float("inf")), dict(threshold=-1e-300),
        dict(odom=[0, 0, 0, 0, 0, float("nan")]), dict(odom=[0, -1e-12, 0, 0, 0, 0]), dict(odom=[float("inf")] * 6),
        dict(n_a=int(c.idx_a.max())), dict(n_b=int(c.idx_b.max())),
    ]
    for kw in refused:
        assert _raw(eng, c, **kw) == (INVALID_ARG, INVALID_ARG, True), kw
    for d in (c._replace(idx_a=idx), c._replace(idx_b=idxn), bad("poses_a", 0, 1, np.nan), bad("poses_b", 199, 6, np.inf), bad("z", 39, 0, -np.inf),
              bad("cov", 3, 6 * 1 + 4, np.nan), c._replace(z=q0), c._replace(poses_a=q4)):
        assert _raw(eng, d) == (INVALID_ARG, INVALID_ARG, True)
    assert _raw(eng, bad("cov", 3, 6 * 4 + 1, np.nan))[:2] == (0, 0)           # below the diagonal: never read
    assert _raw(eng, c, outs=())[0] == INVALID_ARG                              # no output asked for
    for name in ("members", "n_members", "seed"):
        assert _raw(eng, c, null=(name,))[1] == INVALID_ARG
    big = pc.Case(c.poses_a, c.poses_b, np.zeros(4097, np.int32), np.zeros(4097, np.int32), np.tile(c.z[0], (4097, 1)), np.tile(c.cov[0], (4097, 1)),
                  None, c.threshold, None, None)
    assert _raw(eng, big, outs=("degree",)) == (INVALID_ARG, INVALID_ARG, True)
    with pytest.raises(SclError):
        _run(eng, c._replace(idx_a=idx))
    # the clique's own refusals
    lib = eng._lib
    mem = np.full(8, 7, np.int32); nm = c_int(7); seed = c_int(7)

    def clique(words, n):
        w = np.ascontiguousarray(words, np.uint64)
        return lib.scl_pcm_max_clique(eng._h, w.ctypes.data_as(POINTER(c_uint64)), n, mem.ctypes.data_as(POINTER(c_int)), byref(nm), byref(seed))
    assert clique([0b010, 0b000, 0b000], 3) == INVALID_ARG                      # not symmetric
    assert clique([0b001, 0b000, 0b000], 3) == INVALID_ARG                      # a diagonal bit
    assert clique([0b1000, 0b000, 0b000], 3) == INVALID_ARG                     # a bit at n
    assert clique([0], -1) == INVALID_ARG
    assert lib.scl_pcm_max_clique(eng._h, None, 3, mem.ctypes.data_as(POINTER(c_int)), byref(nm), byref(seed)) == INVALID_ARG
    assert clique(np.zeros((4097, 65)), 4097) == INVALID_ARG
    assert (mem == 7).all() and nm.value == 7 and seed.value == 7
    assert clique([0b010, 0b001, 0b000], 3) == 0 and (nm.value, seed.value, mem[:2].tolist()) == (2, 0, [0, 1])


def test_sharded_engine_equals_plain(eng):
    c, _ = pc.case_and_d2("mixed", 129)
    sh = ScanContextEngine(initial_capacity=16, devices=[0, 0], exchange=1)
    try:
        a, b = _run(eng, c), _run(sh, c)
        assert np.array_equal(_bits(a.d2), _bits(b.d2)) and np.array_equal(a.words, b.words) and np.array_equal(a.degree, b.degree)
        sa, sb = _select(eng, c), _select(sh, c)
        assert np.array_equal(sa[0], sb[0]) and sa[1] == sb[1]
        ca, cb = eng.pcm_max_clique(a.words), sh.pcm_max_clique(a.words)
        assert np.array_equal(ca[0], cb[0]) and ca[1] == cb[1]
        # the handle the caller holds answers for the shard that did the work: the message of a refusal, the profile switch
        bad = c.idx_a.copy(); bad[0] = -1
        with pytest.raises(SclError, match="index out of range"):
            _run(sh, c._replace(idx_a=bad))
        with pytest.raises(SclError, match="index out of range"):
            _select(sh, c._replace(idx_a=bad))
        with pytest.raises(SclError, match="not symmetric"):
            sh.pcm_max_clique(np.uint64([2, 0]).reshape(2, 1))
        sh.profile_enable(1)
        _select(sh, c)
        assert min(sh.pcm_last_timing()) > 0.0
        sh.profile_enable(0)
    finally:
        sh.close()


def test_timing_is_reported_under_the_profile_switch(eng):
    c, _ = pc.case_and_d2("mixed", 129)
    eng.profile_enable(1)
    try:
        _select(eng, c)
        pairs_ms, clique_ms = eng.pcm_last_timing()
        assert pairs_ms > 0.0 and clique_ms > 0.0
        _run(eng, c)
        assert eng.pcm_last_timing()[1] == 0.0
    finally:
        eng.profile_enable(0)


def test_icp_and_scoring_around_pcm_answer_as_on_a_twin_that_never_ran_it():
    """PCM shares the engine's stream, lock and device with the ICP batch and the registration scoring: with PCM calls before, between
    and after them they give the bits of a twin engine that never ran PCM"""
    isrc, itgts, G = gc.source(), gc.targets()[:3], gc.guesses()[:3]
    src, tgts, Ts, max_dist = rc.case("list")
    c_small, c_big = pc.case("mixed", 129), pc.case("mixed", 1000)
    e, twin = ScanContextEngine(), ScanContextEngine()
    try:
        pp = e.icp_default_params(); pp.max_iterations = 10

        def same(a, b):
            return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) for x, y in zip(a, b))
        sel = _select(e, c_small)
        for _ in range(2):
            icp, icp_t = e.icp_align_batch_guess(isrc, itgts, G, pp), twin.icp_align_batch_guess(isrc, itgts, G, pp)
            assert same(icp[:5], icp_t[:5])
            big = _run(e, c_big)
            ev, ev_t = e.registration_eval_batch(src, tgts, Ts, max_dist), twin.registration_eval_batch(src, tgts, Ts, max_dist)
            assert same((ev.n_valid, ev.n_inliers, ev.moments), (ev_t.n_valid, ev_t.n_inliers, ev_t.moments)) and ev.n_inliers.any()
            again = _select(e, c_small)
            assert np.array_equal(again[0], sel[0]) and again[1] == sel[1]
        assert np.array_equal(big.adj, pc.graph(pc.case_and_d2("mixed", 1000)[1], c_big.threshold))
    finally:
        e.close(); twin.close()


def _pose7(M):
    """x, y, z, qx, qy, qz, qw of a 4 x 4 rigid motion"""
    R = np.asarray(M, np.float64)[:3, :3]
    K = np.array([[R[0, 0] - R[1, 1] - R[2, 2], 0, 0, 0], [R[0, 1] + R[1, 0], R[1, 1] - R[0, 0] - R[2, 2], 0, 0],
                  [R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], R[2, 2] - R[0, 0] - R[1, 1], 0],
                  [R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], R[0, 0] + R[1, 1] + R[2, 2]]]) / 3.0
    w, v = np.linalg.eigh(K, UPLO="L")
    q = v[:, np.argmax(w)]
    return np.concatenate([np.asarray(M, np.float64)[:3, 3], q if q[3] >= 0 else -q])


def test_the_chain_from_search_to_select_rejects_a_wrong_loop():
    """Two robots on the 20 x 60 grid (the chain of tests/test_gpu_registration_eval.py, five places): per place the inter-robot
    search, the guess from its shift, the guessed ICP from the store, the scoring at the returned T, scl_loop_pose_between and
    scl_loop_covariance(info, s2) as INTEGRATION.md 3c writes them; then scl_pcm_select over the five loops with one between-pose
    replaced by a wrong one (3 m, 0.5 rad).  The wrong loop is not a member, the right ones are.  The odometry term (1 mrad and 1 cm per
    keyframe step) stands for what the pair-count covariance of an ICP does not know: its own error of a millimetre or so."""
    K, sectors = 5, (7, 3, 11, 0, 5)
    W = rigid_transform(0.01, -0.02, 0.7, 40.0, -25.0, 0.5)              # robot 1's world frame in robot 0's
    odom_var = [1e-6] * 3 + [1e-4] * 3
    e = ScanContextEngine(num_ring=20, num_sector=60)
    try:
        clouds = [synth_scan(20000, seed=7 + 10 * k) for k in range(K)]
        poses_pre = [np.float32([14.0 + 9 * k, -6.5 + 4 * k, 0.4 - 0.1 * k, 0.02, -0.015, 1.1 + 0.3 * k]) for k in range(K)]
        for k in range(K):                                                # robot 0: descriptors and clouds, sensor frame
            e.make_and_save(clouds[k], 0, k)
            e.keyframe_put(0, k, clouds[k])
        poses_a, poses_b, zs, covs = [], [], [], []
        for k in range(K):
            Rz = rigid_transform(0.0, 0.0, np.radians(6.0 * sectors[k]), 0, 0, 0)
            M_pre = gc.pose_matrix(poses_pre[k])
            pose_cur = np.float32(e.matrix_to_pose(np.linalg.inv(W) @ M_pre @ np.linalg.inv(Rz)))   # what robot 1 believes of its keyframe
            M_cur = gc.pose_matrix(pose_cur)
            turned = clouds[k].copy()
            turned[:, :3] = (clouds[k][:, :3].astype(np.float64) @ Rz[:3, :3].T).astype(np.float32)
            received = turned.copy()
            xyz = turned[:, :3].astype(np.float64) @ M_cur[:3, :3].T + M_cur[:3, 3]
            received[:, :3] = (xyz + gc.NOISE * np.random.RandomState(90 + k).standard_normal(xyz.shape)).astype(np.float32)
            e.make_and_save(turned, 1, k)                                 # key K + k
            ids, shifts, dists, found = e.sc_search_inter([K + k], 2, robot_pre=0)
            assert found[0] >= 1 and e.get_index(int(ids[0, 0])) == (0, k) and shifts[0, 0] == sectors[k]
            G = e.loop_guess_from_shift(int(shifts[0, 0]), 60, pose_cur, poses_pre[k])[None]
            args = (received, gc.E2E_LEAF, 0, [k], 0, M_pre.astype(np.float32).reshape(1, 1, 4, 4), gc.E2E_LEAF)
            icp = e.icp_align_batch_from_store_guess(*args, G)
            ev = e.registration_eval_batch_from_store(*args, icp[0], 0.5)
            assert ev.overlap[0] > 0.9
            info = ev.information(0)
            s2 = ev.moments[0, 9] / max(1, int(ev.n_inliers[0]) - 6)
            cov = ScanContextEngine.loop_covariance(info, s2)
            assert np.abs(cov @ info / s2 - np.eye(6)).max() <= 64 * 2.0 ** -53 * np.linalg.cond(info)
            zs.append(e.loop_pose_between(icp[0][0], pose_cur, poses_pre[k])[0]); covs.append(cov)
            poses_a.append(_pose7(M_cur)); poses_b.append(_pose7(M_pre))
        idx = np.arange(K, dtype=np.int32)
        case = pc.Case(np.array(poses_a), np.array(poses_b), idx, idx, np.array(zs), np.array(covs).reshape(K, 36), np.array(odom_var),
                       pc.THRESHOLD, None, None)
        right = _run(e, case)
        print("d2 of the five right loops:\n", right.d2)
        assert right.adj.sum() == K * (K - 1)                             # the right loops agree with each other
        wrong = 2
        z = case.z.copy()
        z[wrong] = pc.compose(z[wrong], np.concatenate([[3.0, 0.0, 0.0], pc.rotvec_to_quat([0.0, 0.0, 0.5])]))
        case = case._replace(z=z)
        exact = pc.d2_exact(case)
        got = _run(e, case)
        assert (np.abs(got.d2 - exact) <= pc.TAU["far"] * np.maximum(1.0, exact)).all()       # conditioning inside the families' range
        assert np.array_equal(got.adj, pc.graph(exact, case.threshold))
        mem, seed, deg = _select(e, case)
        assert mem.tolist() == [k for k in range(K) if k != wrong] and seed == 0 and deg[wrong] == 0
    finally:
        e.close()
