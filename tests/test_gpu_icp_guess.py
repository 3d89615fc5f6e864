"""scl_icp_align_batch_guess, scl_loop_icp_batch_from_store_guess and scl_icp_align_batch_from_store_guess (csrc/icp.hip: the batched
ICP with a source and a working order per candidate; include/scl_engine.h "THE BATCHED ICP WITH INITIAL GUESSES") on the list of
tests/icp_guess_cases.py, which tests/test_icp_guess_cases.py pins on the CPU checker.

Bars.  T_icp, fitness, converged and iterations of entry c are scl_icp_align's for (scl_transform_cloud(src, G_c), tgt_c), compared
as uint32 -- on a twin engine for the list, on the same engine elsewhere.  The pairs of icp_guess_cases.CHECKED are held to the
checker as tests/test_gpu_icp_params.py holds its cases: equal converged and iterations, |T_icp - T_o|max < TOL = 1e-5, fitness within
FIT_REL.  T is the double product T_icp * G_c restated with Python scalars in the header's order, bit for bit."""
import functools
from ctypes import POINTER, byref, c_float, c_int, c_void_p

import numpy as np
import pytest

import icp_guess_cases as gc
import icp_param_cases as pc
import verification_guess_cases as vg
from scl_slam_amd import ScanContextEngine
from scl_slam_amd.synth import rigid_transform
from test_gpu_verification_batch import KEYS40, LEAF, N_KF, SN, SRC_LEAF, _fill_store, _windows

pytestmark = pytest.mark.gpu
INVALID_ARG = -1                                                      # include/scl_engine.h
IDENT = np.eye(4, dtype=np.float32)
KEY_CUR = 4                                                           # the loop form's scan: keyframe 4 of the store's world


@pytest.fixture(scope="module")
def eng():
    e = ScanContextEngine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def twin():
    """an engine that never runs a guessed call: the single calls the list is held to"""
    e = ScanContextEngine()
    yield e
    e.close()


def _params(e, pname_or_fields):
    return pc.engine_params(e, gc.PARAMS[pname_or_fields] if isinstance(pname_or_fields, str) else pname_or_fields)


def _singles(e, src, tgts, G, p):
    """the definition: scl_icp_align on the source moved by the candidate's guess"""
    return [e.icp_align(e.transform_cloud(src, g) if len(src) else src, t, p) for t, g in zip(tgts, G)]


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def _assert_entries(got, singles, G, gated=None):
    T, Ti, fit, cv, it = got[:5]
    assert T.shape == Ti.shape == (len(singles), 4, 4) and len(fit) == len(cv) == len(it) == len(singles)
    for c, (T1, f1, c1, i1) in enumerate(singles):
        assert (bool(cv[c]), int(it[c])) == (bool(c1), int(i1)), (c, cv[c], it[c], c1, i1)
        assert _same_bits(Ti[c], T1) and _same_bits(fit[c], f1), (c, Ti[c], T1, fit[c], f1)
        want = IDENT if gated is not None and gated[c] else gc.compose(Ti[c], G[c])
        assert np.array_equal(T[c], want, equal_nan=True) and (np.isnan(want).any() or _same_bits(T[c], want)), c


# ---- the list: every entry against the twin and the checker -----------------------------------------------------------------------
@pytest.mark.parametrize("pname", list(gc.PARAMS))
def test_whole_list_against_the_twin_and_the_checker(eng, twin, pname):
    src, tgts, G = gc.source(), gc.targets(), gc.guesses()
    got = eng.icp_align_batch_guess(src, tgts, G, _params(eng, pname))
    _assert_entries(got, _singles(twin, src, tgts, G, _params(twin, pname)), G)
    est = gc.PARAMS[pname].get("estimator", 0)
    for name, p in gc.CHECKED:
        if p != pname:
            continue
        k = gc.NAMES.index(name)
        To, fo, co, io = gc.oracle(name, pname)
        print(pname, name, "gpu", (bool(got[3][k]), int(got[4][k])), "checker", (co, io), "|dT|", np.abs(got[1][k] - To).max(),
              "fitness", got[2][k], fo)
        assert (bool(got[3][k]), int(got[4][k])) == (co, io)
        assert np.abs(got[1][k] - To).max() < gc.TOL
        assert abs(got[2][k] - fo) <= gc.FIT_REL[est] * max(1e-6, abs(fo)) + 1e-12
        if (name, p) in gc.YAWED:                                     # what the guess is for, on the device
            assert got[3][k] and got[2][k] < gc.FITNESS_MAX and np.abs(got[0][k] - gc.TRUE[name]).max() < gc.T_TRUE_TOL
    if pname == "mcd0.5":
        k = gc.NAMES.index("far")
        want = G[k].copy(); want[3] = (0, 0, 0, 1)
        assert (bool(got[3][k]), int(got[4][k])) == (False, 0) and _same_bits(got[1][k], IDENT) and _same_bits(got[0][k], want)


# ---- candidate counts: the rounds of 32 --------------------------------------------------------------------------------------------
def _distinct(n):
    """n candidates over the list's clouds at 3 000 points, every guess its own"""
    order = [c % len(gc.NAMES) for c in range(n)]
    G = np.stack([(rigid_transform(0, 0, np.radians(0.02 * c), 0.003 * c, -0.002 * c, 0) @ gc.guesses()[order[c]].astype(np.float64)).astype(np.float32)
                  for c in range(n)]) if n else np.zeros((0, 4, 4), np.float32)
    return [np.ascontiguousarray(gc.targets()[k][::2]) for k in order], G


@pytest.mark.parametrize("n", [0, 1, 2, 32, 33])
def test_candidate_counts_with_distinct_guesses(eng, n):
    """600 sources against 3 000-point targets; 33 candidates: the second round reuses the tables, with the 33rd guess"""
    src = np.ascontiguousarray(gc.source()[::5])
    tgts, G = _distinct(n)
    assert len(src) == 600 and len({g.tobytes() for g in G}) == n
    p = _params(eng, {"max_iterations": 12})
    got = eng.icp_align_batch_guess(src, tgts, G, p)
    assert got[0].shape == got[1].shape == (n, 4, 4)
    _assert_entries(got, _singles(eng, src, tgts, G, p), G)
    if n == 33:
        assert not _same_bits(got[1][32], got[1][2]) and bool(got[3][1]) and bool(got[3][31])


# ---- source sizes -------------------------------------------------------------------------------------------------------------------
def _long_source(n):
    s = gc.source()
    parts = [s.copy() for _ in range((n + len(s) - 1) // len(s))]
    for k, part in enumerate(parts):
        part[:, 0] += np.float32(0.013 * k)
    return np.ascontiguousarray(np.concatenate(parts)[:n])


@pytest.mark.parametrize("n_cand", [1, 3])
@pytest.mark.parametrize("n_src", [0, 1, 2, 3, 255, 256, 257, 4097])
def test_source_sizes(eng, n_src, n_cand):
    """around the early exits (fewer than three pairs), one workgroup of the streaming kernels and of the tile search (kTileQ = 256),
    and a source of several sort tiles"""
    src = _long_source(n_src) if n_src else gc.source()[:0]
    idx = [gc.NAMES.index(n) for n in ("yaw90", "near", "yaw180")][:n_cand]
    tgts, G = [gc.targets()[k] for k in idx], gc.guesses()[idx]
    p = _params(eng, {"max_iterations": 12})
    got = eng.icp_align_batch_guess(src, tgts, G, p)
    _assert_entries(got, _singles(eng, src, tgts, G, p), G)
    if n_src < 3:
        assert not got[3].any() and _same_bits(got[1], np.broadcast_to(IDENT, got[1].shape))
        assert _same_bits(got[0][:, :3], G[:, :3]) and _same_bits(got[0][:, 3], IDENT[[3] * n_cand])
    if n_src >= 255:
        assert got[3].all()


# ---- search paths: tiles, no tiles, two parts ----------------------------------------------------------------------------------------
def _far_frames(c):
    """the tile case's source against its targets, every target in a frame of its own (yaws 47 degrees apart, tens of metres), the
    guess that frame behind a small error; the far candidate is the matching place with a guess 50 m too high"""
    tgts, G = [], []
    for k, t in enumerate(c.tgts):
        M = rigid_transform(0.0, 0.0, np.radians(47.0 * k), 11.0 * k, -7.0 * k, 0.2 * k)
        E = rigid_transform(0.0, 0.0, np.radians(0.02), 0.02, -0.01, 0.005 * k)
        if k == c.far:
            t, E = c.tgts[0], rigid_transform(0, 0, 0, 0, 0, pc.FAR_SHIFT)
        tgts.append(np.ascontiguousarray(gc.moved(t, M)))
        G.append((E @ M).astype(np.float32))
    return tgts, np.stack(G)


TILE_CASES = ("tile1-300000-p2p", "tile1-299995-p2p", "tile2-far_in_part0-p2p", "tile2-far_in_part1-p2p", "tile2-far_in_part1-plane")


@pytest.mark.parametrize("name", TILE_CASES)
def test_search_paths_equal_one_by_one(eng, name):
    """5 x 60 000 queries (= kTileMinQueries: tiles), 5 x 59 999 (memory), 8 x 75 000 (two parts), under a 0.5 m rejection distance: the
    far candidate fails in its part's first solve, in part 0 or in part 1, and the others end where their single calls end"""
    c = pc.case(name)
    tgts, G = _far_frames(c)
    p = pc.engine_params(eng, pc.fields(c))
    got = eng.icp_align_batch_guess(c.src, tgts, G, p)
    singles = _singles(eng, c.src, tgts, G, p)
    print(name, [(bool(a), int(b)) for a, b in zip(got[3], got[4])])
    _assert_entries(got, singles, G)
    assert (bool(got[3][c.far]), int(got[4][c.far])) == (False, 0) and _same_bits(got[1][c.far], IDENT)
    assert bool(got[3][0]) and int(got[4][0]) > 1                    # (the place itself goes on while the far candidate has ended)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [3, 4, 8])
def test_record_strides(eng, twin, width):
    src = np.ascontiguousarray(gc.source()[:, :width])
    tgts = [np.ascontiguousarray(t[:, :width]) for t in gc.targets()]
    G = gc.guesses()
    got = eng.icp_align_batch_guess(src, tgts, G, _params(eng, "p2p"))
    _assert_entries(got, _singles(eng, src, tgts, G, _params(eng, "p2p")), G)
    _assert_entries(got, _singles(twin, gc.source(), gc.targets(), G, _params(twin, "p2p")), G)   # the fields behind z play no part


def test_points_that_overflow_only_after_the_move_and_a_nan_source(eng):
    """a finite point times 1e38 is infinite, and a NaN source stays NaN: such rows are unmatched, as in the single call"""
    src = gc.source().copy()
    src[7, 1] = np.nan
    tgts, G = gc.targets()[:3], gc.guesses()[:3].copy()
    G[1] = np.diag([1e38, 1.0, 1.0, 1.0]).astype(np.float32)
    p = _params(eng, {"max_iterations": 12})
    got = eng.icp_align_batch_guess(src, tgts, G, p)
    singles = _singles(eng, src, tgts, G, p)
    _assert_entries(got, singles, G)
    moved = eng.transform_cloud(src, G[1])
    still = int(np.isfinite(moved[:, :3]).all(1).sum())
    assert 0 < still < len(src) - 1
    assert bool(got[3][0]) and bool(got[3][2])                       # the NaN row adds to no sum of the others


# ---- identity guesses: the unguessed calls -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname", ["p2p", "plane"])
def test_identity_guesses_equal_the_unguessed_batch(eng, pname):
    src, tgts = gc.source(), [gc.targets()[0], np.ascontiguousarray(gc.targets()[0][::2]), gc.targets()[1]]
    p = _params(eng, dict(gc.PARAMS[pname], max_iterations=15))
    plain = eng.icp_align_batch(src, tgts, p)
    got = eng.icp_align_batch_guess(src, tgts, np.broadcast_to(IDENT, (3, 4, 4)), p)
    assert _same_bits(got[1], plain[0]) and _same_bits(got[2], plain[1]) and np.array_equal(got[3], plain[2]) and np.array_equal(got[4], plain[3])
    assert _same_bits(got[0], got[1])                                 # T == T_icp


# ---- the store forms ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def store():
    e = ScanContextEngine()
    received = _fill_store(e)
    yield e, received
    e.close()


def _store_guesses(n):
    """small motions, every eighth a wrong 30 degrees; all distinct"""
    return np.stack([rigid_transform(0, 0, np.radians(30.0 if c % 8 == 5 else 0.02 * c), 0.002 * c, -0.001 * c, 0).astype(np.float32)
                     for c in range(n)]) if n else np.zeros((0, 4, 4), np.float32)


def _store_singles(e, src, keys, G, p, min_src_points, min_tgt_points):
    """scl_icp_align(scl_transform_cloud(source, G_c), scl_submap_from_store(key_c, ...)) behind the size gate -> (singles, gated, n_tgts)"""
    subs, out, gated, nt = {}, [], [], []
    for k, g in zip(keys, G):
        if k not in subs:
            subs[k] = e.submap_from_store(0, int(k), SN, _windows([k])[0], LEAF, N_KF * 12000)
        sub = subs[k]
        nt.append(len(sub))
        gated.append(len(src) < min_src_points or len(sub) < min_tgt_points)
        out.append((IDENT, 0.0, False, 0) if gated[-1] else e.icp_align(e.transform_cloud(src, g), sub, p))
    return out, gated, nt


@pytest.mark.parametrize("form", ["loop", "received"])
def test_store_forms_forty_candidates(store, form):
    """two rounds from a store of two robots, keys at both ends of the trajectory and beyond; a min_tgt_points between the submaps'
    sizes, a min_src_points that gates all, and no candidate at all"""
    e, received = store
    G = _store_guesses(40)
    p = _params(e, {"max_iterations": 12})
    if form == "loop":
        src = e.submap_from_store(0, KEY_CUR, 0, [IDENT], LEAF, 12000)
        call = functools.partial(e.loop_icp_batch_from_store_guess, 0, KEY_CUR, IDENT)
    else:
        src = e.voxel_grid(received, SRC_LEAF)
        call = functools.partial(e.icp_align_batch_from_store_guess, received, SRC_LEAF, 0)
    got = call(KEYS40, SN, _windows(KEYS40), LEAF, G, p, min_src_points=300, min_tgt_points=1000)
    singles, gated, nt = _store_singles(e, src, KEYS40, G, p, 300, 1000)
    _assert_entries(got, singles, G, gated)
    assert got[5] == len(src) >= 300 and [int(x) for x in got[6]] == nt and got[3].any()
    sizes = sorted(set(nt))
    cut = sizes[len(sizes) // 2]                                      # gates the candidates with the smaller submaps only
    some = call(KEYS40, SN, _windows(KEYS40), LEAF, G, p, min_src_points=300, min_tgt_points=cut)
    singles, gated, _ = _store_singles(e, src, KEYS40, G, p, 300, cut)
    _assert_entries(some, singles, G, gated)
    small = np.asarray(gated)
    assert small.any() and not small.all() and np.array_equal(some[6], got[6])
    assert _same_bits(some[0][small], np.broadcast_to(IDENT, some[0][small].shape)) and _same_bits(some[1][small], some[0][small])
    assert not some[3][small].any() and not some[2][small].any() and not some[4][small].any()
    none = call(KEYS40, SN, _windows(KEYS40), LEAF, G, p, min_src_points=10 ** 7, min_tgt_points=1000)
    assert _same_bits(none[0], np.broadcast_to(IDENT, none[0].shape)) and _same_bits(none[1], none[0]) and not none[3].any()
    assert none[5] == got[5] and np.array_equal(none[6], got[6])
    empty = call([], SN, _windows([]), LEAF, _store_guesses(0), p)
    assert empty[0].shape == empty[1].shape == (0, 4, 4) and empty[5] == got[5]


def test_identity_guesses_equal_the_unguessed_loop_form(store):
    e, _ = store
    keys = [3, 6, 10, 1, 13]
    p = _params(e, {"max_iterations": 15})
    plain = e.loop_icp_batch_from_store(0, KEY_CUR, IDENT, keys, SN, _windows(keys), LEAF, p)
    got = e.loop_icp_batch_from_store_guess(0, KEY_CUR, IDENT, keys, SN, _windows(keys), LEAF, np.broadcast_to(IDENT, (5, 4, 4)), p)
    assert _same_bits(got[1], plain[0]) and _same_bits(got[2], plain[1]) and _same_bits(got[0], got[1])
    assert np.array_equal(got[3], plain[2]) and np.array_equal(got[4], plain[3]) and got[5] == plain[4] and np.array_equal(got[6], plain[5])
    assert plain[2].any()


# ---- state ------------------------------------------------------------------------------------------------------------------------------
def test_other_calls_around_a_guessed_call():
    """an unguessed batch, a guessed verification batch and scl_nn_correspondences before and after guessed ICP batches answer what a
    twin engine that never ran one answers; a larger guessed call after a smaller one regrows the tables"""
    src, tgts, G = gc.source(), gc.targets(), gc.guesses()
    big = _long_source(5000)
    out = []
    for guessed in (False, True):
        e = ScanContextEngine()
        try:
            p = _params(e, {"max_iterations": 12})
            if guessed:
                small = e.icp_align_batch_guess(src[:700], tgts[:2], G[:2], p)
                _assert_entries(small, _singles(e, src[:700], tgts[:2], G[:2], p), G[:2])
                large = e.icp_align_batch_guess(big, tgts, G, p)
                _assert_entries(large, _singles(e, big, tgts, G, p), G)
            a = e.icp_align_batch(src, tgts[:3], p)
            b = e.geometric_verification_batch_guess(vg.source()[0], vg.clouds(), vg.guesses(), 9, vg.THRESHOLD, vg.RATIO, vg.SEED)
            c = e.nn_correspondences(src, tgts[0])
            out.append((a, b, c))
        finally:
            e.close()
    (a0, b0, c0), (a1, b1, c1) = out
    assert _same_bits(a0[0], a1[0]) and _same_bits(a0[1], a1[1]) and np.array_equal(a0[2], a1[2]) and np.array_equal(a0[3], a1[3])
    assert _same_bits(b0[0], b1[0]) and _same_bits(b0[4], b1[4]) and all(np.array_equal(b0[i], b1[i]) for i in (1, 2, 3))
    assert np.array_equal(c0[0], c1[0]) and _same_bits(c0[1], c1[1])


# ---- errors write nothing ---------------------------------------------------------------------------------------------------------------
def _fp(a):
    return a.ctypes.data_as(POINTER(c_float))


def _ip(a):
    return a.ctypes.data_as(POINTER(c_int))


def _outputs(n):
    k = max(n, 1)
    return [np.full((k, 16), 7.0, np.float32), np.full((k, 16), 7.0, np.float32), np.full(k, 7.0, np.float32), np.full(k, 7, np.int32),
            np.full(k, 7, np.int32)]


def _raw_host(e, src, tgts, G, stride=None, n=None, null_T=False, null_target=None, n_src=None, null_G=False, null_p=False, null_src=False, **fields):
    s = np.ascontiguousarray(src, np.float32)
    arrs = [np.ascontiguousarray(t, np.float32) for t in tgts]
    ptrs = (c_void_p * max(1, len(arrs)))(*[a.ctypes.data for a in arrs])
    if null_target is not None:
        ptrs[null_target] = None
    counts = np.asarray([len(a) for a in arrs] or [0], np.int32)
    g = np.ascontiguousarray(G, np.float32)
    p = pc.engine_params(e, fields)
    out = _outputs(len(arrs))
    rc = e._lib.scl_icp_align_batch_guess(e._h, None if null_src else s.ctypes.data_as(c_void_p), len(s) if n_src is None else n_src, ptrs, _ip(counts),
                                          len(arrs) if n is None else n, s.shape[1] * 4 if stride is None else stride, None if null_G else _fp(g),
                                          None if null_p else byref(p), None if null_T else _fp(out[0]), _fp(out[1]), _fp(out[2]), _ip(out[3]), _ip(out[4]))
    return rc, all((o == 7).all() for o in out)


def _raw_store(e, form, received, robot, keys, sn, G, stride=None, n=None, null_T=False, null_G=False, null_p=False, null_pose=False, src_leaf=SRC_LEAF,
               leaf=LEAF, **fields):
    s = np.ascontiguousarray(received, np.float32)
    k = np.asarray(keys, np.int32)
    poses = _windows(keys, sn).astype(np.float32).reshape(-1)
    g = np.ascontiguousarray(G, np.float32)
    p = pc.engine_params(e, fields)
    out = _outputs(len(k)) + [np.full(max(len(k), 1), 7, np.int32)]
    ns = c_int(7)
    m = len(k) if n is None else n
    tail = (None if null_G else _fp(g), None if null_p else byref(p), 300, 1000, None if null_T else _fp(out[0]), _fp(out[1]), _fp(out[2]), _ip(out[3]),
            _ip(out[4]), byref(ns), _ip(out[5]))
    if form == "loop":
        pose = np.ascontiguousarray(IDENT).reshape(16)
        rc = e._lib.scl_loop_icp_batch_from_store_guess(e._h, robot, KEY_CUR if robot == 0 else 0, None if null_pose else _fp(pose), m, _ip(k), sn, _fp(poses),
                                                        leaf, *tail)
    else:
        rc = e._lib.scl_icp_align_batch_from_store_guess(e._h, s.ctypes.data_as(c_void_p), len(s), s.shape[1] * 4 if stride is None else stride, src_leaf,
                                                         robot, m, _ip(k), sn, _fp(poses), leaf, *tail)
    return rc, all((o == 7).all() for o in out) and ns.value == 7


def _bad_guesses(G):
    for c, r, k, v in ((0, 0, 0, np.nan), (len(G) - 1, 2, 3, np.inf), (1 % len(G), 1, 2, -np.inf)):
        B = G.copy(); B[c, r, k] = v
        yield B


def test_errors_write_nothing(store):
    e, received = store
    src, tgts, G = gc.source(), gc.targets()[:3], gc.guesses()[:3]
    G2 = _store_guesses(2)
    bad_params = (dict(estimator=7), dict(estimator=1, normal_radius=0.0), dict(max_iterations=0))
    assert _raw_host(e, src, tgts, G, null_G=True) == (INVALID_ARG, True)
    for B in _bad_guesses(G):
        assert _raw_host(e, src, tgts, B) == (INVALID_ARG, True)
    for kw in (dict(null_T=True), dict(n=-1), dict(stride=10), dict(stride=14), dict(stride=8), dict(null_target=1), dict(n_src=-1), dict(null_p=True),
               dict(null_src=True)) + bad_params:
        assert _raw_host(e, src, tgts, G, **kw) == (INVALID_ARG, True), kw
    for form in ("loop", "received"):
        assert _raw_store(e, form, received, 0, [3, 5], SN, G2, null_G=True) == (INVALID_ARG, True), form
        for B in _bad_guesses(G2):
            assert _raw_store(e, form, received, 0, [3, 5], SN, B) == (INVALID_ARG, True), form
        for kw in (dict(null_T=True), dict(n=-1), dict(null_p=True), dict(leaf=0.0)) + bad_params:
            assert _raw_store(e, form, received, 0, [3, 5], SN, G2, **kw) == (INVALID_ARG, True), (form, kw)
        assert _raw_store(e, form, received, 1, [0, 1, 0], 0, _store_guesses(3)) == (INVALID_ARG, True)   # keyframe 1 of robot 1 was never stored
        assert _raw_store(e, form, received, 1, [0, 2, 2], 1, _store_guesses(3)) == (INVALID_ARG, True)   # ... and lies inside these windows
    assert _raw_store(e, "loop", received, 0, [3, 5], SN, G2, null_pose=True) == (INVALID_ARG, True)
    for kw in (dict(stride=16), dict(stride=12), dict(src_leaf=0.0)):                                       # (the store's records are 32 bytes)
        assert _raw_store(e, "received", received, 0, [3, 5], SN, G2, **kw) == (INVALID_ARG, True), kw
    # a non-finite LAST row is not read; no candidate needs no guesses
    L = G.copy(); L[:, 3] = np.nan
    rc, untouched = _raw_host(e, src, tgts, L, max_iterations=3)
    assert rc == 0 and not untouched
    assert _raw_host(e, src, [], np.zeros((0, 4, 4)), null_G=True) == (0, True)
    rc, untouched = _raw_store(e, "received", received, 1, [0, 2], 0, G2, max_iterations=3)
    assert rc == 0 and not untouched
    p = _params(e, {"max_iterations": 12})                                                                  # and the engine afterwards
    _assert_entries(e.icp_align_batch_guess(src, tgts, G, p), _singles(e, src, tgts, G, p), G)


# ---- two shards ----------------------------------------------------------------------------------------------------------------------------
def test_sharded_engine_equals_plain(store):
    """a 2-shard engine on one device: candidate c of the host form runs on shard c mod 2 with its own guess; the store forms run on the
    shard that owns the keyframe store"""
    e, received = store
    sh = ScanContextEngine(devices=[0, 0], exchange=1)
    try:
        _fill_store(sh)
        keys, G7 = KEYS40[:7], _store_guesses(7)
        p, ps = _params(e, {"max_iterations": 12}), _params(sh, {"max_iterations": 12})
        a = sh.icp_align_batch_guess(gc.source(), gc.targets(), gc.guesses(), ps)
        b = e.icp_align_batch_guess(gc.source(), gc.targets(), gc.guesses(), p)
        assert all(_same_bits(a[i], b[i]) for i in (0, 1, 2)) and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])
        assert len({t.tobytes() for t in a[1]}) >= 4
        for call_s, call_e in ((functools.partial(sh.loop_icp_batch_from_store_guess, 0, KEY_CUR, IDENT), functools.partial(e.loop_icp_batch_from_store_guess, 0, KEY_CUR, IDENT)),
                               (functools.partial(sh.icp_align_batch_from_store_guess, received, SRC_LEAF, 0), functools.partial(e.icp_align_batch_from_store_guess, received, SRC_LEAF, 0))):
            a = call_s(keys, SN, _windows(keys), LEAF, G7, ps)
            b = call_e(keys, SN, _windows(keys), LEAF, G7, p)
            assert all(_same_bits(a[i], b[i]) for i in (0, 1, 2)) and all(np.array_equal(a[i], b[i]) for i in (3, 4, 6)) and a[5] == b[5]
    finally:
        sh.close()


# ---- end to end on 20 x 60: search -> shift -> guess -> verification -> ICP ------------------------------------------------------------
def test_search_guess_verification_icp_end_to_end():
    """Two robots.  The ranked inter-robot search reports the shift, scl_loop_guess_from_shift turns it and the two poses into the guess,
    the guessed verification answers T, and T is the guess of the received form: the true candidate ends with fitness < 0.3 and
    |T - T_true|max < 5e-3 (tests/test_icp_guess_cases.py shows that the checker meets both on this input).  The same chain from
    identity guesses does not."""
    cloud, other, turned, received, T_true = gc.end_to_end()
    e = ScanContextEngine(num_ring=20, num_sector=60)
    try:
        M_pre = gc.pose_matrix(gc.POSE_PRE).astype(np.float32)
        for k, c in enumerate((other, cloud)):                         # robot 0's keyframes: descriptors and clouds, sensor frame
            e.make_and_save(c, 0, k)
            e.keyframe_put(0, k, c)
        e.make_and_save(turned, 1, 0)                                 # the received keyframe's descriptor: key 2
        ids, shifts, dists, found = e.sc_search_inter([2], 2, robot_pre=0)
        print("search", ids, shifts, dists, found)
        assert found[0] == 2 and ids[0, 0] == 1 and shifts[0, 0] == gc.SECTORS_TURNED
        index = [e.get_index(int(i)) for i in ids[0]]
        assert index[0] == (0, 1) and index[1] == (0, 0)
        keys = [int(i[1]) for i in index]
        G = np.stack([e.loop_guess_from_shift(int(shifts[0, j]), 60, gc.POSE_CUR, gc.POSE_PRE if keys[j] == 1 else np.zeros(6)) for j in range(2)])
        windows = np.stack([M_pre if k == 1 else IDENT for k in keys]).reshape(2, 1, 4, 4)
        args = (received, gc.E2E_LEAF, 0, keys, 0, windows, gc.E2E_LEAF)
        out = {}
        for name, g in (("guess", G), ("identity", np.broadcast_to(IDENT, (2, 4, 4)))):
            ver = e.geometric_verification_batch_from_store_guess(*args, g, 300, 0.25, 0.45, 1)
            got = e.icp_align_batch_from_store_guess(*args, ver[0])
            err = np.abs(got[0][0].astype(np.float64) - T_true).max()
            print(name, "verified", ver[1], "inliers", ver[5], "icp", got[3], got[4], "fitness", got[2], "|T - T_true|", err)
            assert _same_bits(got[0][0], gc.compose(got[1][0], ver[0][0]))
            out[name] = (ver[1][0], got[3][0], got[2][0], err)
        ok, cv, f, err = out["guess"]
        assert ok and cv and f < gc.FITNESS_MAX and err < gc.T_TRUE_TOL
        ok, cv, f, err = out["identity"]
        assert not (f < gc.FITNESS_MAX and err < gc.T_TRUE_TOL)
    finally:
        e.close()
