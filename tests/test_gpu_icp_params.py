"""ICP off its defaults: GPU (through the C ABI) vs the CPU restatement with the rejection distance and the two stop epsilons of
scl_icp_params moved, on the inputs of tests/icp_param_cases.py (tests/test_icp_param_cases.py proves those sensitive to the field they
move and off every knife edge, with the checker alone).
Bar: converged and iterations equal, |T_gpu - T_oracle|max < 1e-5, fitness within 1e-5 (point to point) / 1e-4 (point to plane)
relative, as tests/test_gpu_icp.py; the lattice bit for bit; batch == one by one bit for bit on both sides of kTileMinQueries and
in two parts, with an alignment that fails in its first solve among them."""
import numpy as np
import pytest

import icp_param_cases as pc
import oracle_icp_binding as oi
from scl_slam_amd import ScanContextEngine
from scl_slam_amd.synth import rigid_transform
from test_gpu_keyframe_store import _window, world  # noqa: F401  (the store's world builder, a fixture)

pytestmark = pytest.mark.gpu
IDENT = np.eye(4, dtype=np.float32)


@pytest.fixture(scope="module")
def eng():
    e = ScanContextEngine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def checker():
    """every checker result this file compares with, computed side by side, once"""
    pc.oracle_many([(c, cand, True, None) for c in pc.all_cases() for cand in c.checked])
    return pc.oracle


def _bits_equal(a, b):
    """two (T, fitness, converged, iterations) bit for bit"""
    return (np.array_equal(np.asarray(a[0], np.float32).view(np.uint32), np.asarray(b[0], np.float32).view(np.uint32))
            and np.float32(a[1]).view(np.uint32) == np.float32(b[1]).view(np.uint32) and bool(a[2]) == bool(b[2]) and int(a[3]) == int(b[3]))


def _assert_matches_checker(name, g, o, estimator):
    Tg, fg, cg, ig = g
    To, fo, co, io = o
    print(name, "gpu", (bool(cg), int(ig)), "checker", (co, io), "|dT|", np.abs(Tg - To).max(), "fitness", fg, fo, abs(fg - fo) / max(1e-6, abs(fo)))
    assert (bool(cg), int(ig)) == (co, io)
    assert np.abs(Tg - To).max() < pc.TOL
    assert abs(fg - fo) <= pc.FIT_REL[estimator] * max(1e-6, abs(fo)) + 1e-12


def _batch(eng, c, moved=True):
    Tb, fb, cb, ib = eng.icp_align_batch(c.src, c.tgts, pc.engine_params(eng, pc.fields(c, moved)))
    return [(Tb[k], fb[k], cb[k], ib[k]) for k in range(len(c.tgts))]


@pytest.mark.parametrize("c", pc.small_cases() + pc.edge_cases(), ids=lambda c: c.name)
def test_icp_align_off_defaults_matches_oracle(eng, checker, c):
    g = eng.icp_align(c.src, c.tgts[0], pc.engine_params(eng, pc.fields(c)))
    o = checker(c)
    _assert_matches_checker(c.name, g, o, c.base.get("estimator", 0))
    if c.about == "few":                                             # fewer than three pairs at the first search: nothing moved, and the
        assert (g[2], g[3]) == (False, 0)                            # fitness is still the mean over ALL sources (its pass has no threshold)
        assert np.array_equal(g[0].view(np.uint32), IDENT.view(np.uint32))
        _, d2 = oi.nn(c.src, c.tgts[0])
        want = d2.astype(np.float64).mean()
        assert abs(g[1] - want) <= 1e-6 * want
    if c.group == "edge" and c.moved["max_correspondence_dist"] == 0.5:
        assert np.array_equal(g[0].view(np.uint32), o[0].view(np.uint32))   # d2 == maxd2 is kept: exactly the checker's transform
    if c.group == "edge" and c.moved["max_correspondence_dist"] == 0.4999999:
        assert (g[2], g[3]) == (False, 0) and np.array_equal(g[0].view(np.uint32), IDENT.view(np.uint32))


@pytest.fixture(scope="module")
def tile_runs(eng):
    """name -> (batch results, one-by-one results) of every tile case, each run once"""
    runs = {}
    for c in pc.tile_cases():
        p = pc.engine_params(eng, pc.fields(c))
        runs[c.name] = (_batch(eng, c), [eng.icp_align(c.src, t, p) for t in c.tgts])
    return runs


@pytest.mark.parametrize("c", pc.tile_cases(), ids=lambda c: c.name)
def test_batch_under_a_threshold_equals_one_by_one(tile_runs, c):
    """scl_icp_align_batch's promise under a finite rejection distance: by tiles (>= 300 000 queries), in memory (below), in two parts"""
    batch, single = tile_runs[c.name]
    for k, (b, s) in enumerate(zip(batch, single)):
        print(c.name, c.tgt_keys[k], "batch", (bool(b[2]), int(b[3])), "one by one", (s[2], s[3]))
        assert _bits_equal(b, s), (c.name, c.tgt_keys[k])


@pytest.mark.parametrize("c", pc.tile_cases(), ids=lambda c: c.name)
def test_batch_under_a_threshold_matches_oracle(tile_runs, checker, c):
    batch, _ = tile_runs[c.name]
    for cand in c.checked:
        o = checker(c, cand)
        _assert_matches_checker(f"{c.name} {c.tgt_keys[cand]}", batch[cand], o, c.base.get("estimator", 0))
        assert o[3] > 1                                              # (these go on while the far candidate's alignment has ended)


@pytest.mark.parametrize("c", pc.tile_cases(), ids=lambda c: c.name)
def test_alignment_that_fails_at_once_leaves_its_part_running(tile_runs, c):
    """no source within the rejection distance of the far candidate: not converged, 0 iterations, identity, in the first solve of its
    part; the part's other alignments end where their one-by-one calls end (and not in the first iteration)"""
    batch, single = tile_runs[c.name]
    T, f, cv, it = batch[c.far]
    assert (bool(cv), int(it)) == (False, 0) and np.array_equal(T.view(np.uint32), IDENT.view(np.uint32))
    per_part = len(c.tgts) if c.group == "tile1" else len(c.tgts) // 2       # (icp_batch_run: one part, or two of equal size)
    part = range(per_part * (c.far // per_part), per_part * (c.far // per_part) + per_part)
    for k in part:
        if k == c.far:
            continue
        assert bool(batch[k][2]) and int(batch[k][3]) == single[k][3]
        if not c.tgt_keys[k].endswith("_self"):
            assert int(batch[k][3]) > 1, c.tgt_keys[k]


def test_both_sides_of_the_tile_threshold_agree(tile_runs):
    """5 x 60 000 queries (tiles) and 5 x 59 999 (memory) differ by one source, the last, which lies outside every box and is
    rejected, so it adds to no sum of an iteration: transform, convergence and iteration count agree bit for bit on the 59 999
    sources the two share.  (The fitness counts the last source and is not compared; the copy of the source as target holds that
    source itself.)  Each side is also held bit for bit to its one-by-one calls above."""
    a, b = pc.case("tile1-300000-p2p"), pc.case("tile1-299995-p2p")
    ra, rb = tile_runs[a.name][0], tile_runs[b.name][0]
    for k, key in enumerate(a.tgt_keys):
        if key.endswith("_self"):
            continue
        print(key, (bool(ra[k][2]), int(ra[k][3])), (bool(rb[k][2]), int(rb[k][3])), "|dT|", np.abs(ra[k][0] - rb[k][0]).max())
        assert (bool(ra[k][2]), int(ra[k][3])) == (bool(rb[k][2]), int(rb[k][3])), key
        assert np.array_equal(ra[k][0].view(np.uint32), rb[k][0].view(np.uint32)), key


@pytest.mark.parametrize("c", pc.edge_tile_cases(), ids=lambda c: c.name)
def test_exact_edge_in_the_tile_finish(eng, checker, c):
    """the lattice at 60 800 points, five copies of the target in one batch (304 000 queries: searched by tiles, the records formed
    by icp_tile_finish_kernel): d2 == maxd2 == 0.25f is kept there too -- every candidate the checker's transform bit for bit, and
    the one-by-one call's"""
    o = checker(c)
    p = pc.engine_params(eng, pc.fields(c))
    single = eng.icp_align(c.src, c.tgts[0], p)
    for k, b in enumerate(_batch(eng, c)):
        assert (bool(b[2]), int(b[3])) == (o[2], o[3]), k
        assert np.array_equal(b[0].view(np.uint32), o[0].view(np.uint32)), k
        assert _bits_equal(b, single), k
        assert abs(b[1] - o[1]) <= pc.FIT_REL[0] * o[1]


@pytest.mark.parametrize("estimator", [0, 1])
def test_nothing_of_a_threshold_sticks(eng, tile_runs, estimator):
    """one engine: threshold 0.5, defaults, threshold 0.5 again -- the first and the third bit for bit, the second a fresh engine's"""
    c = pc.case("tile2-far_in_part0-" + ("plane" if estimator else "p2p"))
    first = tile_runs[c.name][0]
    second = _batch(eng, c, moved=False)
    third = _batch(eng, c)
    fresh_eng = ScanContextEngine()
    try:
        fresh = _batch(fresh_eng, c, moved=False)
    finally:
        fresh_eng.close()
    for k in range(len(c.tgts)):
        assert _bits_equal(first[k], third[k]), c.tgt_keys[k]
        assert _bits_equal(second[k], fresh[k]), c.tgt_keys[k]
    assert not all(_bits_equal(first[k], second[k]) for k in range(len(c.tgts)))


def test_store_forms_off_defaults(world):  # noqa: F811
    """scl_loop_icp_batch_from_store == scl_loop_icp_from_store per candidate, and == scl_icp_align on the submaps scl_submap_from_store
    returns, with the rejection distance and the transformation epsilon moved"""
    e, clouds, poses = world
    drift = rigid_transform(0.01, -0.015, 0.04, 0.25, -0.2, 0.05)
    cur = pc.outlier_source(clouds[5], drift, 1, seed=41)            # keyframe 5's place again, from a slightly wrong pose, with outliers
    e.keyframe_put(0, 12, cur)
    sn, leaf = 1, 0.4
    keys = [5, 2, 9, 6]
    allposes = list(poses) + [poses[5]]
    wins = np.stack([np.stack(_window(allposes, k, sn)) for k in keys])
    moved = {"max_correspondence_dist": 0.5, "transformation_epsilon": 1e-3}
    for base in ({"max_iterations": 30}, {"max_iterations": 30, "estimator": 1, "normal_radius": 1.5}):
        p = pc.engine_params(e, dict(base, **moved))
        Tb, fb, cb, ib, ns, ntb = e.loop_icp_batch_from_store(0, 12, poses[5], keys, sn, wins, leaf, p)
        for k, key in enumerate(keys):
            T1, f1, c1, i1, ns1, nt1 = e.loop_icp_from_store(0, 12, poses[5], key, sn, _window(allposes, key, sn), leaf, p)
            assert (ns, ntb[k]) == (ns1, nt1) and ns >= 300 and nt1 >= 1000
            assert _bits_equal((Tb[k], fb[k], cb[k], ib[k]), (T1, f1, c1, i1)), (base, key)
        src = e.submap_from_store(0, 12, 0, [poses[5]], leaf, cur.shape[0])
        tgt = e.submap_from_store(0, 5, sn, _window(allposes, 5, sn), leaf, 40000)
        assert (ns, ntb[0]) == (src.shape[0], tgt.shape[0])
        assert _bits_equal((Tb[0], fb[0], cb[0], ib[0]), e.icp_align(src, tgt, p))
        # the moved fields decide this outcome (checker alone, on the same submaps): otherwise the equalities above would say nothing
        om = oi.icp_align(src, tgt, pc.oracle_params(dict(base, **moved)))
        od = oi.icp_align(src, tgt, pc.oracle_params(base))
        print(base, "gpu", (bool(cb[0]), int(ib[0])), "checker", om[2:], "defaults", od[2:], "|dT|", np.abs(Tb[0] - om[0]).max())
        assert (om[2], om[3]) != (od[2], od[3]) or np.abs(om[0] - od[0]).max() > 100 * pc.TOL
