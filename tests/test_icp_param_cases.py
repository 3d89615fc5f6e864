"""The inputs of tests/icp_param_cases.py, proven with the CPU checker alone (no GPU): every case is sensitive to the field it moves
and is not on a knife edge, so that tests/test_gpu_icp_params.py may rest on it.

Sensitive: the checker's (converged, iterations, T) under the case's fields differs from its answer under defaults -- another iteration
count, or |dT|max > 100 * TOL.  The "both epsilons 0" cases instead need defaults to stop before the cap.  For threshold cases the
share of the sources within the threshold at the first search lies in [0.02, 0.9] (0 for the "fewer than three pairs" cases; the
lattice has its own exact answers).

Not on a knife edge: copies of the source with half of the coordinates moved to the neighbouring float give the same (converged,
iterations), T within TOL / 2 and a fitness within half of the relative bound the GPU test uses.  Three copies for every checked
candidate but one: the unrelated place of the two-part point-to-point cases has a single copy (below).  The lattice IS the edge in x (d2 == maxd2 exactly, by inputs that
are exact in float32 and an increment-free first iteration), so its copies move y and z only, which leaves every d2 bit unchanged
(0.25 + ulp^2 rounds to 0.25) and must leave the answer where it is.

Largest deviations measured over these copies (x86-64, this file's seeds):
  small, point to point   |dT| 1.15e-6 (max_correspondence_dist 0.2), fitness 9.8e-8 relative
  small, point to plane   |dT| 2.21e-6 (max_correspondence_dist 0.2), fitness 9.8e-8 relative
  lattice                 |dT| 2.0e-7, fitness 6.1e-7 relative
  tiles, point to point   |dT| 2.19e-6 (75 000 sources, an unrelated place), fitness 1.6e-7 relative
  tiles, point to plane   |dT| 7.5e-8, fitness 8.1e-8 relative
The point-to-point alignments of unrelated places under a hard threshold are the touchy ones: a neighbour that flips between two target
points moves T by about (their distance) / (pairs), 1e-5 at these sizes, and of the candidates and outlier seeds tried about half
stayed within TOL / 2 under one jittered copy.  The seeds and the checked candidates in icp_param_cases.py are ones that did.  Under
THREE copies none of the 15 unrelated candidates tried at 75 000 sources (outlier seeds 25, 27, 28) stayed within TOL / 2: the best
reached 5.2e-6, 6.2e-6 and 6.9e-6, the committed one (seed 25, other4) 1.13e-5 on its third copy, always with the same (converged,
iterations); the matching place stays below 1.4e-6 under all three, the 60 000-source candidates below 2.6e-6, point to plane below
2.1e-7.  So that one candidate is held to one copy, the least a tile case may have: for it this file shows the iteration count robust
and T robust only to the copy it runs.  What the GPU test
rests on is narrower than a jittered input: the engine's neighbours and distances are bit-identical to the checker's, and its sums
differ from the checker's in float64 rounding only."""
import numpy as np
import pytest

import icp_param_cases as pc

SMALL_EDGE = pc.small_cases() + pc.edge_cases() + pc.edge_tile_cases()
TILES = pc.tile_cases()


@pytest.fixture(scope="module")
def results():
    """every checker run this file needs, side by side, once"""
    reqs = []
    for c in SMALL_EDGE + TILES:
        for cand in c.checked:
            reqs += [(c, cand, True, None), (c, cand, False, None)]
            reqs += [(c, cand, True, j) for j in pc.jitter_copies(c, cand)]
    pc.oracle_many(reqs)
    return pc.oracle


def _same_answer(a, b):
    return (a[2], a[3]) == (b[2], b[3]) and np.abs(a[0] - b[0]).max() <= 100 * pc.TOL


@pytest.mark.parametrize("c", SMALL_EDGE + TILES, ids=lambda c: c.name)
def test_case_is_sensitive_to_the_field_it_moves(results, c):
    for cand in c.checked:
        moved, dflt = results(c, cand, True), results(c, cand, False)
        print(c.name, cand, "moved", moved[2:], "defaults", dflt[2:], "|dT|", np.abs(moved[0] - dflt[0]).max())
        if c.about == "cap":
            cap = c.base["max_iterations"]
            assert dflt[2] and dflt[3] < cap and moved[2] and moved[3] == cap
        elif c.group.startswith("edge"):
            others = [results(o, 0, True) for o in pc.edge_cases() + pc.edge_tile_cases() if o.src is c.src and o.name != c.name]
            assert not any(_same_answer(moved, o) for o in others)
        else:
            assert not _same_answer(moved, dflt)
        if c.about == "few":
            assert pc.first_search_share(c, cand) == 0.0 and (moved[2], moved[3]) == (False, 0)
        elif c.about == "max_correspondence_dist" and not c.group.startswith("edge"):
            assert 0.02 <= pc.first_search_share(c, cand) <= 0.9


@pytest.mark.parametrize("c", SMALL_EDGE + TILES, ids=lambda c: c.name)
def test_case_is_not_on_a_knife_edge(results, c):
    fit_rel = 0.5 * pc.FIT_REL[c.base.get("estimator", 0)]
    for cand in c.checked:
        T, f, cv, it = results(c, cand, True)
        for j in pc.jitter_copies(c, cand):
            Tj, fj, cvj, itj = results(c, cand, True, j)
            print(c.name, cand, j, "|dT|", np.abs(Tj - T).max(), "fitness", abs(fj - f) / max(1e-6, abs(f)))
            assert (cvj, itj) == (cv, it)
            assert np.abs(Tj - T).max() <= 0.5 * pc.TOL
            assert abs(fj - f) <= fit_rel * max(1e-6, abs(f)) + 1e-12


def test_out_of_box_sources_are_beyond_every_threshold():
    """the last N_OUT_OF_BOX sources of every cloud with outliers lie further than the default 100 m from every one of its targets
    (but the copy of the source itself and the cloud moved FAR_SHIFT away, which no test compares under defaults with the checker)"""
    import oracle_icp_binding as oi
    for c in (pc.case("small-p2p-mcd0.5"), pc.case("tile1-300000-p2p"), pc.case("tile2-far_in_part0-p2p")):
        for t, key in zip(c.tgts, c.tgt_keys):
            if key.endswith("_self") or key.endswith("_far"):
                continue
            _, d2 = oi.nn(c.src[-pc.N_OUT_OF_BOX:], t)
            assert d2.min() > 100.0 ** 2


def test_far_candidate_has_no_source_within_the_threshold():
    import oracle_icp_binding as oi
    for c in (pc.case("tile1-300000-p2p"), pc.case("tile2-far_in_part0-p2p")):
        _, d2 = oi.nn(c.src[::25], c.tgts[c.far])                    # a sample for the walk's sake; the bound below covers every source
        assert d2.min() > 0.25
        lo_t = c.tgts[c.far][:, :3].min(0)
        inside = c.src[:-pc.N_OUT_OF_BOX, :3]
        # every in-box source lies below the far cloud's box in z by more than the threshold (sources reach z < 6 + outliers)
        assert (lo_t[2] - inside[:, 2]).min() > 0.5


def test_lattice_answers_are_exact(results):
    src, tgt = pc.edge_clouds()
    d2 = ((src[:, :3] - tgt[:, :3]) ** 2).sum(1, dtype=np.float32)
    assert set(d2.tolist()) == {0.25, 0.5625}                        # exact in float32: d2 == maxd2 is decided by the comparison alone
    at = {c.moved["max_correspondence_dist"]: results(c, 0, True) for c in pc.edge_cases()}
    T, f, cv, it = at[0.5]                                            # d2 == maxd2 == 0.25f is kept: the even sources alone
    want = np.eye(4, dtype=np.float32); want[0, 3] = -0.5
    assert (cv, it) == (True, 1) and np.array_equal(T.view(np.uint32), want.view(np.uint32))
    T, f, cv, it = at[0.4999999]                                      # nothing within: not converged, untouched
    assert (cv, it) == (False, 0) and np.array_equal(T, np.eye(4, dtype=np.float32))
    T, f, cv, it = at[0.75]                                           # everything within, as under the default
    assert (cv, it) == (True, 1) and abs(T[0, 3] + 0.61099) < 1e-5
    Td = results(pc.case("edge-mcd0.75"), 0, False)[0]
    assert np.array_equal(T.view(np.uint32), Td.view(np.uint32))


@pytest.mark.parametrize("shape", list(pc.EDGE_TILE_SHAPES))
def test_large_lattice_answers_are_exact(results, shape):
    """the lattice of 60 800 points (searched by tiles as a batch of five): the same exact answers"""
    src, tgt = pc.edge_tile_clouds(shape)
    d2 = ((src[:, :3] - tgt[:, :3]) ** 2).sum(1, dtype=np.float32)
    assert set(d2.tolist()) == {0.25, 0.5625}
    assert pc.EDGE_TILE_COPIES * src.shape[0] >= 300000
    at = {c.moved["max_correspondence_dist"]: results(c, 0, True) for c in pc.edge_tile_cases() if c.src is src}
    want = np.eye(4, dtype=np.float32); want[0, 3] = -0.5
    T, f, cv, it = at[0.5]
    assert (cv, it) == (True, 1) and np.array_equal(T.view(np.uint32), want.view(np.uint32))
    T, f, cv, it = at[0.4999999]
    assert (cv, it) == (False, 0) and np.array_equal(T, np.eye(4, dtype=np.float32))


def test_tile_case_sizes_sit_where_the_dispatch_rule_changes():
    """kTileMinQueries = 300 000 (csrc/icp.hip): 5 x 60 000 is the first batch searched by tiles, 5 x 59 999 the last one that is
    not; 8 x 75 000 runs as two parts of 4 alignments and 300 000 queries each, the far candidate in part 0 or in part 1"""
    t1 = [c for c in TILES if c.group == "tile1"]
    assert [len(c.tgts) * c.src.shape[0] for c in t1] == [300000, 299995]
    assert np.array_equal(t1[0].src[:59999].view(np.uint32), t1[1].src.view(np.uint32))
    for c in TILES:
        if c.group == "tile2":
            assert len(c.tgts) == 8 and (len(c.tgts) // 2) * c.src.shape[0] >= 300000
    assert {c.far // (len(c.tgts) // 2) for c in TILES if c.group == "tile2"} == {0, 1}
