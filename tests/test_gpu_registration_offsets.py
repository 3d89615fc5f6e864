"""The registration path kilometres from the origin: scl_transform_cloud, scl_voxel_grid, scl_assemble_submap, scl_nn_correspondences,
scl_nn_correspondences_moved, scl_target_normals, scl_icp_align[_batch], scl_ransac_correspondences, scl_geometric_verification and
scl_registration_eval_batch on the inputs of tests/offset_cases.py, 0, 500, 2 000 and 8 000 m out (tests/test_offset_cases.py shows with the CPU checker alone
that its grid walk equals its brute force there, that the inputs catch a wrong pruning margin, and measures the bars).

Bit for bit against the checker: the transform, the voxel filter, the submap, both neighbour searches (indices and distance bits,
against BRUTE FORCE), the exact lattice moved by an integer vector (the unshifted lattice's answers), and the batch by tiles against
its one-by-one calls in memory at 8 km.
Within the measured bars: ICP on icp_small -- (converged, iterations) equal, moved source points within offset_cases.icp_offset_bound,
fitness within offset_cases.fitness_bar, and at offset 0 the TOL / FIT_REL of tests/test_gpu_icp_params.py as well; the normals within
tests/test_gpu_registration_plane.py's bar (translation-invariant: the reference covariance is formed from differences that are exact
in float64); RANSAC's mask, count and best hypothesis equal; the verification's counts equal and its T, a rigid fit, within
test_verification_cases.offset_bound's bar on its inlier pairs (not bit for bit: see test_geometric_verification_far_out); the
scoring's n_valid and n_inliers equal, with overlap and the RMSE's sum under tests/test_gpu_registration_eval.py's bar.
The scoring's nine moments and the information matrix are left out here: sums of coordinates and their products 8 km out need a bar
of their own."""
from fractions import Fraction

import numpy as np
import pytest

import icp_param_cases as pc
import offset_cases as oc
import oracle_icp_binding as oi
from scl_slam_amd import ScanContextEngine

pytestmark = pytest.mark.gpu
IDENT = np.eye(4, dtype=np.float32)
SLACK = Fraction(2) ** -53 * (1 + Fraction(2) ** -20)                 # tests/test_gpu_registration_eval.py
OFFS = pytest.mark.parametrize("off", oc.OFFSETS, ids=lambda v: f"{v:g}m")
FAMS = pytest.mark.parametrize("name", oc.FAMILIES)


@pytest.fixture(scope="module")
def eng():
    e = ScanContextEngine()
    yield e
    e.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _bits_equal(a, b):
    """two (T, fitness, converged, iterations) bit for bit"""
    return (np.array_equal(_bits(a[0]), _bits(b[0])) and np.float32(a[1]).view(np.uint32) == np.float32(b[1]).view(np.uint32)
            and bool(a[2]) == bool(b[2]) and int(a[3]) == int(b[3]))


def _batch(eng, src, tgts, p):
    Tb, fb, cb, ib = eng.icp_align_batch(src, tgts, p)
    return [(Tb[k], fb[k], cb[k], ib[k]) for k in range(len(tgts))]


def _assert_nn(where, got, src, tgt):
    gi, gd = got
    bi, bd = oi.nn(src, tgt, use_grid=False)
    wrong = (gi != bi) | (_bits(gd) != _bits(bd))
    print(where, int(wrong.sum()), "of", len(src), "queries differ from brute force", np.flatnonzero(wrong)[:8].tolist())
    assert np.array_equal(gi, bi) and np.array_equal(_bits(gd), _bits(bd))


# ---- bit for bit: transform, voxel filter, submap ---------------------------------------------------------------------------------
@OFFS
def test_transform_cloud(eng, off):
    c, T = oc.transform_input(off)
    assert np.array_equal(_bits(eng.transform_cloud(c, T)), _bits(oi.transform(c, T)))


@OFFS
@pytest.mark.parametrize("name,leaf", [("scene", 0.4), ("dense", 0.01)])
def test_voxel_grid(eng, name, leaf, off):
    c = oc.family(name, off)[1]
    g, o = eng.voxel_grid(c, leaf), oi.voxel_grid(c, leaf)
    print(name, off, len(c), "->", len(o), "voxels")
    assert o is not None and 1 < len(o) < len(c)
    assert g.shape == o.shape and np.array_equal(_bits(g), _bits(o))


@OFFS
def test_assemble_submap(eng, off):
    clouds, Ts = oc.submap_input(off)
    g = eng.assemble_submap(clouds, Ts, 0.4)
    o = oi.voxel_grid(np.concatenate([oi.transform(c, T) for c, T in zip(clouds, Ts)]), 0.4)
    assert g.shape == o.shape and np.array_equal(_bits(g), _bits(o))


# ---- bit for bit: the searches ------------------------------------------------------------------------------------------------------
@OFFS
@FAMS
def test_nn_correspondences(eng, name, off):
    src, tgt = oc.family(name, off)
    _assert_nn(f"{name} at {off:g} m:", eng.nn_correspondences(src, tgt), src, tgt)


@OFFS
@FAMS
@pytest.mark.parametrize("move", oc.MOVES)
def test_nn_correspondences_moved(eng, name, off, move):
    """the warm walk: searched from the unmoved source's neighbours == a cold brute-force search of the moved cloud"""
    src, tgt = oc.family(name, off)
    T = oc.hair(move)
    _assert_nn(f"{name} at {off:g} m moved by {move:g}:", eng.nn_correspondences_moved(src, tgt, T), oi.transform(src, T), tgt)


# ---- bit for bit: the exact lattice moved by (8192, -4096, 2048) -----------------------------------------------------------------------
@pytest.mark.parametrize("name", oc.EXACT_EDGE)
def test_exact_lattice_shifted(eng, name):
    """the assertions of test_gpu_icp_params.test_icp_align_off_defaults_matches_oracle, the expected values those of the UNSHIFTED
    lattice (tests/test_offset_cases.py: the checker's answer carries over bit for bit)"""
    c = oc.exact_lattice(name)
    g = eng.icp_align(c.src, c.tgts[0], pc.engine_params(eng, pc.fields(c)))
    o = pc.oracle(pc.case(name))
    print(c.name, "gpu", (bool(g[2]), int(g[3])), "checker", (o[2], o[3]), "|dT|", np.abs(g[0] - o[0]).max(), "fitness", g[1], o[1])
    assert (bool(g[2]), int(g[3])) == (o[2], o[3])
    assert np.abs(g[0] - o[0]).max() < pc.TOL
    assert abs(g[1] - o[1]) <= pc.FIT_REL[0] * max(1e-6, abs(o[1])) + 1e-12
    if c.moved["max_correspondence_dist"] == 0.5:
        assert np.array_equal(_bits(g[0]), _bits(o[0]))              # d2 == maxd2 is kept: exactly the checker's transform
    else:
        assert (g[2], g[3]) == (False, 0) and np.array_equal(_bits(g[0]), _bits(IDENT))


@pytest.mark.parametrize("name", oc.EXACT_TILE)
def test_exact_lattice_shifted_in_the_tile_finish(eng, name):
    """the assertions of test_gpu_icp_params.test_exact_edge_in_the_tile_finish on the 60 800-point lattice in five copies"""
    c = oc.exact_lattice(name)
    o = pc.oracle(pc.case(name))
    p = pc.engine_params(eng, pc.fields(c))
    single = eng.icp_align(c.src, c.tgts[0], p)
    for k, b in enumerate(_batch(eng, c.src, c.tgts, p)):
        assert (bool(b[2]), int(b[3])) == (o[2], o[3]), k
        assert np.array_equal(_bits(b[0]), _bits(o[0])), k
        assert _bits_equal(b, single), k
        assert abs(b[1] - o[1]) <= pc.FIT_REL[0] * o[1]
    if c.moved["max_correspondence_dist"] == 0.4999999:
        assert (o[2], o[3]) == (False, 0) and np.array_equal(_bits(single[0]), _bits(IDENT))


# ---- tiles against memory, 8 km out --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [60000, 59999])
def test_batch_by_tiles_equals_one_by_one_far_out(eng, n):
    """5 x 60 000 queries = kTileMinQueries: searched by tiles, the smallest batch they ever run on; the five one-by-one calls search
    in memory.  5 x 59 999: the batch in memory too.  Bit for bit in T, fitness, converged and iterations; the far candidate answers
    (False, 0) and the identity.  (The checker is not run at this size.)"""
    src, tgts = oc.icp_tile(8000.0)
    src = src if n == len(src) else src[:n].copy()
    p = pc.engine_params(eng, oc.TILE_FIELDS)
    batch = _batch(eng, src, tgts, p)
    single = [eng.icp_align(src, t, p) for t in tgts]
    print(n, "iterations", [int(b[3]) for b in batch], "one by one", [int(s[3]) for s in single], "converged", [bool(b[2]) for b in batch])
    for k, (b, s) in enumerate(zip(batch, single)):
        assert _bits_equal(b, s), pc.TILE1_ORDER[k]
    far = batch[pc.TILE1_ORDER.index("far")]
    assert (bool(far[2]), int(far[3])) == (False, 0) and np.array_equal(_bits(far[0]), _bits(IDENT))
    assert int(batch[pc.TILE1_ORDER.index("match")][3]) > 1


# ---- within the measured bars -----------------------------------------------------------------------------------------------------------
@OFFS
@pytest.mark.parametrize("estimator", [0, 1])
def test_icp_align_far_out(eng, estimator, off):
    src, tgt = oc.icp_small(off)
    Tg, fg, cg, ig = eng.icp_align(src, tgt, pc.engine_params(eng, oc.ICP_FIELDS[estimator]))
    To, fo, co, io = oc.icp_checker(off, estimator)
    p = src[:, :3].astype(np.float64)
    err, bound, fbar = float(np.abs(oc.moved(Tg, p) - oc.moved(To, p)).max()), oc.icp_offset_bound(off, estimator), oc.fitness_bar(off, estimator)
    print(f"estimator {estimator} at {off:g} m: gpu {(bool(cg), int(ig))} checker {(co, io)}, moved points differ by {err:.3e} m (bound {bound:.3e}), "
          f"|dT| {np.abs(Tg - To).max():.3e}, fitness {fg} {fo} relative {abs(fg - fo) / fo:.3e} (bar {fbar:.3e})")
    assert (bool(cg), int(ig)) == (co, io)
    assert err <= bound
    assert abs(fg - fo) <= fbar * abs(fo)
    if off == 0.0:                                                    # the bars near the origin are the ones there have always been
        assert np.abs(Tg - To).max() < pc.TOL
        assert abs(fg - fo) <= pc.FIT_REL[estimator] * max(1e-6, abs(fo)) + 1e-12


@OFFS
@pytest.mark.parametrize("name,radius", [("scene", 1.5), ("border_lattice", 2 * oc.PITCH)])
def test_target_normals_far_out(eng, name, radius, off):
    """on the lattice the radius is two pitches: there are points at exactly r, up to the rounding of the coordinates"""
    tgt = oc.family(name, off)[1]
    nrm = eng.target_normals(tgt, radius)
    few, unit, res = oc.normal_residuals(tgt, radius, nrm)
    print(f"{name} at {off:g} m, radius {radius}: {int(few.sum())} of {len(tgt)} without a normal, worst | |n| - 1 | "
          f"{unit[~few].max() * 2 ** 23:.3f} x 2^-23, worst residual {res[~few].max() * 2 ** 23:.3f} x 2^-23 l_max")
    assert np.array_equal(~(nrm != 0).any(1), few)
    assert not few.all()
    assert (unit[~few] <= 2.0 ** -23).all() and (res[~few] <= 2.0 ** -23).all()


@OFFS
@pytest.mark.parametrize("name", oc.RANSACS)
def test_ransac_far_out(eng, name, off):
    """mask, inlier count and best hypothesis equal to the checker's, as test_gpu_verification_edges._assert_ransac; the inlier sets
    are strict subsets that depend on the hypothesis (35 % and 90 % outliers, a tie between two clean hypotheses, a last hypothesis
    that alone is clean).  The winning hypothesis's T: the checker's is float64 and the device returns float32, whose rounding is 2^-24
    of an entry -- 5e-4 m on a translation of 8 km, where _assert_ransac's 1e-6 cannot hold -- so each entry is held to 1e-6 (that
    bar) plus 2^-23 of the entry (the rounding, twice)"""
    src, tgt, si, ti, iters, thr, seed, good = oc.ransac_input(name, off)
    gm, gn, gb, gT = eng.ransac_correspondences(src, tgt, si, ti, iters, thr, seed)
    om, on, ob_, oT = oc.ransac_checked(name, off)
    dT = np.abs(gT[:3].astype(np.float64) - oT)
    print(f"{name} at {off:g} m: gpu {(gn, gb)} checker {(on, ob_)}, mask differs in {int((gm != om).sum())} pairs, worst |dT| / bar "
          f"{(dT / (1e-6 + 2.0 ** -23 * np.abs(oT))).max():.3f}")
    assert (gn, gb) == (on, ob_)
    assert np.array_equal(gm, om) and np.array_equal(gm.astype(bool), good)
    assert (dT <= 1e-6 + 2.0 ** -23 * np.abs(oT)).all()
    if off == 0.0:
        assert dT.max() < 1e-6


@OFFS
@pytest.mark.parametrize("name", oc.VERIFICATIONS)
def test_geometric_verification_far_out(eng, name, off):
    """success, pair count and inlier count equal to the checker's (`ratio_exact`: half of the pairs are inliers, a set only a clean
    hypothesis finds, and the ratio gate sits on its boundary); the pairs and RANSAC on them, through scl_nn_correspondences and scl_ransac_correspondences, bit for bit (indices,
    mask, count, best hypothesis).  The final T is NOT held bit for bit, which the rigid fit cannot be: the device forms it in one
    pass with the polar factor, the checker in two with Horn's quaternion.  It is held to the rigid fit's bar far from the origin
    (offset_cases.verification_checked; test_rigid_svd_far_from_the_origin), and to TOL as ever at offset 0"""
    src, tgt, iters, thr, ratio, seed = oc.verification(name, off)
    g = eng.geometric_verification(src, tgt, iters, thr, ratio, seed)
    o, p, spread, bound, (si, ti, mask, n_inl, best, Tb) = oc.verification_checked(name, off)
    err = float(np.abs(oc.moved(g[0], p) - oc.moved(o[0], p)).max())
    print(f"verification of {name} at {off:g} m: gpu {g[1:]} checker {o[1:]}, moved points differ by {err:.3e} m (bound {bound:.3e}), "
          f"|dR| {np.abs(g[0][:3, :3] - o[0][:3, :3]).max():.3e}")
    assert g[1:] == o[1:]
    gi, _ = eng.nn_correspondences(src, tgt)
    assert np.array_equal(np.flatnonzero(gi >= 0), si) and np.array_equal(gi[si], ti)
    gm, gn, gb, _ = eng.ransac_correspondences(src, tgt, si, ti, iters, thr, seed)
    assert (gn, gb) == (n_inl, best) and np.array_equal(gm, mask)
    assert err <= bound
    assert np.abs(g[0][:3, :3] - o[0][:3, :3]).max() < pc.TOL
    if off == 0.0:
        assert np.abs(g[0] - o[0]).max() < pc.TOL


@OFFS
def test_registration_eval_batch_far_out(eng, off):
    src, tgts, Ts, max_dist = oc.eval_list(off)
    got = eng.registration_eval_batch(src, tgts, Ts, max_dist)
    want = oc.eval_checked(off)
    worst = Fraction(0)
    for c, (nv, m, S, A) in enumerate(want):
        assert (int(got.n_valid[c]), int(got.n_inliers[c])) == (nv, m), (c, got.n_valid[c], got.n_inliers[c], nv, m)
        err = abs(Fraction(float(got.moments[c, 9])) - Fraction(float(S[9])))
        bound = m * SLACK * Fraction(float(A[9]))
        assert err <= bound, (c, float(err), float(bound))
        if bound:
            worst = max(worst, err / bound)
        assert got.overlap[c] == m / len(src)
        if m:
            # every d2 is positive, so the sum's bound is relative, m 2^-53; the root halves it, the division and the root round once each
            assert abs(got.rmse[c] - np.sqrt(S[9] / m)) <= (m + 4) * 2.0 ** -53 * got.rmse[c]
    print(f"scoring at {off:g} m: valid {got.n_valid.tolist()} inliers {got.n_inliers.tolist()}, sum d2 worst error / bound {float(worst):.3f}")
