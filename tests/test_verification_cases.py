"""The CPU checker's rigid fit, RANSAC and geometric verification (oracle/icp_oracle.c) pinned on the inputs of
tests/verification_cases.py -- against a float64 Kabsch SVD, against the residual bounds the RANSAC cases promise and against the
pair counts the verification cases are built for.  Without this, tests/test_gpu_verification_edges.py's "GPU == checker" would prove
little.  No GPU needed.

The reference spread of the offset cases -- max |T_checker p - T_kabsch p| over the paired sources, in float64 -- and the bound the
GPU is held to there (the larger of 4 x the spread and 2 fp32 ulps of the largest coordinate; reference_spread, offset_bound):
    centroid    0 m from the origin: spread 3.0e-7 m, bound 1.9e-6 m  (2 ulps)
              500 m                : spread 9.5e-6 m, bound 6.1e-5 m  (2 ulps)
            2 000 m                : spread 4.3e-5 m, bound 2.4e-4 m  (2 ulps)
            8 000 m                : spread 1.2e-4 m, bound 9.8e-4 m  (2 ulps)
The spread is the checker's float T (a rotation rounded to 2^-24 carried over the offset); 4 x it stays below the 2 ulps throughout.
"""
import numpy as np
import pytest

import oracle_icp_binding as oi
import verification_cases as vc


def _moved(T, p):
    return p @ np.asarray(T, np.float64)[:3, :3].T + np.asarray(T, np.float64)[:3, 3]


def reference_spread(name):
    """max |T_oracle p - T_kabsch p| over the paired sources, in float64: how far the two references are apart on one case"""
    src, tgt, si, ti, _ = vc.rigid_cases()[name]
    p = src[si, :3].astype(np.float64)
    return float(np.abs(_moved(oi.rigid_svd(src, tgt, si, ti), p) - _moved(vc.kabsch(src, tgt, si, ti), p)).max())


def offset_bound(name):
    """what the GPU may differ from the checker by on an offset case, on moved points: 4 x the spread of the two references, or 2
    fp32 ulps of the largest coordinate (both sides round T to float), whichever is larger"""
    src, tgt, si, ti, _ = vc.rigid_cases()[name]
    big = np.float32(max(np.abs(src[si, :3]).max(), np.abs(tgt[ti, :3]).max()))
    return max(4.0 * reference_spread(name), 2.0 * float(np.spacing(big)))


@pytest.mark.parametrize("name", [n for n in vc.rigid_names() if not n.startswith("collinear")])
def test_checker_rigid_fit_equals_kabsch(name):
    """rotation to 1e-6 (the checker's T is float), translation to 1e-6 plus the rotation's rounding carried over the centroid's
    distance from the origin plus one rounding of t itself"""
    src, tgt, si, ti, T_true = vc.rigid_cases()[name]
    To, Tk = oi.rigid_svd(src, tgt, si, ti).astype(np.float64), vc.kabsch(src, tgt, si, ti)
    R = To[:3, :3]
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(R) - 1) < 1e-6
    assert np.abs(R - Tk[:3, :3]).max() < 1e-6
    reach = np.abs(src[si, :3]).max()
    assert np.abs(To[:3, 3] - Tk[:3, 3]).max() < 1e-6 + 3 * 2.0 ** -24 * reach + 2.0 ** -24 * np.abs(Tk[:3, 3]).max()
    if T_true is not None and not name.startswith(("pairs_3", "pairs_4")):    # (three or four noisy pairs fit their noise)
        assert np.abs(R - T_true[:3, :3]).max() < 5e-3
    if name == "mirrored":
        assert np.abs(Tk[:3, :3] - np.eye(3)).max() < 0.05 and np.abs(R - np.eye(3)).max() < 0.05
    if name == "identical":
        assert np.array_equal(R, np.eye(3)) and np.array_equal(To[:3, 3], np.float64(tgt[5, :3]) - np.float64(src[2, :3]))


def test_pair_lists_hold_repeats_and_a_permutation():
    cs = vc.rigid_cases()
    assert [len(cs[f"pairs_{n}"][2]) for n in vc.PAIR_COUNTS] == list(vc.PAIR_COUNTS)
    for n in vc.PAIR_COUNTS:
        src, tgt, si, ti, _ = cs[f"pairs_{n}"]
        assert len(src) == (8000 if n >= 32768 else 600) and not np.array_equal(si, ti)
        assert (len(np.unique(si)) < n) == (n > 4) and np.isfinite(src).all() and np.isfinite(tgt).all()
    assert {cs[f"pairs_{n}"][0].shape[1] for n in vc.PAIR_COUNTS} == {3, 4, 8}


def test_slabs_straddle_the_switch():
    """which side of det > 1e-5 every slab falls on (computed as the device forms it): at least two on either side, the thick ones on
    the polar side, the thin ones on Horn's; the planar cloud, the mirrored target and identical points are all on Horn's"""
    cs = vc.rigid_cases()
    det = {eps: vc.switch_det(*cs[f"slab_{eps:g}"][:4]) for eps in vc.SLAB_EPS}
    print({k: f"{v:.3e}" for k, v in det.items()})
    polar = [eps for eps in vc.SLAB_EPS if det[eps] > vc.POLAR_DET]
    horn = [eps for eps in vc.SLAB_EPS if not det[eps] > vc.POLAR_DET]
    assert len(polar) >= 2 and len(horn) >= 2
    assert set(polar) >= {1e-1, 1e-2, 6e-3} and set(horn) >= {4.5e-3, 2e-3, 1e-4}
    assert abs(det[5.3e-3] / vc.POLAR_DET - 1) < 0.15                 # ... and one within 15 % of it
    for name in ("planar", "mirrored", "identical", "pairs_3"):
        assert not vc.switch_det(*cs[name][:4]) > vc.POLAR_DET
    assert vc.switch_det(*cs["pairs_1024"][:4]) > 1e-2


def test_offset_cases_and_their_reference_spread():
    cs = vc.rigid_cases()
    for off in vc.OFFSETS:
        name = f"offset_{off:g}"
        src, tgt, si, ti, T = cs[name]
        c = src[:, :3].astype(np.float64).mean(0)
        assert abs(np.linalg.norm(c) - off) < 0.5
        spread, bound = reference_spread(name), offset_bound(name)
        print(f"{name}: spread {spread:.3e} m, bound {bound:.3e} m")
        assert spread < 1e-6 + 4 * 2.0 ** -24 * max(off, 20.0)        # the checker's float T, carried over the offset
        assert bound >= 2.0 * float(np.spacing(np.float32(max(off * 0.48, 1.0))))


def test_collinear_cases_are_collinear():
    for name in vc.rigid_names("collinear"):
        src, tgt, si, ti, _ = vc.rigid_cases()[name]
        p = src[si, :3].astype(np.float64); p -= p.mean(0)
        s = np.linalg.svd(p, compute_uv=False)
        assert s[1] < 1e-5 * s[0]


@pytest.mark.parametrize("name", vc.ransac_names())
def test_ransac_case_bounds_and_checker_count(name):
    case, iters, thr, seed = vc.ransac_get(name)
    src, tgt, si, ti, good = case["src"], case["tgt"], case["si"], case["ti"], case["good"]
    res = np.linalg.norm(_moved(vc.T_RANSAC, src[si, :3].astype(np.float64)) - tgt[ti, :3].astype(np.float64), axis=1)
    assert case["n_good"] >= 3 and res[good].max() <= 1e-3 * vc.THRESHOLD
    assert good.all() or res[~good].min() >= 10 * vc.THRESHOLD
    assert res.max() < 100.0                                          # threshold 1e3 admits every pair, under any of the models
    mask, n_inl, best_h, T = oi.ransac(src, tgt, si, ti, iters, thr, seed)
    assert n_inl == vc.ransac_expected_count(case, thr) == int(mask.sum()) and 0 <= best_h < iters
    if thr == vc.THRESHOLD:
        assert np.array_equal(mask.astype(bool), good) and np.abs(T - vc.T_RANSAC[:3]).max() < 1e-3
    if thr != vc.THRESHOLD or len(si) == 3 or good.all():
        assert best_h == 0                                            # every hypothesis ties: the lowest wins


def test_ransac_table_covers_the_issue():
    t = vc.RANSAC_TABLE
    assert {r[1] for r in t} >= set(vc.RANSAC_SIZES) | {16} and {r[3] for r in t} == set(vc.RANSAC_ITERATIONS) | {65536}
    assert {(r[1], r[3]) for r in t} >= {(n, it) for n in vc.RANSAC_SIZES for it in vc.RANSAC_ITERATIONS}
    for col, want in ((2, vc.RANSAC_FRACTIONS), (4, vc.RANSAC_THRESHOLDS), (5, vc.RANSAC_SEEDS), (6, vc.WIDTHS)):
        assert {r[col] for r in t} == set(want)
    assert [r for r in t if r[3] == 65536] == [r for r in t if r[1] == 16] and len({r[0] for r in t}) == len(t)
    # the ties away from hypothesis 0 are ties: two clean hypotheses, the lower one wins and is not the first
    for name in (n for n in vc.ransac_names() if n.startswith("tie_")):
        case, iters, thr, seed = vc.ransac_get(name)
        row = next(r for r in t if r[0] == name)
        mask, n_inl, best_h, T = oi.ransac(case["src"], case["tgt"], case["si"], case["ti"], iters, thr, seed)
        assert 0 < best_h <= row[7][0] < row[7][1] and n_inl == case["n_good"]    # (row[7][1] is clean as well: it ties and loses)
    # the sampler restated here is the checker's: on three pairs every hypothesis draws the same set
    assert sorted(vc.sample(vc.M64, 5, 3)) == [0, 1, 2] and len(set(vc.sample(0, 0, 4))) == 3


def test_last_hypothesis_wins_where_it_is_the_only_clean_one():
    """the cases that put the best hypothesis into the last slot (next to a workgroup's surplus slots, or in the picking kernel's
    second trip over the counts) exist: 90 % outliers, best = iterations - 1"""
    last = []
    for name in vc.ransac_names():
        case, iters, thr, seed = vc.ransac_get(name)
        if name.startswith("last_"):
            best_h = oi.ransac(case["src"], case["tgt"], case["si"], case["ti"], iters, thr, seed)[2]
            if best_h == iters - 1:
                last.append(iters)
    print(sorted(last))
    assert sorted(last) == [7, 8, 9, 255, 256, 257]


@pytest.mark.parametrize("name", vc.verification_names())
def test_checker_verification(name):
    src, tgt, iters, thr, ratio, seed = vc.verification_cases()[name]
    T, ok, nc, ni = oi.geometric_verification(vc.checker_source(name), tgt, iters, thr, ratio, seed)
    print(name, ok, nc, ni)
    finite = int(np.isfinite(src[:, :3]).all(1).sum())
    assert nc == (finite if len(tgt) else 0)                          # every finite source finds a neighbour, no other does
    if name in vc.NONFINITE_COUNTS:
        assert nc == len(src) - vc.NONFINITE_COUNTS[name] and len(src) == 2000
    if nc < 3 or name == "few_inliers":
        assert ni < 3 and np.array_equal(T, np.eye(4, dtype=np.float32))
        assert ok == (name == "few_inliers" and ratio == 0.0)
    if name in ("matching", "nonfinite_3"):
        assert ok and ni > 0.9 * nc
    if name == "scrambled":
        assert not ok and ni < 0.45 * nc
    if name == "ratio_0":
        assert ok and ni < 0.45 * nc
    if name == "ratio_1":
        assert ok == (ni == nc)
    if name == "ratio_exact":
        assert (ok, nc, ni) == (True, 200, 100) and ratio * nc == ni
    if name == "ratio_above":
        assert (ok, nc, ni) == (False, 200, 100)
    if name == "nonfinite_1997":
        assert (nc, ni) == (3, 3) and ok
    if name == "nonfinite_1998":
        assert (ok, nc, ni) == (False, 2, 0)
    if name == "sizes_2_4000":
        assert (ok, nc, ni) == (False, 2, 0)


def test_checker_drops_nonfinite_sources():
    """what vc.CHECKER_ON_FINITE_ROWS relies on, where the checker is quick: with 3 and with 30 non-finite sources its four outputs
    on the cloud are, bit for bit, those on the finite rows alone, and n_corr = n_src - k; on the large cases every non-finite row
    -- and no other -- is without a neighbour (brute force on all rows, the grid walk on 24 of the non-finite ones)"""
    src, tgt, iters, thr, ratio, seed = vc.verification_cases()["matching"]
    for k in (3, 30):
        bad, rows = vc.with_nonfinite(src, k)
        a = oi.geometric_verification(bad, tgt, iters, thr, ratio, seed)
        b = oi.geometric_verification(np.delete(bad, rows, axis=0), tgt, iters, thr, ratio, seed)
        assert a[1:] == b[1:] and a[2] == len(src) - k and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    assert np.array_equal(vc.with_nonfinite(src, 3)[0].view(np.uint32), vc.verification_cases()["nonfinite_3"][0].view(np.uint32))
    for name in vc.CHECKER_ON_FINITE_ROWS:
        bad = vc.verification_cases()[name][0]
        nonfinite = ~np.isfinite(bad[:, :3]).all(1)
        assert nonfinite.sum() == vc.NONFINITE_COUNTS[name] and len(vc.checker_source(name)) == len(bad) - nonfinite.sum()
        idx, _ = oi.nn(bad, tgt, use_grid=False)
        assert np.array_equal(idx < 0, nonfinite)
        some = bad[nonfinite][::80]
        assert len(some) >= 24 and (oi.nn(some, tgt, use_grid=True)[0] == -1).all()
        kinds = {(a, str(v)) for r in bad[nonfinite] for a, v in enumerate(r[:3]) if not np.isfinite(v)}
        assert len(kinds) == 9                                        # NaN, inf and -inf, each in x, y and z
