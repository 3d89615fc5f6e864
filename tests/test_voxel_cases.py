"""The CPU checker's voxel filter (oracle/icp_oracle.c, icpo_voxel_grid) pinned on the clouds of tests/voxel_cases.py -- by answers
written out by hand (which points share a voxel, the output's order, the clouds that come back unchanged) and by a second, plain
numpy statement of the filter, bit for bit -- and the conditions the cases promise.  Without this, tests/test_gpu_voxel.py's
"GPU == checker" would prove little.  No GPU needed."""
import numpy as np
import pytest

import oracle_icp_binding as oi
import voxel_cases as vc


def _centroids(cloud, groups):
    """the hand-written answer: one output point per group of rows, fp32 sums in the rows' order, other fields zero"""
    out = np.zeros((len(groups), cloud.shape[1]), np.float32)
    for g, rows in enumerate(groups):
        for col in (0, 1, 2, 4)[:4 if cloud.shape[1] >= 5 else 3]:
            s = np.float32(0)
            for r in rows:
                s = np.float32(s + cloud[r, col])
            out[g, col] = s / np.float32(len(rows))
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_boundary_points_by_hand():
    """leaf 0.5 (1 / leaf = 2 exactly), nine points on a line: floor, not truncation, and a voxel's lower face belongs to it"""
    f = np.float32
    dn, up = (lambda v: np.nextafter(f(v), f(-np.inf))), (lambda v: np.nextafter(f(v), f(np.inf)))
    xs = [f(-1.0), dn(-1.0), up(-1.0), f(-0.5), f(-0.0), f(0.0), dn(0.0), f(0.5), dn(0.5)]
    #     voxel -2    -3        -2        -1        0        0       -1       1        0       (truncation would put 3, 6 into voxel 0)
    groups = [[1], [0, 2], [3, 6], [4, 5, 8], [7]]
    for axis in range(3):
        c = np.full((9, 8), 0.25, np.float32); c[:, 3:] = 0
        c[:, axis] = xs; c[:, 4] = np.arange(9)
        want = _centroids(c, groups)
        assert np.array_equal(_bits(oi.voxel_grid(c, 0.5)), _bits(want))
        assert np.array_equal(_bits(vc.restate(c, 0.5)), _bits(want))


@pytest.mark.parametrize("leaf", [0.25, 0.5])
def test_boundary_case_lines_on_exact_leaves(leaf):
    """k * leaf and its upper neighbour lie in voxel k, its lower neighbour in voxel k - 1; both zeros in voxel 0"""
    vals = vc.boundary_values(leaf)
    c = np.zeros((vals.size, 3), np.float32); c[:, 0] = vals
    rows, f = vc.voxel_index(c, leaf)
    k = np.arange(-40, 41)
    assert rows.size == vals.size
    assert np.array_equal(f[:-2, 0].reshape(81, 3), np.stack([k, k, k - 1], 1)) and list(f[-2:, 0]) == [0, 0]
    # ... and that is how the checker groups them: 82 voxels (-41 .. 40), voxel -41 holds one point, voxel 40 two, 0 five, the others three
    o = oi.voxel_grid(c, leaf)
    assert o.shape[0] == 82
    groups = [[2]] + [[3 * i, 3 * i + 1, 3 * (i + 1) + 2] + ([243, 244] if i == 40 else []) for i in range(80)] + [[240, 241]]
    assert np.array_equal(_bits(o), _bits(_centroids(c, groups)))


def test_index_range_by_hand():
    cs = vc.cases()
    c, leaf = cs["index_below_2_31"]                                  # 2048 x 1024 x 1023 = 2^31 - 2^21 voxels: filtered
    want = _centroids(c, [[0, 4], [3], [1, 2]])                       # voxels 0, 1000 + 500 * 2048 + 511 * 2^21, 2^31 - 2^21 - 1
    assert np.array_equal(_bits(oi.voxel_grid(c, leaf)), _bits(want))
    c, leaf = cs["index_2_31"]                                        # 2048 x 1024 x 1024 = 2^31 voxels: one too many
    assert oi.voxel_grid(c, leaf) is None and vc.restate(c, leaf) is None
    c, leaf = cs["index_min_int"]                                     # floor = -2^31 is an int32
    o = oi.voxel_grid(c, leaf)
    assert o.shape == (1, 8) and o[0, 0] == -2147483648.0 and o[0, 4] == 7 and not o[0, [1, 2, 3, 5, 6, 7]].any()
    c, leaf = cs["index_inf_inv"]                                     # 1 / 1e-39 = inf in fp32
    with np.errstate(over="ignore"):
        assert np.isinf(np.float32(1) / np.float32(leaf)) and np.float32(leaf) > 0
    assert oi.voxel_grid(c, leaf) is None and vc.restate(c, leaf) is None


def test_strides_by_hand():
    """two voxels of leaf 1; every field filled with other values: x, y, z always, the intensity from 20 bytes up, zero elsewhere"""
    for stride in vc.STRIDES:
        w = stride // 4
        c = np.arange(1, 4 * w + 1, dtype=np.float32).reshape(4, w) * 0.5 + 100
        c[:, :3] = [[1.25, 0.5, 0.5], [0.25, 0.5, 0.75], [1.5, 0.25, 0.5], [0.75, 0.5, 0.25]]
        o = oi.voxel_grid(c, 1.0)
        want = np.zeros((2, w), np.float32)
        want[:, :3] = [[0.5, 0.5, 0.5], [1.375, 0.375, 0.5]]          # voxel 0: rows 1, 3; voxel 1: rows 0, 2
        if w >= 5:
            want[:, 4] = [(c[1, 4] + c[3, 4]) / 2, (c[0, 4] + c[2, 4]) / 2]
        assert np.array_equal(_bits(o), _bits(want)), stride
    for stride in vc.STRIDES:
        c, leaf = vc.cases()[f"stride_{stride}"]
        o = oi.voxel_grid(c, leaf)
        keep = [0, 1, 2] + ([4] if stride >= 20 else [])
        assert o.shape[0] > 100 and not np.delete(o, keep, axis=1).any() and o[:, keep].all()


def test_all_distinct_comes_back_reversed_and_one_voxel_is_one_point():
    c, leaf = vc.cases()["all_distinct"]
    want = c[::-1].copy()
    assert np.array_equal(_bits(oi.voxel_grid(c, leaf)), _bits(want))
    c, leaf = vc.cases()["one_voxel"]
    assert np.array_equal(_bits(oi.voxel_grid(c, leaf)), _bits(_centroids(c, [list(range(5000))])))


def test_nonfinite_cases_by_hand():
    cs = vc.cases()
    c, leaf = cs["nonfinite_mixed"]
    bad = ~np.isfinite(c[:, :3]).all(1)
    assert list(np.nonzero(bad)[0]) == [0, 1, 254, 255, 256, 257, 258, 598, 599]
    seen = {(a, str(c[r, a])) for r in np.nonzero(bad)[0] for a in range(3) if not np.isfinite(c[r, a])}
    assert len(seen) == 9 and (~np.isfinite(c[bad, :3])).sum() == 9   # NaN, inf, -inf in x only, y only, z only
    assert np.array_equal(_bits(oi.voxel_grid(c, leaf)), _bits(oi.voxel_grid(c[~bad], leaf)))
    c, leaf = cs["nonfinite_all"]
    assert not np.isfinite(c[:, :3]).all(1).any() and oi.voxel_grid(c, leaf).shape == (0, 8)
    c, leaf = cs["nonfinite_fields"]
    assert np.isfinite(c[:, :3]).all() and np.isnan(c[:, 4]).sum() == 6 and np.isnan(c[:, 6]).sum() == 4
    o = oi.voxel_grid(c, leaf)
    clean = c.copy(); clean[np.isnan(c[:, 4]), 4] = 0
    p = oi.voxel_grid(clean, leaf)                                    # the points stay: same voxels, same coordinates
    assert o.shape == p.shape and np.array_equal(_bits(o[:, :4]), _bits(p[:, :4])) and not o[:, 5:].any()
    assert 1 <= np.isnan(o[:, 4]).sum() <= 6 and np.array_equal(_bits(o[~np.isnan(o[:, 4])]), _bits(p[~np.isnan(o[:, 4])]))


def test_order_case_depends_on_the_order_of_a_voxels_points():
    """in at least half of the 200 voxels the fp32 sums the centroid is made of (x, y, z, intensity), taken in reversed point order,
    differ in bits from the sums in input order: a sort that does not keep a voxel's points in input order cannot pass.  (All four
    sums count: a sum of positive numbers lies within an ulp of the exact one in either order, so ONE coordinate's two sums agree
    about every other time however the magnitudes are spread -- x alone: 80 to 90 of 200 --, and a wrong order shows in any of them.)"""
    c, leaf = vc.cases()["order"]
    rows, f = vc.voxel_index(c, leaf)
    vox = (f[:, 1] + 20 * f[:, 2]).astype(int)
    assert rows.size == c.shape[0] and set(vox) == set(range(200)) and not f[:, 0].any()
    differ = differ_x = 0
    for v in range(200):
        p = c[vox == v][:, [0, 1, 2, 4]]
        x = p[:, 0]
        assert 3 <= x.size <= 9 and 2.0 ** 12 <= x.max() / x.min() <= 2.0 ** 21
        fwd, rev = np.zeros(4, np.float32), np.zeros(4, np.float32)
        for a, b in zip(p, p[::-1]):
            fwd, rev = fwd + a, rev + b
        differ += (fwd.view(np.uint32) != rev.view(np.uint32)).any()
        differ_x += fwd.view(np.uint32)[0] != rev.view(np.uint32)[0]
    assert differ >= 100 and differ_x >= 50, (differ, differ_x)
    first = np.array([np.nonzero(vox == v)[0][0] for v in range(200)])
    assert (np.diff(first) < 0).sum() > 50                            # scattered: the voxels do not appear in their order either


def test_subnormal_case_stays_subnormal():
    tiny = np.float32(2.0 ** -126)
    for name in ("subnormal", "subnormal_leaf"):
        c, leaf = vc.cases()[name]
        assert (np.abs(c[:, [0, 1, 2, 4]]) < tiny).all() and (c[:, [0, 1, 2, 4]] != 0).all()
    c, leaf = vc.cases()["subnormal"]
    o = oi.voxel_grid(c, leaf)
    rows, f = vc.voxel_index(c, leaf)
    assert o.shape[0] == 8 and set(np.unique(f)) == {-1.0, 0.0}
    for v in range(8):                                                # the sums themselves, not only the centroids
        m = (f[:, 0] == v % 2 - 1) & (f[:, 1] == v // 2 % 2 - 1) & (f[:, 2] == v // 4 - 1)
        s = c[m][:, [0, 1, 2, 4]].astype(np.float64).sum(0)
        assert (np.abs(s) < 2.0 ** -126).all() and m.sum() > 10
    assert (np.abs(o[:, [0, 1, 2, 4]]) < tiny).all() and (o[:, [0, 1, 2, 4]] != 0).all()
    rows, f = vc.voxel_index(*vc.cases()["subnormal_leaf"])
    assert f.min() == -2 and f.max() == 1                              # a subnormal leaf spreads subnormal points over voxels


def test_sizes_and_case_list():
    cs = vc.cases()
    assert [cs[f"size_{n}"][0].shape[0] for n in vc.SIZES] == list(vc.SIZES)
    assert [cs[f"stride_{s}"][0].shape[1] * 4 for s in vc.STRIDES] == list(vc.STRIDES)
    assert cs["boundaries_0.1"][0][:, :3].min() < -3.9 and len(cs) == 31


@pytest.mark.parametrize("name", vc.names())
def test_restatement_equals_checker(name):
    c, leaf = vc.cases()[name]
    o, r = oi.voxel_grid(c, leaf), vc.restate(c, leaf)
    if o is None or r is None:
        assert o is None and r is None
        assert name in ("index_2_31", "index_inf_inv")
    else:
        assert name not in ("index_2_31", "index_inf_inv") and vc.same_bits(r, o)
        if not np.isnan(o).any():
            assert np.array_equal(_bits(r), _bits(o))
