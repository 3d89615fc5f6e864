"""Every grid scl_create accepts answers as the CPU checker does -- on the named grids of tests/grid_cases.py, which sit on the edges
of the kernels' grid-dependent paths (csrc/grid_limits.hpp has the limits, tests/test_grid_limits.py the refused side):

  descriptor parity   scl_make_descriptor, scl_make_and_save and scl_make_and_save_many on the grid's cloud (boundary points, guard-band
                      points, special values; tests/test_grid_cases.py shows it reaches them) against the checker's values and ring
                      key, bit for bit; the sector key against a second engine fed the checker's values through scl_save_bulk;
  search parity       40 keyframes saved from points, revisits turned by whole sectors: the full-range detection, the ring-key top-k
                      and rows of the distance matrix against the checker;
  margin              scl_selftest_bin_margin: the fast binning never disagrees with the reference's chain where it is sure, and its
                      quotients stay within a QUARTER of the grid's guard of the chain's -- the project's rule is "guards = four times
                      the derived error" (csrc/device_common.hpp), so the bound is that rule and not a measurement; the measured
                      maxima are printed and recorded in profiles/grids/README.md."""
import numpy as np
import pytest

import oracle_binding as ob
from grid_cases import GRIDS, SEARCH_GRIDS, grid_cloud, guard_ring, guard_sect, rotated
from scl_slam_amd import ScanContextEngine
from scl_slam_amd.synth import synth_scan

pytestmark = pytest.mark.gpu


def ids(grids):
    return [f"{r}x{s}" for r, s in grids]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(u), b.view(u))


def restride(cloud, floats):
    out = np.zeros((cloud.shape[0], floats), np.float32)
    out[:, :3] = cloud[:, :3]
    return out


@pytest.mark.parametrize("R,S", GRIDS, ids=ids(GRIDS))
def test_descriptor_front_end_equals_the_checker(R, S):
    cloud = grid_cloud(R, S)
    cfg = ob.make_config(R=R, S=S)
    eng = ScanContextEngine(num_ring=R, num_sector=S, initial_capacity=32)
    db = ob.OracleDB(cfg)
    want = ob.make_scancontext(cfg, cloud)
    assert same_bits(eng.make_descriptor(cloud), want)
    assert eng.get_size() == 0
    assert same_bits(eng.make_and_save(cloud, 0, 0), db.make_and_save(cloud, 0, 0))
    # six ragged clouds per record stride (12, 16 and 32 bytes), one of them empty, one longer than a scatter workgroup's slice
    cuts = [(0, 9001), (9001, 9258), (0, 0), (10000, 14097), (15000, 27345), (cloud.shape[0] - 1, cloud.shape[0])]
    for floats in (3, 4, 8):
        batch = [restride(cloud[a:b], floats) for a, b in cuts]
        first = eng.get_size()
        vals = eng.make_and_save_many(batch, robots=[1] * 6, indexs=list(range(first, first + 6)))
        for j, c in enumerate(batch):
            assert same_bits(vals[j], db.make_and_save(c, 1, first + j)), (floats, j)
    n = eng.get_size()
    assert n == db.size() == 19
    values = eng.get_descriptors(0, n)[:n]
    fed = ScanContextEngine(num_ring=R, num_sector=S, initial_capacity=32)
    fed.save_bulk(values)
    for i in range(n):
        assert same_bits(eng.get_ringkey(i), db.ringkey(i)), i
        assert same_bits(fed.get_ringkey(i), db.ringkey(i)), i
        assert same_bits(eng.get_sectorkey(i), fed.get_sectorkey(i)), i
    # the sector key itself: the column means in fp64, as the reference forms them (D.h:1482-1486: sequential over the rings)
    v0 = want.reshape(R, S).astype(np.float64)
    key = np.zeros(S)
    for r in range(R):
        key = key + v0[r]
    assert same_bits(eng.get_sectorkey(0), key / float(R))
    eng.close(); fed.close(); db.close()


@pytest.mark.parametrize("R,S", SEARCH_GRIDS, ids=ids(SEARCH_GRIDS))
def test_plain_search_equals_the_checker(R, S):
    n, excl = 40, 5
    turn = 7 % S if 7 % S else 3
    eng = ScanContextEngine(num_ring=R, num_sector=S, num_exclude_recent=excl, initial_capacity=64)
    db = ob.OracleDB(ob.make_config(R=R, S=S, exclude_recent=excl))
    clouds = []
    for i in range(n):
        c = grid_cloud(R, S)[:8000] if i == 0 else synth_scan(5000 + 300 * (i % 5), seed=3000 + 41 * R + i)
        if i >= excl + 2 and i % 3 == 0:                                   # a revisit of scan i - excl - 2, turned by whole sectors
            c = rotated(clouds[i - excl - 2], turn, S)
        clouds.append(c)
        assert same_bits(eng.make_and_save(c, 0, i), db.make_and_save(c, 0, i)), i
    found = 0
    for key in (39, 38, 36, 21, 9, 7):
        g = eng.detect_full_range(key, 0, max(0, key - excl))
        o_lid, o_nn, o_sh, o_dist = db.detect_full(key)
        if o_nn >= 0:
            assert (g[0], g[1]) == (o_nn, o_sh) and same_bits(np.float64(g[2]), np.float64(o_dist)), (key, g, o_nn, o_sh, o_dist)
            found += g[2] < 0.05
        else:
            assert g[0] == -1, (key, g)
    assert found >= 3                                                       # keys 39, 36, 21, 9 are revisits
    keys = db.ringkeys()
    for k in (1, 3, 25):
        for q, lo, hi in ((39, 0, 34), (17, 2, 31)):
            idx, d2, cnt = eng.ringkey_topk(q, lo, hi, k)
            o_idx, o_d2, o_cnt = ob.knn(keys[lo:hi], keys[q], k)
            assert cnt == o_cnt == k, (k, q)
            assert np.array_equal(idx, (o_idx + lo).astype(np.int32)) and same_bits(d2, o_d2), (k, q, idx, o_idx + lo)
    rows = [39, 5, 22]
    dist, shift = eng.sc_distance_matrix(rows, 0, n)
    for j, q in enumerate(rows):
        o_dist, o_shift = db.distance_batch(q, n=n)
        assert same_bits(dist[j], o_dist) and np.array_equal(shift[j], o_shift), (q, np.flatnonzero(dist[j] != o_dist)[:5])
        b_dist, b_shift = eng.sc_distance_batch(q, n=n)
        assert same_bits(b_dist, o_dist) and np.array_equal(b_shift, o_shift), q
    eng.close(); db.close()


@pytest.mark.parametrize("R,S", GRIDS, ids=ids(GRIDS))
def test_fast_binning_keeps_a_quarter_of_its_guard_on_every_grid(R, S):
    eng = ScanContextEngine(num_ring=R, num_sector=S, initial_capacity=4)
    gr, gs = float(guard_ring(R)), float(guard_sect(S))
    got = []
    for mode, n in ((0, 1 << 26), (1, 1 << 24), (2, 1 << 24)):
        bad, sure, dev_r, dev_s = eng.selftest_bin_margin(mode, 0x5c1 + 977 * mode + R * 1024 + S, n)
        print(f"bin margin {R}x{S} mode {mode}: {n} points, {sure} sure, {bad} disagreements, ring deviation {dev_r:.3e} "
              f"(guard {gr:.3e}), sector deviation {dev_s:.3e} (guard {gs:.3e})")
        got.append((mode, n, bad, sure, dev_r, dev_s))
    eng.close()
    for mode, n, bad, sure, dev_r, dev_s in got:
        assert bad == 0, (mode, bad)
        # uniform points: a point is unsure inside a guard band (2 gr + 2 gs of them, below 2e-3) or on an axis.  At the bands' edges
        # the float rounding of the generated coordinates (6e-8 of the quotient, up to a twentieth of the guard) puts a few inside
        assert sure > (0.99 if mode == 0 else 0.9) * n, (mode, sure, n)
        if mode == 0 and R >= 5:
            # ... and the bands are as wide as THIS grid's guards say (a guard that stopped growing with the grid would pass every
            # line above): the unsure share of uniform points is the bands' measure, 2 gr + 2 gs.  Off by the quotients' float
            # steps (a band is a whole number of them: at most one step in the 20 or more of a band's width, and only in the
            # quotient's highest binade) and by the ring quotient's uneven density on few rings (R >= 5: below 2 %) -- 3 %
            assert abs((n - sure) / n / (2 * gr + 2 * gs) - 1.0) <= 0.03, (n - sure, n, gr, gs)
        assert dev_r <= gr / 4, (mode, dev_r, gr)
        assert dev_s <= gs / 4, (mode, dev_s, gs)
