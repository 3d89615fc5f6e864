"""The clouds of tests/grid_cases.py reach what they are meant to reach -- checked on the CPU, with the checker's descriptor: a GPU test
that compares the engine with the checker on them proves something only if the clouds do put points next to every boundary, on both
sides of the fast binning's guard bands, and into every row and column of the grid."""
import numpy as np
import pytest

import oracle_binding as ob
from grid_cases import GRIDS, MAX_RADIUS, grid_cloud, guard_ring, guard_sect, ring_quotient, sector_quotient

IDS = [f"{r}x{s}" for r, s in GRIDS]


def _finite(cloud):
    return cloud[np.isfinite(cloud[:, :3]).all(axis=1)]


@pytest.mark.parametrize("R,S", GRIDS, ids=IDS)
def test_cloud_size_and_points_next_to_ring_and_sector_boundaries_on_each_side(R, S):
    cloud = grid_cloud(R, S)
    assert cloud.shape[1] == 8 and 4000 < cloud.shape[0] <= 30000
    pts = _finite(cloud)
    gr, gs = float(guard_ring(R)), float(guard_sect(S))
    q = ring_quotient(pts, R)
    b = np.rint(q)
    d = (q - b)[(b >= 1) & (b <= R)]
    assert np.count_nonzero((d > 0) & (d <= 2 * gr)) >= 100 and np.count_nonzero((d < 0) & (d >= -2 * gr)) >= 100
    # ... and on either side of the band's edge itself: inside it (the chain's points) and just outside (the closest sure points)
    for lo, hi in ((0.5 * gr, gr), (gr, 1.5 * gr)):
        assert np.count_nonzero((d > lo) & (d < hi)) >= 50 and np.count_nonzero((d < -lo) & (d > -hi)) >= 50, (lo, hi)
    inside = pts[(q > 0.01 * R) & (q < R)]
    t = sector_quotient(inside, S)
    e = t - np.rint(t)
    assert np.count_nonzero((e > 0) & (e <= 2 * gs)) >= 100 and np.count_nonzero((e < 0) & (e >= -2 * gs)) >= 100
    for lo, hi in ((0.5 * gs, gs), (gs, 1.5 * gs)):
        assert np.count_nonzero((e > lo) & (e < hi)) >= 50 and np.count_nonzero((e < -lo) & (e > -hi)) >= 50, (lo, hi)
    # every boundary has points within two guard widths of it
    near_r = np.unique(b[(b >= 1) & (b <= R) & (np.abs(q - b) <= 2 * gr)])
    assert near_r.size == R
    near_s = np.unique(np.mod(np.rint(t[np.abs(e) <= 2 * gs]), S))
    assert near_s.size == S


@pytest.mark.parametrize("R,S", GRIDS, ids=IDS)
def test_cloud_fills_the_first_and_last_ring_and_sector_and_every_row_and_column(R, S):
    cloud = grid_cloud(R, S)
    pts = _finite(cloud)
    q, t = ring_quotient(pts, R), sector_quotient(pts, S)
    kept = (q > 0) & (q < R)
    # counted well inside the cells (a tenth of a cell from their edges), so no rounding decides it
    ring = np.ceil(q); sect = np.ceil(t)
    clear = kept & (np.abs(q - np.rint(q)) > 0.1) & (np.abs(t - np.rint(t)) > 0.1)
    for r in (1, R):
        assert np.count_nonzero(clear & (ring == r)) >= 10, r
    for s in (1, S):
        assert np.count_nonzero(clear & (sect == s)) >= 10, s
    # just inside and just outside max_radius
    rng = np.sqrt(pts[:, 0].astype(np.float64) ** 2 + pts[:, 1].astype(np.float64) ** 2)
    assert np.count_nonzero((rng < MAX_RADIUS) & (rng > MAX_RADIUS * (1 - 2e-5))) >= 10
    assert np.count_nonzero((rng > MAX_RADIUS) & (rng < MAX_RADIUS * (1 + 2e-5))) >= 10
    desc = ob.make_scancontext(ob.make_config(R=R, S=S), cloud).reshape(R, S)
    assert (desc != 0).any(axis=1).all() and (desc != 0).any(axis=0).all()


def test_the_special_values_are_in_every_cloud():
    for R, S in GRIDS[:4]:
        cloud = grid_cloud(R, S)
        assert np.isnan(cloud[:, 0]).any() and np.isnan(cloud[:, 2]).any() and np.isinf(cloud[:, 0]).any()
        assert ((cloud[:, 0] == 0) & np.signbit(cloud[:, 0])).any() and (np.abs(cloud[:, 1]) > 1e7).any()
