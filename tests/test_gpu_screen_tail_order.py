"""The order of the finishing workgroups of a screening launch (sc_screen.hip: finish_block_of) and the scan's ring key staged in
LDS, against the CPU checker.  A finishing workgroup's index is dealt to (scan, chunk of 256 keyframes) in groups of eight chunks,
the grid is rounded up to whole groups, and workgroups behind the last chunk leave at once: the shapes here are the smallest at
which that can go wrong -- chunk counts that are no multiple of eight (1, 7, 9, 18) and one that is (8), fewer chunks than a
group, launches of 2, 4, 5 and 16 scans, and scans of one launch whose ranges end in different chunks.  Every scan of every case
is compared; the checker's distances are computed once per grid (threaded) and shared."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_binding as ob
from scl_slam_amd import ScanContextEngine
from scl_slam_amd.synth import synth_descriptors

pytestmark = pytest.mark.gpu
THREADS = min(16, os.cpu_count() or 1)
NQ = 16


class World:
    """n keyframes + 16 scans (rotated, perturbed copies of keyframes all over the database) on the engine and on the checker,
    and the checker's distance and shift of every (scan, keyframe) pair"""

    def __init__(self, R, S, n):
        self.R, self.S, self.n = R, S, n
        descs = synth_descriptors(n + NQ, R, S, seed=2024, revisit_frac=0.05)
        rs = np.random.RandomState(5)
        # what the screening cannot bound: all-zero, sparse, huge and NaN keyframes -- in the first chunk and at chunk edges
        descs[30] = 0.0; descs[31][:, ::3] = 0.0; descs[32] = descs[n - 1] * np.float32(1e25); descs[33][5, 7] = np.nan
        descs[255] = 0.0; descs[256][5, 7] = np.nan; descs[2047][:, ::3] = 0.0; descs[2048] = 0.0
        for i in range(NQ):
            src = descs[int(rs.randint(40, n - 40))]
            d = np.roll(src, int(rs.randint(0, S)), axis=1)
            descs[n + i] = np.clip(d + np.float32(10.0 ** -(i % 4 + 2)) * rs.standard_normal(d.shape).astype(np.float32) * (d > 0), 0, None)
        self.eng = ScanContextEngine(num_ring=R, num_sector=S, num_candidates=3, initial_capacity=n + NQ)
        self.db = ob.OracleDB(ob.make_config(R=R, S=S, k=3))
        self.eng.save_bulk(descs); self.db.save_bulk(descs)
        self.scans = np.arange(n, n + NQ, dtype=np.int32)
        cand = np.arange(n, dtype=np.int32)
        ref = [self.db.distance_batch_mt(int(q), cand, True, THREADS) for q in self.scans]
        self.d_ref = np.stack([r[0] for r in ref]); self.s_ref = np.stack([r[1] for r in ref])
        self.d_ref.setflags(write=False); self.s_ref.setflags(write=False)

    def winner(self, i, lo, hi):
        """the checker's (index, shift, distance) of scan i over [lo, hi): the first minimum; None where no keyframe has a distance"""
        if hi <= lo:
            return None
        d = self.d_ref[i, lo:hi]
        ok = d < 1e7
        if not ok.any():
            return None
        b = int(np.flatnonzero(ok)[np.argmin(d[ok])])
        return lo + b, int(self.s_ref[i, lo + b]), d[b]

    def close(self):
        self.eng.close(); self.db.close()


@pytest.fixture(scope="module")
def world():
    w = World(64, 120, 4400)
    yield w
    w.close()


@pytest.fixture(scope="module")
def wide():
    w = World(80, 180, 2100)
    yield w
    w.close()


def check_launches(w, lo, hi, launches):
    """screen_distances_many over [lo, hi) for launches of the given sizes: every finite value within the engine's eps of the
    checker's distance, keyframes without a distance flagged; returns the worst error"""
    worst = 0.0
    for nq in launches:
        first = NQ - nq
        approx, eps = w.eng.screen_distances_many(w.scans[first:], lo, hi)
        assert approx.shape == (nq, hi - lo)
        for i in range(nq):
            a, d_ref = approx[i], w.d_ref[first + i, lo:hi]
            finite = np.isfinite(a)
            ok = d_ref < 1e7
            assert np.all(a[~ok & ~np.isneginf(a)] == np.inf), (nq, i)
            err = np.abs(a[finite & ok].astype(np.float64) - d_ref[finite & ok])
            assert err.size == 0 or err.max() <= eps, (nq, i, float(err.max()), eps)
            assert finite[ok].mean() > 0.9 or ok.sum() < 8, (nq, i)           # the bound is met by values, not by flagging everything
            worst = max(worst, float(err.max()) if err.size else 0.0)
    print(f"{w.R}x{w.S} [{lo}, {hi}) launches of {launches}: worst |d~ - d| = {worst:.3e}")
    return worst


@pytest.mark.parametrize("lo,size", [(0, 200), (0, 1792), (0, 2048), (0, 2049), (0, 4353), (3, 2049)])
def test_launches_of_4_5_and_16_scans_over_1_to_18_chunks(world, lo, size):
    """64 x 120: 1, 7, 8, 9 and 18 chunks of 256 keyframes, and nine chunks that start at keyframe 3"""
    assert check_launches(world, lo, lo + size, (4, 5, 16)) < 4e-4


@pytest.mark.parametrize("size", [255, 2049])
def test_launches_of_2_and_16_scans_on_the_80x180_grid(wide, size):
    """80 x 180 (twenty ring groups: the keyframe's ring key is asked for behind the barrier, the scan's comes from LDS all the same)"""
    assert check_launches(wide, 0, size, (2, 16)) < 4e-4


def ragged(w, his):
    qs = np.resize(w.scans, len(his)).astype(np.int32)
    nn, sh, dd = w.eng.detect_full_stream(qs, 0, np.asarray(his, dtype=np.int32), 16, 2)
    for i, hi in enumerate(his):
        want = w.winner(i % NQ, 0, int(hi))
        if want is None:
            assert nn[i] == -1, (i, hi, nn[i])
            continue
        assert (nn[i], sh[i]) == want[:2] and dd[i].view(np.uint64) == want[2].view(np.uint64), (i, hi, nn[i], sh[i], want)


def test_ragged_launches_of_the_stream(world):
    """32 scans, 16 per launch, hi_i = hi - 257 i: the scans of a launch end in different chunks (the launch's grid is sized by its
    longest range; the other scans' workgroups behind their last chunk find nobody alive).  Once with i counted over the call --
    ranges of 18 chunks down to one, the scans behind them with nothing to score -- and once counted within each launch from a
    multiple of 257, so that every launch ends in a scan of exactly one full chunk."""
    ragged(world, [4400 - 257 * i for i in range(32)])
    ragged(world, [4112 - 257 * (i % 16) for i in range(32)])


def test_ragged_launches_with_the_second_form_on_every_batch():
    """... and with SCL_SCREEN_V2_MIN=1 (read once per process: a child interpreter), where the short launches at the end of the
    call finish by the same workgroup order as well"""
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x", "-k", "ragged_launches_of_the_stream"],
                         env=dict(os.environ, SCL_SCREEN_V2_MIN="1"), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]


def test_ring_key_metric_of_every_scan(world):
    """The finishing forms nanoflann's metric of every pair from the scan's ring key in LDS.  scl_detect_full_submit_many launches
    four scans at a time and scl_get_last_topk reports the FIRST scan of the last launch (it does not report the other scans of a
    batched pass), so sixteen launches of four put every scan in front once: after each collected ticket the candidates must be the
    checker's -- indices and the bits of the metric -- and every ticket's winner the checker's."""
    w, lo, hi = world, 0, 2049
    keys = w.db.ringkeys(hi)[lo:]
    for i in range(NQ):
        group = [(i + j) % NQ for j in range(4)]
        o_idx, o_d2, o_found = ob.knn(keys, w.db.ringkey(int(w.scans[i])), 3)
        assert o_found == 3
        tickets = w.eng.detect_full_submit_many(w.scans[group], lo, hi)
        for j, t in zip(group, tickets):
            nn, sh, d = w.eng.detect_full_collect(t)
            want = w.winner(j, lo, hi)
            assert (nn, sh) == want[:2] and np.float64(d).view(np.uint64) == want[2].view(np.uint64), (i, j, nn, sh, want)
            idx, d2 = w.eng.last_topk(3)
            assert list(idx) == [int(x) + lo for x in o_idx], (i, j, idx, o_idx)
            assert np.array_equal(d2.view(np.uint32), o_d2.view(np.uint32)), (i, j)


def test_matrix_rows_through_the_finishing_with_shift_masks(world):
    """sc_distance_matrix: the finishing with MASKS = true leaves the shifts the exact evaluation still has to score.  16 rows over
    nine chunks (one launch group: the stand-alone finishing), then the same rows twice (two groups: the first one's finishing
    rides beside the second one's alignment in the tail launch).  Every pair's distance and shift are the checker's, bit for bit."""
    w, lo, hi = world, 0, 2049
    for rows in (np.arange(NQ), np.concatenate([np.arange(NQ), np.arange(NQ)])):
        d, s = w.eng.sc_distance_matrix(w.scans[rows], lo, hi)
        assert d.shape == (len(rows), hi - lo)
        for r, i in enumerate(rows):
            same = d[r].view(np.uint64) == w.d_ref[i, lo:hi].view(np.uint64)
            assert same.all() and np.array_equal(s[r], w.s_ref[i, lo:hi]), (r, int(np.argmin(same)))
