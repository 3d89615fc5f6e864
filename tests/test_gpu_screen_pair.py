"""Two consecutive full launch groups of the stream form share ONE products launch on the 64 x 120 grid (sc_screen.hip:
sc_screen2_kernel with two scan sets; engine.hip: stream_screened_locked).  With two sets a launch has
W = (CUs / 32) x 8 index groups x 16 waves per (ring half, set) -- 1 024 on 256 CUs -- and a wave takes every W-th keyframe of the
union of both sets' ranges, so the edges are at keyframe counts around W, not at the workload's size: fewer keyframes than waves
(1, 15, W - 1), exactly one per wave (W), one wave with two (W + 1), two rounds and one (2 W + 1), several (4 400).  Per count the
stream runs with 16 scans per launch over 32 scans (one pair), 48 (pair + single group), 33 (pair + a one-scan group, which takes
the products' first form), 64 and 144 (crosses the 128-scan chunk: the last pair of a chunk carries the alignment of the next
chunk's first group).  Every winner is the CPU checker's first minimum -- index, shift and the bits of the distance -- and equals
the same call with SCL_SCREEN_PAIR=0; so do the survivor and alignment counts, which follow from the partial sums and the first
shifts (bit-identical by construction: a workgroup runs the single launch's instruction sequence on its own set).  The checker's
distances are computed once per module (threaded); the calls without pairs run once, in one child interpreter (the switch is read
once per process), which writes every case's results to a file."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from scl_slam_amd import ScanContextEngine
from scl_slam_amd.synth import synth_descriptors

pytestmark = pytest.mark.gpu
THREADS = min(16, os.cpu_count() or 1)
NQ = 16
N_MAIN, N_SMALL, N_APPEND = 4400, 1100, 60
SCAN_COUNTS = (32, 48, 33, 64, 144)


def waves_per_set():
    """waves of a paired launch per (ring half, set) on the default device: (CUs / 32) x 8 index groups x 16 waves"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return max(1, cus // 32) * 8 * 16


def descriptors(n):
    """n keyframes + 16 scans (rotated, perturbed copies of keyframes all over the database); among the keyframes what the
    screening cannot bound: all-zero, sparse, huge and NaN ones -- in the first chunk and at chunk edges"""
    R, S = 64, 120
    descs = synth_descriptors(n + NQ, R, S, seed=2024, revisit_frac=0.05)
    rs = np.random.RandomState(5)
    descs[30] = 0.0; descs[31][:, ::3] = 0.0; descs[32] = descs[n - 1] * np.float32(1e25); descs[33][5, 7] = np.nan
    descs[255] = 0.0; descs[256][5, 7] = np.nan
    if n > 2048:
        descs[2047][:, ::3] = 0.0; descs[2048] = 0.0
    for i in range(NQ):
        src = descs[int(rs.randint(40, n - 40))]
        d = np.roll(src, int(rs.randint(0, S)), axis=1)
        descs[n + i] = np.clip(d + np.float32(10.0 ** -(i % 4 + 2)) * rs.standard_normal(d.shape).astype(np.float32) * (d > 0), 0, None)
    return descs


def appended(descs):
    """the keyframes the append case adds between its two calls: shifted copies of keyframes of the database"""
    return np.stack([np.roll(descs[17 * j + 3], 5 + j, axis=1) for j in range(N_APPEND)])


def keyframe_counts(W):
    return (1, 15, W - 1, W, W + 1, 2 * W + 1, N_MAIN)


def range_cases():
    """name -> (lo, hi) per scan, scans per launch: ranges that differ inside a pair"""
    i = np.arange(32)
    lo_u = np.where(i < 16, 0, 500 + 13 * (i - 16)); hi_u = np.where(i < 16, 3000 - 37 * i, N_MAIN - 5 * (i - 16))
    full_lo, full_hi = np.zeros(33, np.int64), np.full(33, N_MAIN, np.int64)
    e32_hi = full_hi[:32].copy(); e32_hi[5] = 0                         # 31 scans to score: a full group and one of 15 -- no pair
    e33_lo = full_lo.copy(); e33_lo[20] = 700; e33_hi = full_hi.copy(); e33_hi[20] = 700   # 32 to score: a pair, its groups cut at scan 17
    mid_hi = full_hi[:32].copy(); mid_hi[3] = 256 * 5 + 100; mid_hi[19] = 256 * 2 + 1
    return {"unions_differ": (lo_u, hi_u, 16), "one_empty_of_32": (full_lo[:32], e32_hi, 16), "one_empty_of_33": (e33_lo, e33_hi, 16),
            "ends_mid_chunk": (full_lo[:32], mid_hi, 16), "eight_per_launch": (full_lo[:32], full_hi[:32], 8)}


def stream(eng, scans, lo, hi, spl):
    """one stream call (scan i of the call = scan i mod 16 of the world) -> index, shift and distance bits per scan, and
    [survivor sum, survivor max, aligned pairs, exact fall-backs, profile entries of the screening launches]"""
    qs = np.resize(scans, len(lo)).astype(np.int32)
    eng.survivor_stats(reset=True); eng.alignment_stats(reset=True)
    eng.profile_reset(); eng.profile_enable(2)
    nn, sh, dd = eng.detect_full_stream(qs, np.asarray(lo, dtype=np.int32), np.asarray(hi, dtype=np.int32), spl, 2)
    eng.profile_enable(False)
    sv = eng.survivor_stats(); al = eng.alignment_stats()
    stats = np.array([sv[1], sv[2], al[0], al[1], eng.profile()["sc_distance_launches"]], dtype=np.int64)
    return nn.astype(np.int64), sh.astype(np.int64), dd.view(np.uint64).copy(), stats


def run_main_cases(eng, scans, W):
    out = {}
    for nk in keyframe_counts(W):
        for m in SCAN_COUNTS:
            out[f"kf{nk}_m{m}"] = stream(eng, scans, np.zeros(m, np.int64), np.full(m, nk, np.int64), 16)
    for name, (lo, hi, spl) in range_cases().items():
        out[name] = stream(eng, scans, lo, hi, spl)
    return out


def run_append_cases(eng, scans, extra):
    out = {"append_before": stream(eng, scans, np.zeros(64, np.int64), np.full(64, N_SMALL, np.int64), 16)}
    eng.save_bulk(extra)
    total = N_SMALL + NQ + N_APPEND
    out["append_after"] = stream(eng, scans, np.zeros(64, np.int64), np.full(64, total, np.int64), 16)
    return out


def flatten(results):
    return {f"{k}/{j}": v[j] for k, v in results.items() for j in range(4)}


def child(path):
    """the same calls with whatever SCL_SCREEN_PAIR the environment holds; results to `path`"""
    W = waves_per_set()
    d = descriptors(N_MAIN)
    eng = ScanContextEngine(num_ring=64, num_sector=120, num_candidates=3, initial_capacity=N_MAIN + NQ)
    eng.save_bulk(d)
    res = run_main_cases(eng, np.arange(N_MAIN, N_MAIN + NQ, dtype=np.int32), W)
    eng.close()
    d2 = descriptors(N_SMALL)
    eng2 = ScanContextEngine(num_ring=64, num_sector=120, num_candidates=3, initial_capacity=N_SMALL + NQ)
    eng2.save_bulk(d2)
    res.update(run_append_cases(eng2, np.arange(N_SMALL, N_SMALL + NQ, dtype=np.int32), appended(d2)))
    eng2.close()
    np.savez(path, **flatten(res))


class World:
    def __init__(self, n, extra=False):
        import oracle_binding as ob
        self.n = n
        descs = descriptors(n)
        self.eng = ScanContextEngine(num_ring=64, num_sector=120, num_candidates=3, initial_capacity=n + NQ)
        self.db = ob.OracleDB(ob.make_config(R=64, S=120, k=3))
        self.eng.save_bulk(descs); self.db.save_bulk(descs)
        self.extra = appended(descs) if extra else None
        total = n
        if extra:                                            # the checker holds the appended keyframes from the start: its distances are per pair
            self.db.save_bulk(self.extra); total = n + NQ + N_APPEND
        self.scans = np.arange(n, n + NQ, dtype=np.int32)
        cand = np.arange(total, dtype=np.int32)
        ref = [self.db.distance_batch_mt(int(q), cand, True, THREADS) for q in self.scans]
        self.d_ref = np.stack([r[0] for r in ref]); self.s_ref = np.stack([r[1] for r in ref])
        self.d_ref.setflags(write=False); self.s_ref.setflags(write=False)

    def winner(self, i, lo, hi):
        """the checker's (index, shift, distance bits) of scan i over [lo, hi): the first minimum; None where no keyframe has a distance"""
        if hi <= lo:
            return None
        d = self.d_ref[i, lo:hi]
        ok = d < 1e7
        if not ok.any():
            return None
        b = int(np.flatnonzero(ok)[np.argmin(d[ok])])
        return lo + b, int(self.s_ref[i, lo + b]), int(d[b:b + 1].view(np.uint64)[0])

    def check(self, got, lo, hi):
        nn, sh, dd, _ = got
        for i in range(len(nn)):
            want = self.winner(i % NQ, int(lo[i]), int(hi[i]))
            if want is None:
                assert nn[i] == -1, (i, nn[i])
                continue
            assert (int(nn[i]), int(sh[i]), int(dd[i])) == want, (i, int(lo[i]), int(hi[i]), nn[i], sh[i], want)

    def close(self):
        self.eng.close(); self.db.close()


@pytest.fixture(scope="module")
def W():
    return waves_per_set()


@pytest.fixture(scope="module")
def world():
    w = World(N_MAIN)
    yield w
    w.close()


@pytest.fixture(scope="module")
def unpaired(tmp_path_factory):
    """every case of this module with SCL_SCREEN_PAIR=0, from one fresh interpreter"""
    path = str(tmp_path_factory.mktemp("pair") / "unpaired.npz")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=dict(os.environ, SCL_SCREEN_PAIR="0"),
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def same_as_unpaired(unpaired, name, got, launches_on, launches_off):
    """winners, survivor sum and max, alignment pairs and fallbacks equal; the profile's entries: a pair is ONE"""
    for j in range(3):
        assert np.array_equal(got[j], unpaired[f"{name}/{j}"]), (name, j)
    off = unpaired[f"{name}/3"]
    assert np.array_equal(got[3][:4], off[:4]), (name, got[3], off)
    assert (int(got[3][4]), int(off[4])) == (launches_on, launches_off), (name, got[3], off)


def launches(m, spl=16, paired=True):
    """profile entries of a stream call of m scans over non-empty ranges: per chunk of 128 scans, pairs of full groups + the rest"""
    total = 0
    for c0 in range(0, m, 128):
        mc = min(128, m - c0)
        full, rest = divmod(mc, spl)
        groups = full + (1 if rest else 0)
        total += groups - (full // 2 if paired and spl == 16 else 0)
    return total


@pytest.mark.parametrize("which", range(7))
def test_keyframe_counts_around_the_waves_of_a_set(world, unpaired, W, which):
    nk = keyframe_counts(W)[which]
    assert 0 < nk <= N_MAIN
    for m in SCAN_COUNTS:
        got = stream(world.eng, world.scans, np.zeros(m, np.int64), np.full(m, nk, np.int64), 16)
        world.check(got, np.zeros(m, np.int64), np.full(m, nk, np.int64))
        same_as_unpaired(unpaired, f"kf{nk}_m{m}", got, launches(m), launches(m, paired=False))


@pytest.mark.parametrize("name", ["unions_differ", "one_empty_of_32", "one_empty_of_33", "ends_mid_chunk", "eight_per_launch"])
def test_ranges_that_differ_inside_a_pair(world, unpaired, name):
    lo, hi, spl = range_cases()[name]
    got = stream(world.eng, world.scans, lo, hi, spl)
    world.check(got, lo, hi)
    scored = int(np.sum(hi > lo))
    same_as_unpaired(unpaired, name, got, launches(scored, spl), launches(scored, spl, paired=False))


def test_keyframes_appended_between_two_stream_calls(unpaired):
    """the capacity doubles between the calls: the second call's launches read the new arrays (the database view is formed per launch)"""
    w = World(N_SMALL, extra=True)
    try:
        res = run_append_cases(w.eng, w.scans, w.extra)
        total = N_SMALL + NQ + N_APPEND
        w.check(res["append_before"], np.zeros(64, np.int64), np.full(64, N_SMALL, np.int64))
        w.check(res["append_after"], np.zeros(64, np.int64), np.full(64, total, np.int64))
        for name in ("append_before", "append_after"):
            same_as_unpaired(unpaired, name, res[name], 2, 4)
    finally:
        w.close()


if __name__ == "__main__":
    child(sys.argv[1])
