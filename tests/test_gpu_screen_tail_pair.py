"""A pair of the 64 x 120 stream has ONE tail launch (sc_screen.hip: sc_screen2_tail_pair_kernel): both sets finish in one grid and
the alignment of the group(s) behind the pair -- for a pair behind it, one wave per keyframe of the union of both groups' ranges,
the keyframe's image, LDS tile and A fragments shared between the two sets (sc_align2_pair_role).  SCL_TAIL_PAIR=0 keeps a tail per
set.  Every stream call here must give the CPU checker's first minimum per scan -- index, shift and the bits of the fp64 distance --
and equal the same call under SCL_TAIL_PAIR=0 in winners, survivor sum and max, aligned pairs, exact fall-backs and profile entries.

test_gpu_screen_pair.py resizes 16 scans to the call's length, so both sets of a pair hold the same scans there: a joint role that
used set 0's keys or buffers for set 1 would pass it.  Here a call cycles through 32 DISTINCT scans (rotated, perturbed copies of
keyframes), so the two sets of every pair differ.  Among the keyframes: what the filters cannot decide (all-zero, sparse, huge and
NaN ones) and eleven that are periodic in the sectors (a 30-sector pattern tiled four times): their correlation ties between four
shifts, so both filter stages leave every pair with them open and the exact fp64 evaluation decides -- the fall-back counts are
then not zero, which is checked on the numbers of the SCL_TAIL_PAIR=0 child.

Keyframe counts sit at the edges of the launch: an alignment workgroup's four waves and twelve keyframes (1, 3, 12, 13), a finishing
chunk of 256 (255, 256, 257), a group of eight chunks (2 048, 2 049), and one count 300 past the alignment's cap of 12 x 2 x CUs
keyframes per pass of its grid (waves then take a second keyframe).  Scan counts, 16 per launch: 32 (one pair, nothing to align), 48
(the joint tail aligns ONE group), 64 (two groups), 80, 33 (a one-scan group behind the pair: the products' first form, two tails),
144 (the last pair of a 128-scan chunk aligns a single group of the next chunk), 160 (... the next chunk's pair, behind the wait for
that chunk's buffer sets).  Ranges that differ between the sets: see range_cases.

The checker's distances are computed once per module (threaded); the SCL_TAIL_PAIR=0 calls run once, in one child interpreter (the
switch is read once per process), which writes every case's results to a file."""
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
NQ = 16                      # scans per launch
NSCAN = 32                   # distinct scans of the world: the two sets of a pair never hold the same ones
SCAN_COUNTS = (32, 48, 64, 80, 33, 144, 160)
PERIODIC = (2, 5, 11, 100, 254, 257, 2046, 2049, 3000, 4100, 6200)   # keyframes whose sector key has period 30: alignment ties


def align_cap():
    """keyframes one pass of the alignment's grid takes on the default device: 2 workgroups per CU, 12 keyframes each"""
    import torch
    return 12 * 2 * torch.cuda.get_device_properties(0).multi_processor_count


def keyframe_counts(n_main):
    return (1, 3, 12, 13, 255, 256, 257, 2048, 2049, n_main)


def descriptors(n):
    """n keyframes + 32 scans.  Keyframes: synthetic, with the undecidable and the periodic ones in the first workgroup's share, at
    chunk edges and all over the database; scans: rotated, perturbed copies of keyframes, half of them of keyframes below 256 so
    that the short ranges hold near matches too"""
    R, S = 64, 120
    descs = synth_descriptors(n + NSCAN, R, S, seed=2025, revisit_frac=0.05)
    rs = np.random.RandomState(7)
    descs[30] = 0.0; descs[31][:, ::3] = 0.0; descs[32] = descs[n - 1] * np.float32(1e25); descs[33][5, 7] = np.nan
    descs[255] = 0.0; descs[256][5, 7] = np.nan
    descs[2047][:, ::3] = 0.0; descs[2048] = 0.0
    for i in PERIODIC:
        if i < n:
            descs[i] = np.tile(descs[i][:, :30], (1, 4))
    for i in range(NSCAN):
        src = descs[int(rs.randint(40, 250 if i % 2 else n - 40))]
        d = np.roll(src, int(rs.randint(0, S)), axis=1)
        descs[n + i] = np.clip(d + np.float32(10.0 ** -(i % 4 + 2)) * rs.standard_normal(d.shape).astype(np.float32) * (d > 0), 0, None)
    return descs


def range_cases(n_main):
    """name -> (lo, hi) per scan of the call (16 per launch): ranges that differ between the two sets of a pair"""
    out = {}
    # three pairs; pairs 0 and 1 end in a joint tail.  Pair 0: set 0 ends inside the first chunk, set 1 spans nine chunks; pair 1 the
    # other way round -- the finishing grid is sized for the longer set either way
    i = np.arange(96)
    hi = np.where(i < 16, 100 + i, np.where(i < 32, 2048 + 50 + i, np.where(i < 48, 2048 + 7 * (i - 32), np.where(i < 64, 17 + i, 1500))))
    out["finishing_grids_differ"] = (np.zeros(96, np.int64), hi.astype(np.int64))
    # the pair behind the first has disjoint ranges with a hole between them (keyframes in one set only, or in neither); so has the third
    lo = np.where(i < 32, 0, np.where(i < 48, 3 * (i - 32), np.where(i < 64, 1000 + (i - 48), np.where(i < 80, 2100, 10 + i))))
    hi = np.where(i < 32, 1800, np.where(i < 48, 300 + (i - 32), np.where(i < 64, 1500 - (i - 48), np.where(i < 80, 2100 + 270 + i, 700))))
    out["disjoint_with_a_hole"] = (lo.astype(np.int64), hi.astype(np.int64))
    # one empty range inside a pair: 65 scans, 64 to score -- the groups are cut one scan later from there on
    j = np.arange(65)
    lo = np.zeros(65, np.int64); hi = 2300 + 3 * j.astype(np.int64); lo[20] = 700; hi[20] = 700
    out["one_empty_of_65"] = (lo, hi)
    # ranges that end mid-chunk, some a keyframe past a chunk's edge, one at the database's end
    k = np.arange(64)
    hi = np.full(64, 256 * 5 + 100, np.int64); hi[k % 3 == 1] = 256 * 2 + 1; hi[k % 5 == 2] = 256 * 3 - 1; hi[37] = n_main
    out["ends_mid_chunk"] = (np.where(k % 4 == 3, 129, 0).astype(np.int64), hi)
    return out


def stream(eng, scans, lo, hi):
    """one stream call, 16 scans per launch (scan i of the call = scan i mod 32 of the world) -> index, shift and distance bits per
    scan, and [survivor sum, survivor max, aligned pairs, exact fall-backs, profile entries of the screening launches]"""
    qs = np.resize(scans, len(lo)).astype(np.int32)
    eng.survivor_stats(reset=True); eng.alignment_stats(reset=True)
    eng.profile_reset(); eng.profile_enable(2)
    nn, sh, dd = eng.detect_full_stream(qs, np.asarray(lo, dtype=np.int32), np.asarray(hi, dtype=np.int32), NQ, 2)
    eng.profile_enable(False)
    sv = eng.survivor_stats(); al = eng.alignment_stats()
    stats = np.array([sv[1], sv[2], al[0], al[1], eng.profile()["sc_distance_launches"]], dtype=np.int64)
    return nn.astype(np.int64), sh.astype(np.int64), dd.view(np.uint64).copy(), stats


def run_cases(eng, scans, n_main):
    out = {}
    for nk in keyframe_counts(n_main):
        for m in SCAN_COUNTS:
            out[f"kf{nk}_m{m}"] = stream(eng, scans, np.zeros(m, np.int64), np.full(m, nk, np.int64))
    for name, (lo, hi) in range_cases(n_main).items():
        out[name] = stream(eng, scans, lo, hi)
    return out


def child(path):
    """the same calls with whatever SCL_TAIL_PAIR the environment holds; results to `path`"""
    n_main = align_cap() + 300
    eng = ScanContextEngine(num_ring=64, num_sector=120, num_candidates=3, initial_capacity=n_main + NSCAN)
    eng.save_bulk(descriptors(n_main))
    res = run_cases(eng, np.arange(n_main, n_main + NSCAN, dtype=np.int32), n_main)
    eng.close()
    np.savez(path, **{f"{k}/{j}": v[j] for k, v in res.items() for j in range(4)})


class World:
    def __init__(self, n):
        import oracle_binding as ob
        self.n = n
        descs = descriptors(n)
        self.eng = ScanContextEngine(num_ring=64, num_sector=120, num_candidates=3, initial_capacity=n + NSCAN)
        self.db = ob.OracleDB(ob.make_config(R=64, S=120, k=3))
        self.eng.save_bulk(descs); self.db.save_bulk(descs)
        self.scans = np.arange(n, n + NSCAN, dtype=np.int32)
        cand = np.arange(n, dtype=np.int32)
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
            want = self.winner(i % NSCAN, int(lo[i]), int(hi[i]))
            if want is None:
                assert nn[i] == -1, (i, nn[i])
                continue
            assert (int(nn[i]), int(sh[i]), int(dd[i])) == want, (i, int(lo[i]), int(hi[i]), nn[i], sh[i], want)

    def close(self):
        self.eng.close(); self.db.close()


@pytest.fixture(scope="module")
def n_main():
    return align_cap() + 300


@pytest.fixture(scope="module")
def world(n_main):
    w = World(n_main)
    yield w
    w.close()


@pytest.fixture(scope="module")
def tail_per_set(tmp_path_factory):
    """every case of this module with SCL_TAIL_PAIR=0, from one fresh interpreter"""
    path = str(tmp_path_factory.mktemp("tail_pair") / "tail_per_set.npz")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=dict(os.environ, SCL_TAIL_PAIR="0"),
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def same_as_tail_per_set(ref, name, got):
    """winners; survivor sum and max, aligned pairs, exact fall-backs and profile entries (a pair is one entry either way)"""
    for j in range(3):
        assert np.array_equal(got[j], ref[f"{name}/{j}"]), (name, j)
    print(name, "stats", got[3].tolist(), "tail per set", ref[f"{name}/3"].tolist())
    assert np.array_equal(got[3], ref[f"{name}/3"]), (name, got[3], ref[f"{name}/3"])


@pytest.mark.parametrize("which", range(10))
def test_keyframe_counts_at_the_edges_of_the_joint_tail(world, tail_per_set, n_main, which):
    nk = keyframe_counts(n_main)[which]
    assert 0 < nk <= n_main and n_main > 2049
    for m in SCAN_COUNTS:
        lo, hi = np.zeros(m, np.int64), np.full(m, nk, np.int64)
        got = stream(world.eng, world.scans, lo, hi)
        world.check(got, lo, hi)
        same_as_tail_per_set(tail_per_set, f"kf{nk}_m{m}", got)


@pytest.mark.parametrize("name", ["finishing_grids_differ", "disjoint_with_a_hole", "one_empty_of_65", "ends_mid_chunk"])
def test_ranges_that_differ_between_the_sets(world, tail_per_set, n_main, name):
    lo, hi = range_cases(n_main)[name]
    assert hi.max() <= n_main and lo.min() >= 0
    got = stream(world.eng, world.scans, lo, hi)
    world.check(got, lo, hi)
    same_as_tail_per_set(tail_per_set, name, got)


def test_the_tail_per_set_path_takes_exact_fallbacks_where_two_sets_are_aligned(tail_per_set, n_main):
    """without this the equality of the fall-back counts would show nothing: on the SCL_TAIL_PAIR=0 child's numbers, the calls whose
    joint tails align two sets (64 scans and more) over ranges that hold periodic keyframes count exact fall-backs"""
    for name in ("kf2049_m64", f"kf{n_main}_m64", "kf13_m160", "disjoint_with_a_hole"):
        assert int(tail_per_set[f"{name}/3"][3]) > 0, (name, tail_per_set[f"{name}/3"])


if __name__ == "__main__":
    child(sys.argv[1])
