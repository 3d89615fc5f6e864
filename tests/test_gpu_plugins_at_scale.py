"""The host layer the descriptor plugins share (scl_slam_amd/csrc/plugin_host.hpp) and Iris's own database, past the first
capacity of 256 keyframes and past one workgroup of 256 candidates.  Reference: tests/m2dp_checker.py::CheckerDB and
tests/fpfh_checker.py::FpfhChecker as tests/plugin_cases.py extends them (nanoflann's rule for NaN distances, a vectorised 1-NN
held to the loop form in tests/test_plugin_cases.py) and oracle/iris_plugin_oracle.py; loop ids equal, float distances equal by their uint32 pattern.

Which test reaches what the small suites never execute:
  * FloatRows::grow with live rows (256 -> 512 -> 1024 -> 2048, old rows copied): test_growth_keeps_every_row, and inside one
    make_and_save_many call: test_a_batch_across_the_first_boundary, test_a_rejected_batch_at_the_boundary_changes_nothing;
  * nn_l2_kernel over several workgroups, the cross-workgroup 64-bit atomicMin, explicit lists and the snapshot
    (inter_mode = 0, list == nullptr) above 256 rows, DIM % 4 == 0 (M2DP, float4 reads) and DIM % 4 != 0 (FPFH, 33 floats, tail
    loop): test_m2dp_detection_over_several_workgroups, test_fpfh_detection_over_several_workgroups, test_*_at_10000;
  * ties whose equal winners sit in different lanes, waves and workgroups: test_ties_go_to_the_lowest_position,
    test_every_candidate_the_same_row;
  * the d_list regrow of nearest_locked: test_the_list_buffer_regrows;
  * NaN / inf rows from the wire: test_non_finite_wire_rows;
  * Iris: grow() of iris.hip (images, row keys, T, M copied), iris_rowkey_d2_kernel above one workgroup and the k-nearest tie
    rule across its workgroups, the list_cap regrow: test_iris_700_keyframes_16x72; the job_cap / fm_cap / rolls_cap regrows:
    test_iris_300_keyframes_80x360_and_the_work_buffers_regrow.

Checker side of each test on the CPU, engine calls answered by the checker itself (seconds, one core): growth and batches below 0.1,
M2DP detection 0.1 - 0.6 per case, FPFH detection 0.1 - 1.0 per case, 10 000 keys 1, ties 0.1, regrow 0.1,
non-finite 1, Iris 16 x 72 6 (windows) and 2 (every shift), Iris 80 x 360 12.
"""
import numpy as np
import pytest

import oracle_binding as ob
import oracle_iris_binding as oi
from oracle.iris_plugin_oracle import IrisPluginOracle
from plugin_cases import FpfhChecker, M2dpChecker, iris_like, same_detection, same_f32, same_iris_detection, vector_rows
from scl_slam_amd.synth import synth_scan

PLUGINS = ("m2dp", "fpfh")
DIMS = {"m2dp": 192, "fpfh": 33}
SIZES = (255, 256, 257, 511, 513, 2000)


def _engine(plugin, **kw):
    if plugin == "m2dp":
        from scl_slam_amd import M2dpEngine
        return M2dpEngine(**kw)
    from scl_slam_amd import FpfhEngine
    return FpfhEngine(**kw)


def _iris_engine(**kw):
    from scl_slam_amd.iris import IrisEngine
    return IrisEngine(**kw)


def _checker(plugin, **kw):
    return M2dpChecker(vectorised=True, **kw) if plugin == "m2dp" else FpfhChecker(**kw)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _fill(e, c, rows, robot_num, first=0):
    """rows from the wire, robot = key % robot_num (interleaved arrival), index = 7 * key"""
    for i, v in enumerate(rows):
        k = first + i
        e.save_from_wire(v, k % robot_num, 7 * k)
        if c is not None:
            c.save(v, k % robot_num, 7 * k)


def _queries(n_avail, excl, count, seed):
    """the exclusion window's edges (excl, excl + 1), the first and the last index and `count` random ones of [0, n_avail)"""
    if n_avail <= 0:
        return []
    fixed = {0, min(excl, n_avail - 1), min(excl + 1, n_avail - 1), n_avail - 1}
    rs = np.random.RandomState(seed)
    return sorted(fixed | set(int(x) for x in rs.choice(n_avail, size=min(count, n_avail), replace=False)))


def _compare(e, c, form, cur, nan_ok=False):
    g = getattr(e, "detect_" + form)(cur); o = getattr(c, "detect_" + form)(cur)
    assert same_detection(g, o, nan_ok), (form, cur, g, o)
    return g


# ---- growth ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("plugin", PLUGINS)
def test_growth_keeps_every_row(plugin):
    """1 100 rows one by one: FloatRows::grow runs at rows 256, 512 and 1 024 with live rows to copy.  Around every doubling the
    first row, rows 255 / 256, the newest and 20 random ones read back as sent, uint32 for uint32, and the registry with them."""
    rows = vector_rows(plugin, 1100, seed=11)
    e = _engine(plugin, robot_num=3)
    rs = np.random.RandomState(12)
    for k in range(1100):
        e.save_from_wire(rows[k], k % 3, 7 * k)
        if k in (255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1099):
            assert e.get_size() == k + 1
            for r in sorted({0, min(255, k), min(256, k), k} | set(int(x) for x in rs.randint(0, k + 1, size=20))):
                assert np.array_equal(_bits(e.get_signature(r)), _bits(rows[r])), (k, r)
                assert e.get_index(r) == (r % 3, 7 * r) and e.local_to_global(r % 3, r // 3) == r
    e.close()


def _boundary_engine(plugin):
    rows = vector_rows(plugin, 250, seed=21)
    e = _engine(plugin, robot_num=2)
    _fill(e, None, rows, 2)
    clouds = [synth_scan(1500 + 40 * i, seed=900 + i) for i in range(16)]
    singles = np.stack([e.make(c) for c in clouds])              # single scans: nothing stored
    assert e.get_size() == 250
    return e, rows, clouds, singles


def _check_batch_landed(e, rows, clouds, singles):
    robots = [i % 2 for i in range(16)]
    out = e.make_and_save_many(clouds, robots=robots, indexs=[5000 + i for i in range(16)])
    assert e.get_size() == 266
    assert np.array_equal(_bits(out), _bits(singles))
    for i in range(16):
        assert np.array_equal(_bits(e.get_signature(250 + i)), _bits(singles[i])), i
        assert e.get_index(250 + i) == (robots[i], 5000 + i)
        assert e.local_to_global(robots[i], 125 + i // 2) == 250 + i
    for r in range(250):
        assert np.array_equal(_bits(e.get_signature(r)), _bits(rows[r])), r
    assert e.get_size(0) == e.get_size(1) == 133


@pytest.mark.gpu
@pytest.mark.parametrize("plugin", PLUGINS)
def test_a_batch_across_the_first_boundary(plugin):
    """250 rows from the wire, then one make_and_save_many of 16 clouds: rows 250 - 265, FloatRows::grow inside the call with the
    kernels writing straight into the new allocation.  The values equal the single-scan make of each cloud, rows 0 - 249 stay."""
    e, rows, clouds, singles = _boundary_engine(plugin)
    _check_batch_landed(e, rows, clouds, singles)
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("plugin", PLUGINS)
def test_a_rejected_batch_at_the_boundary_changes_nothing(plugin):
    """the same call with a NaN in its 12th cloud: it has grown the database and written rows 250 - 265 before the flag is read,
    and must leave 250 keyframes, rows 0 - 249 as they were; a good call after it lands in rows 250 - 265 with its registry
    entries"""
    e, rows, clouds, singles = _boundary_engine(plugin)
    bad = list(clouds)
    bad[11] = clouds[11].copy(); bad[11][7, 1] = np.nan
    with pytest.raises(e.ERROR) as ei:
        e.make_and_save_many(bad, robots=[1] * 16, indexs=list(range(16)))
    assert ei.value.status == -1 and e.get_size() == 250 and e.get_size(1) == 125
    for r in range(250):
        assert np.array_equal(_bits(e.get_signature(r)), _bits(rows[r])), r
    with pytest.raises(e.ERROR):
        e.get_signature(250)
    _check_batch_landed(e, rows, clouds, singles)
    e.close()


# ---- detection over several workgroups -----------------------------------------------------------------------------------------
def _run_detections(e, c, this_id, count, seed, excl, min_queries):
    """detect_intra on `count` local indices and detect_inter on `count` keys (edges, last, a fixed random sample), engine
    against checker; returns how many of each ran"""
    n_mine, n_all = c_size(c, this_id), c_size(c, -1)
    q_intra = _queries(n_mine, excl, count, seed)
    q_inter = _queries(n_all, excl, count, seed + 1)
    loops = 0
    for cur in q_intra:
        loops += _compare(e, c, "intra", cur)[0] >= 0
    for cur in q_inter:
        loops += _compare(e, c, "inter", cur)[0] >= 0
    assert len(q_intra) >= min(min_queries, n_mine) and len(q_inter) >= min(min_queries, n_all)
    return loops


def c_size(c, robot):
    l2g = c.l2g
    return sum(len(x) for x in l2g) if robot < 0 else len(l2g[robot])


@pytest.mark.gpu
@pytest.mark.parametrize("robot_num", [1, 3])
@pytest.mark.parametrize("n", SIZES)
def test_m2dp_detection_over_several_workgroups(n, robot_num):
    """M2DP (192 floats: the float4 branch of nn_l2_kernel), explicit lists.  One robot: n + 5 keys with 5 excluded, so the last
    local index searches exactly n rows and the sample every size below it.  Three robots, this one in the middle, n keys
    arriving interleaved: detect_inter of an own key searches the sorted concatenation of robots 0 and 2 (position != key),
    of a received key this robot's list.  At least 200 queries per mode wherever that many keyframes exist."""
    excl = 5
    kw = dict(robot_num=robot_num, this_id=robot_num // 2, num_exclude_recent=excl, dist_thres=0.3)
    e, c = _engine("m2dp", **kw), _checker("m2dp", **kw)
    _fill(e, c, vector_rows("m2dp", n + (excl if robot_num == 1 else 0), seed=n + robot_num), robot_num)
    assert _run_detections(e, c, kw["this_id"], 220, n, excl, 200) > 0
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("robot_num", [1, 3])
@pytest.mark.parametrize("n", SIZES)
def test_fpfh_detection_over_several_workgroups(n, robot_num):
    """FPFH (33 floats: the DIM % 4 != 0 branch, eight groups of four and one tail element).  inter_mode 0 is the snapshot
    (list == nullptr, rows 0 .. snap_n - 1): it is taken half way through the fill, so the next nine inter detections search the
    stale, smaller set after the database has grown past it, and the tenth takes a new one of n rows (one robot: n + 30 keys).
    inter_mode 1 searches the sorted lists.  report_dims 21 and 33 both ways at n = 2 000, one each below."""
    excl = 30
    configs = [(0, 21), (1, 33)] + ([(0, 33), (1, 21)] if n == 2000 else [])
    rows = vector_rows("fpfh", n + (excl if robot_num == 1 else 0), seed=3 * n + robot_num)
    for mode, rdims in configs:
        kw = dict(robot_num=robot_num, this_id=robot_num // 2, num_exclude_recent=excl, inter_mode=mode, report_dims=rdims, dist_thres=60.0)
        e, c = _engine("fpfh", **kw), _checker("fpfh", **kw)
        half = len(rows) // 2
        _fill(e, c, rows[:half], robot_num)
        _compare(e, c, "inter", half - 1)
        _fill(e, c, rows[half:], robot_num, first=half)
        assert _run_detections(e, c, kw["this_id"], 220, n + mode, excl, 200) > 0
        e.close()


@pytest.mark.gpu
def test_m2dp_at_10000():
    """the headline database size: 10 000 keys of three robots; an own key's inter detection reduces 6 667 candidates over 27
    workgroups, an intra detection up to 3 300; 60 queries each"""
    kw = dict(robot_num=3, this_id=0, num_exclude_recent=30, dist_thres=0.3)
    e, c = _engine("m2dp", **kw), _checker("m2dp", **kw)
    _fill(e, c, vector_rows("m2dp", 10000, seed=10000), 3)
    assert _run_detections(e, c, 0, 60, 10000, 30, 50) > 0
    e.close()


@pytest.mark.gpu
def test_fpfh_at_10000():
    """10 030 keys of one robot: the snapshot holds 10 000 rows (40 workgroups, no list), the last intra detection searches
    10 000; 60 queries each"""
    kw = dict(robot_num=1, this_id=0, num_exclude_recent=30, inter_mode=0, report_dims=21, dist_thres=60.0)
    e, c = _engine("fpfh", **kw), _checker("fpfh", **kw)
    _fill(e, c, vector_rows("fpfh", 10030, seed=10001), 1)
    assert _run_detections(e, c, 0, 60, 10001, 30, 50) > 0
    assert c.snap_n == 10000
    e.close()


# ---- ties ----------------------------------------------------------------------------------------------------------------------
TIE_L = 6 * 256 + 40                     # 1 576 candidates: workgroups 0 .. 5 full, workgroup 6 holds 40
TIE_CASES = [                            # (what, list positions of the planted duplicate, the duplicate is the query's own row)
    ("twice inside one wave", (2 * 256 + 64 + 5, 2 * 256 + 64 + 50), False),
    ("two waves of one workgroup", (256 + 10, 256 + 200), False),
    ("workgroups 0 and 5", (100, 5 * 256 + 7), False),
    ("only the last, partly filled workgroup", (6 * 256 + 3, 6 * 256 + 39), False),
    ("list positions 255 and 256", (255, 256), False),
    ("the query's own row: distance +0, the key's high word 0", (700, 1400), True),
]


def _distinct_rows(plugin, n, rs):
    if plugin == "m2dp":
        return (np.abs(rs.standard_normal((n, 192))) * 0.1).astype(np.float32)
    return (100.0 * rs.dirichlet(np.full(11, 0.7), size=(n, 3))).astype(np.float32).reshape(n, 33)


def _tie_rows(plugin, seed):
    """(candidate rows by list position, one query row per case): every case has a prototype of its own, far from the others"""
    rs = np.random.RandomState(seed)
    cand = _distinct_rows(plugin, TIE_L, rs)
    protos = _distinct_rows(plugin, len(TIE_CASES), rs)
    step = np.float32(0.01 if plugin == "m2dp" else 0.5)
    queries = []
    for (_, positions, own), q in zip(TIE_CASES, protos):
        dup = q if own else (q + step * rs.standard_normal(q.size).astype(np.float32)).astype(np.float32)
        for p in positions:
            cand[p] = dup
        queries.append(q)
    return cand, queries


@pytest.mark.gpu
@pytest.mark.parametrize("plugin,form", [("m2dp", "inter"), ("m2dp", "intra"), ("fpfh", "inter"), ("fpfh", "intra"), ("fpfh", "snapshot")])
def test_ties_go_to_the_lowest_position(plugin, form):
    """exact duplicates planted so that the minimum of nn_l2_kernel is attained twice: in one wave (the shuffle reduction
    decides), in two waves of a workgroup, in workgroups 0 and 5, only in the last partly filled workgroup, at positions 255 / 256
    (the atomicMin decides), and as a copy of the query itself.  Three robots arriving interleaved: in the inter form the sorted
    list of robots 1 and 2 holds key 3 * (p // 2) + 1 + p % 2 at position p, so a kernel that reduced anything but the list
    position would report another key.  The expected key is stated here, not taken from the checker."""
    excl, n_q = 30, len(TIE_CASES)
    cand, queries = _tie_rows(plugin, seed=31)
    rs = np.random.RandomState(32)
    kw = dict(num_exclude_recent=excl, dist_thres=50.0)
    if plugin == "fpfh":
        kw.update(inter_mode=0 if form == "snapshot" else 1, report_dims=33)
    if form == "snapshot":                                     # one robot: keys 0 .. L - 1, then the queries among the 30 newest
        kw.update(robot_num=1, this_id=0)
        seq = [(0, v) for v in cand] + [(0, q) for q in queries] + [(0, v) for v in _distinct_rows(plugin, excl - n_q, rs)]
        ask = [("inter", TIE_L + j) for j in range(n_q)]
        key_at = lambda p: p
    elif form == "inter":                                      # robots 1 and 2 hold the candidates, robot 0 the queries
        kw.update(robot_num=3, this_id=0)
        n = 3 * TIE_L // 2
        filler = iter(_distinct_rows(plugin, n // 3 + 1, rs)); cands = iter(cand); qs = iter(queries)
        seq = [(k % 3, next(cands) if k % 3 else (next(qs) if k // 3 < n_q else next(filler))) for k in range(n)]
        ask = [("inter", 3 * j) for j in range(n_q)]
        key_at = lambda p: 3 * (p // 2) + 1 + p % 2
    else:                                                      # robot 0: the candidates, 30 fillers, then the queries; position = local index
        kw.update(robot_num=3, this_id=0)
        mine = list(cand) + list(_distinct_rows(plugin, excl, rs)) + queries
        other = _distinct_rows(plugin, 2 * len(mine), rs)
        seq = [(k % 3, mine[k // 3] if k % 3 == 0 else other[k - k // 3 - 1]) for k in range(3 * len(mine))]
        ask = [("intra", TIE_L + excl + j) for j in range(n_q)]
        key_at = lambda p: p
    e, c = _engine(plugin, **kw), _checker(plugin, **kw)
    for k, (robot, v) in enumerate(seq):
        e.save_from_wire(v, robot, k); c.save(v, robot, k)
    for (what, positions, own), (which, cur) in zip(TIE_CASES, ask):
        g = _compare(e, c, which, cur)
        assert g[0] == key_at(min(positions)), (what, g)
        assert (float(g[1]) == 0.0) == own and not np.signbit(g[1]), (what, g)
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("plugin", PLUGINS)
def test_every_candidate_the_same_row(plugin):
    """600 candidates (robots 1 and 2) that are all one row: every lane of every wave of three workgroups holds the same distance
    and position 0 (key 1) must win -- for a query elsewhere and for a query that is that row too (every key's high word 0)"""
    rs = np.random.RandomState(41)
    row, other = _distinct_rows(plugin, 2, rs)
    kw = dict(robot_num=3, this_id=0, num_exclude_recent=30, dist_thres=1000.0)
    if plugin == "fpfh":
        kw.update(inter_mode=1, report_dims=33)
    e, c = _engine(plugin, **kw), _checker(plugin, **kw)
    for k in range(900):
        v = row if k % 3 or k == 3 else other
        e.save_from_wire(v, k % 3, k); c.save(v, k % 3, k)
    far, same = _compare(e, c, "inter", 0), _compare(e, c, "inter", 3)
    assert far[0] == 1 and float(far[1]) > 0.0 and same[0] == 1 and float(same[1]) == 0.0
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("plugin", PLUGINS)
def test_the_list_buffer_regrows(plugin):
    """one engine, search sets of 300, then 2 000, then 300 again: nearest_locked allocates d_list for 300 + 150 + 256 entries,
    frees and allocates it again for the 2 000 (nothing copied), and the small set afterwards sits in the larger buffer"""
    kw = dict(robot_num=2, this_id=0, num_exclude_recent=30, dist_thres=0.3 if plugin == "m2dp" else 60.0)
    if plugin == "fpfh":
        kw.update(inter_mode=1)
    e, c = _engine(plugin, **kw), _checker(plugin, **kw)
    rows = vector_rows(plugin, 2300, seed=51)
    for k, v in enumerate(rows):                               # robot 0 (this): 300 keyframes, robot 1: 2 000
        robot = 0 if k % 23 < 3 else 1
        e.save_from_wire(v, robot, k); c.save(v, robot, k)
    assert e.get_size(0) == 300 and e.get_size(1) == 2000
    mine, theirs = c.l2g[0], c.l2g[1]
    for keys in (theirs[5:10], mine[5:10], theirs[1500:1505], mine[200:205]):      # received keys search 300, own keys 2 000
        for key in keys:
            _compare(e, c, "inter", key)
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("plugin", PLUGINS)
def test_non_finite_wire_rows(plugin):
    """save_from_wire does not check its values (include/scl_m2dp.h, scl_fpfh.h).  A NaN squared distance never beats another one
    (nanoflann admits a point only when dist < worst; in nn_l2_kernel a NaN's bit pattern sorts above +inf's), so a NaN row is
    never anybody's neighbour, a row with an infinity is at +inf from every finite row, and the NaN row as the query finds
    nothing: loop -1 and a NaN distance, as the headers say.  600 ordinary rows of two robots, an inf row and a NaN row in each;
    FPFH's non-finite values sit in float 30, past report_dims = 21 and in the tail of the 33."""
    dim = DIMS[plugin]
    at = 30 if plugin == "fpfh" else 77
    kw = dict(robot_num=2, this_id=0, num_exclude_recent=30, dist_thres=0.3 if plugin == "m2dp" else 60.0)
    if plugin == "fpfh":
        kw.update(inter_mode=1, report_dims=21)
    e, c = _engine(plugin, **kw), _checker(plugin, **kw)
    rows = vector_rows(plugin, 604, seed=61)
    special = {100: np.inf, 101: np.nan, 300: np.nan, 301: -np.inf, 602: np.nan, 603: np.nan}      # even keys: robot 0, odd: robot 1
    for k, bad in special.items():
        rows[k] = rows[k - 50]                                 # a copy of an ordinary row (queries near it: the row itself and its twins)
        rows[k, at] = bad
    assert rows.shape[1] == dim
    _fill(e, c, rows, 2)
    for key in range(604):
        _compare(e, c, "inter", key, nan_ok=True)
    for cur in range(302):
        _compare(e, c, "intra", cur, nan_ok=True)
    for form, cur in (("inter", 101), ("inter", 300), ("inter", 602), ("inter", 603), ("intra", 150), ("intra", 301)):
        g = getattr(e, "detect_" + form)(cur)
        assert g[0] == -1 and np.isnan(g[1]), (form, cur, g)
    g = e.detect_inter(51)                                     # the twin of the NaN row 101 of its own robot: searched among robot 0's
    assert not np.isnan(g[1])
    e.close()


# ---- Iris above 256 keyframes ------------------------------------------------------------------------------------------------
def _iris_rowkeys(n, rows, seed):
    return np.random.RandomState(seed).uniform(0.0, 1.0, size=(n, rows)).astype(np.float32)


TIED = (10, 130, 255, 256, 300, 400, 511, 512, 600, 601, 605, 620)     # this robot's local indices that share one row key


def _scan_image(cfg, seed):
    """the image of a real-shaped scan scaled to the configuration's range (no exactly cancelling responses: its templates are
    held to the checker's encode; on drawn images a few imaginary responses cancel exactly and rounding decides their sign, see
    tests/test_iris_fftmatch.py)"""
    return oi.make_image(cfg, synth_scan(20000, seed=seed, max_range=float(cfg.rows) + 5.0))[0]


@pytest.mark.gpu
@pytest.mark.parametrize("shift_search", [0, 1])
def test_iris_700_keyframes_16x72(shift_search):
    """16 x 72, nscale 2 (64 template rows), 700 keyframes from save_image: robot 0 (this one) 640, robots 1 and 2 30 each,
    arriving interleaved.  grow() of iris.hip runs at 256 and 512 with images, row keys, T and M to copy: after keys 256, 257, 512,
    513 and 699 the image, row key and templates of keys 0, 255, 256 and the newest equal the checker's (those keyframes hold
    images of scans), and every other keyframe's templates still equal what the engine gave right after it was stored.  The
    detections run on the engine's own templates, as tests/test_iris_fftmatch.py does for drawn images.  Intra detections and the
    inter detections of received keys rank up to 640 row keys (iris_rowkey_d2_kernel over three workgroups, d_list / d_d2 regrown
    from the 60 an own key searches).  Twelve keyframes share one row key (positions 10 ... 300 ... 600 ... 620): the k-nearest
    selection takes the ten at the lowest positions (equal distance -> ascending position), the ninth of them local 600, whose
    image is the query's turned by 9 columns; the copy at local 605 is the eleventh and must stay out.  Windows (shift_search
    0) and every shift (1)."""
    rows, cols = 16, 72
    kw = dict(rows=rows, cols=cols, nscale=2, num_candidates=10, num_exclude_recent=30, robot_num=3, this_id=0, shift_search=shift_search)
    e, po = _iris_engine(**kw), IrisPluginOracle(oi, ob, **kw)
    robot_of = [0 if k % 70 < 64 else (1 if k % 70 < 67 else 2) for k in range(700)]
    keys = _iris_rowkeys(700, rows, seed=71)
    shared = _iris_rowkeys(1, rows, seed=72)[0]
    probe_img = iris_like(7000, rows, cols)
    scans = (0, 255, 256, 257, 512, 513, 699)                  # global keys that hold the image of a scan
    local = [0, 0, 0]
    probes = []                                                # (global key, local index, robot) of the queries near the shared row key
    stored = []                                                # the engine's templates right after each save
    for k in range(700):
        r = robot_of[k]; key = keys[k]
        img = _scan_image(po.cfg, 7100 + k) if k in scans else iris_like(1000 + k, rows, cols)
        if k not in scans and r == 0 and local[0] in TIED:
            key = shared
            if local[0] in (600, 605):
                img = np.roll(probe_img, 9, axis=1)
        if k not in scans and ((r == 0 and local[0] in (636, 639)) or (r == 1 and local[1] == 29)):
            key = (shared + np.float32(0.05)).astype(np.float32); img = probe_img
            probes.append((k, local[r], r))
        e.save_image(img, key, r, 3 * k); po.save(img, key, r, 3 * k)
        T_g, M_g = e.get_feature(k)
        if k in scans:
            assert np.array_equal(T_g, po.features[r][-1][1]) and np.array_equal(M_g, po.features[r][-1][2]), k
        po.features[r][-1] = (po.features[r][-1][0], T_g, M_g)
        stored.append((T_g, M_g))
        local[r] += 1
        if k in (256, 257, 512, 513, 699):
            for g in sorted({0, 255, 256, k} | set(range(3, k, 37))):
                rr, _ = po.get_index(g); ll = po.local2global[rr].index(g)
                img_g, key_g = e.get_image(g); T_g, M_g = e.get_feature(g)
                assert np.array_equal(img_g, po.features[rr][ll][0]) and np.array_equal(_bits(key_g), _bits(po.rowkeys[rr][ll])), (k, g)
                assert np.array_equal(T_g, stored[g][0]) and np.array_equal(M_g, stored[g][1]), (k, g)
                if g in scans:
                    T_o, M_o = oi.encode(po.cfg, po.features[rr][ll][0])
                    assert np.array_equal(T_g, T_o) and np.array_equal(M_g, M_o), (k, g)
    assert local == [640, 30, 30] and len(probes) == 3 and e.get_size() == 700 and e.get_size(0) == 640
    rs = np.random.RandomState(73)
    own = po.local2global[0]
    g = e.detect_inter(own[100])                               # an own key first: 60 candidates; the 640 below regrow the list
    assert same_iris_detection(g, po.detect_inter(own[100]))
    q_intra = sorted({41, 42, 286, 287, 288, 542, 543, 639, 636} | set(int(x) for x in rs.randint(41, 640, size=60)))
    for cur in q_intra:
        g, o = e.detect_intra(cur), po.detect_intra(cur)
        assert same_iris_detection(g, o), (cur, g, o)
    q_inter = sorted(set(po.local2global[1]) | set(po.local2global[2]) | set(own[int(x)] for x in rs.randint(0, 640, size=20)))
    assert len(q_intra) >= 60 and len(q_inter) >= 60
    for key in q_inter:
        g, o = e.detect_inter(key), po.detect_inter(key)
        assert same_iris_detection(g, o), (key, g, o)
    for key, loc, r in probes:                                 # the tie rule decides: local 600 is found, its copy at 605 never
        g = e.detect_intra(loc) if r == 0 else e.detect_inter(key)
        # (a turned copy's templates are the original's turned, up to the sign of a response that rounding decides: a few bits of 4 608)
        assert g[0] == (600 if r == 0 else own[600]) and g[2] < 0.02, (key, loc, r, g)
    e.close()


class _EngineFeatures:
    """a robot's feature list for the checker whose templates are the engine's own, fetched when first asked for (a detection
    touches a handful of the 300; the checker's encode at 80 x 360 is ~40 M multiply-adds per image)"""

    def __init__(self, eng, images, n=None, cache=None):
        self.eng, self.images, self.n, self.cache = eng, images, n, {} if cache is None else cache

    def __len__(self):
        return len(self.images) if self.n is None else self.n

    def __getitem__(self, i):
        if isinstance(i, slice):
            start, stop, step = i.indices(len(self))
            assert start == 0 and step == 1
            return _EngineFeatures(self.eng, self.images, stop, self.cache)
        i = int(i)
        if i not in self.cache:
            self.cache[i] = (self.images[i],) + tuple(self.eng.get_feature(i))
        return self.cache[i]


@pytest.mark.gpu
def test_iris_300_keyframes_80x360_and_the_work_buffers_regrow():
    """the default geometry past its first capacity: 300 keyframes of one robot (grow() copies 256 images of 28 800 bytes and
    2 x 256 x 7 200 template words; keys 0, 255, 256 and 298 hold images of scans and their templates equal the checker's after
    it), four intra detections with num_candidates 3 on the engine's own templates, then on the same engine compare() with 3 and
    with 40 candidates (fm_cap: the FFT work buffers; job_cap: 40 x 5 Hamming jobs; rolls_cap) and hamming_all_shifts with 2 and
    with 30 (job_cap again: 30 x 360 jobs).  Five candidates of each large call equal the checker, and the small calls repeated
    after the large ones give the bits they gave before."""
    kw = dict(num_candidates=3, num_exclude_recent=30)
    e, po = _iris_engine(**kw), IrisPluginOracle(oi, ob, **kw)
    keys = _iris_rowkeys(300, 80, seed=81)
    scans = (0, 255, 256, 298)
    imgs = [_scan_image(po.cfg, 8100 + k) if k in scans else iris_like(2000 + k) for k in range(300)]
    imgs[290] = np.roll(imgs[200], 33, axis=1); keys[290] = keys[200] + np.float32(0.02)      # turned revisits of keyframes the doubling copied
    imgs[299] = np.roll(imgs[12], -50, axis=1); keys[299] = keys[12] + np.float32(0.02)
    for k in range(300):
        e.save_image(imgs[k], keys[k], 0, k)
        po.rowkeys[0].append(keys[k]); po.local2global[0].append(k); po.indexs.append((0, k))
    po.features[0] = _EngineFeatures(e, imgs)
    for g in scans + (299,):
        img_g, key_g = e.get_image(g)
        assert np.array_equal(img_g, imgs[g]) and np.array_equal(_bits(key_g), _bits(keys[g])), g
        if g in scans:
            T_g, M_g = e.get_feature(g); T_o, M_o = oi.encode(po.cfg, imgs[g])
            assert np.array_equal(T_g, T_o) and np.array_equal(M_g, M_o), g
    found = {}
    for cur in (299, 290, 280, 257):
        g, o = e.detect_intra(cur), po.detect_intra(cur)
        assert same_iris_detection(g, o), (cur, g, o)
        found[cur] = g[0]
    assert found[299] == 12 and found[290] == 200
    feat = lambda k: po.features[0][k]
    small = [12, 100, 256]
    large = list(range(0, 280, 7))
    assert len(large) == 40
    d3, b3 = e.compare(299, small)
    d40, b40 = e.compare(299, large)
    for i in (0, 7, 19, 37, 39):
        k2 = large[i]
        d_o, b_o, _ = oi.compare(po.cfg, 2, imgs[299], feat(299)[1], feat(299)[2], imgs[k2], feat(k2)[1], feat(k2)[2])
        assert b40[i] == b_o and same_f32(d40[i], d_o, nan_ok=True), (k2, d40[i], d_o, b40[i], b_o)
    d3b, b3b = e.compare(299, small)
    assert np.array_equal(_bits(d3), _bits(d3b)) and np.array_equal(b3, b3b) and d3[0] < 0.02
    a2 = e.hamming_all_shifts(290, [200, 5])
    d30, b30 = e.hamming_all_shifts(290, list(range(255, 285)))
    for i in (0, 1, 15, 22, 29):
        k2 = 255 + i
        d_o, b_o = oi.hamming_all(po.cfg, feat(290)[1], feat(290)[2], feat(k2)[1], feat(k2)[2])
        assert b30[i] == b_o and same_f32(d30[i], d_o, nan_ok=True), (k2, d30[i], d_o)
    a2b = e.hamming_all_shifts(290, [200, 5])
    assert np.array_equal(_bits(a2[0]), _bits(a2b[0])) and np.array_equal(a2[1], a2b[1]) and a2[0][0] < 0.02
    e.close()
