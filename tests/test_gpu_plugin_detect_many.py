"""The batch calls of the M2DP, FPFH and GRSD plugins (detect_intra_many, detect_inter_many, save_from_wire_many,
make_save_and_detect; nn_l2_many_kernel and nearest_many_locked in scl_slam_amd/csrc/plugin_host.hpp).  The defining property: a
batched call returns, element by element and bit for bit, what the same single calls made in array order return, and leaves the
handle in the same state.  So two handles get the same rows; handle A answers with the batch calls, handle B with single calls in
the same order, and up to 2 000 keys the CPU checkers (tests/plugin_cases.py, tests/plugin_batch_cases.py) answer too.  Loop ids
equal, float distances equal by their uint32 pattern; two NaNs of any payload count as equal only where a row holds a NaN."""
import numpy as np
import pytest

from plugin_batch_cases import FpfhChecker, GrsdChecker, M2dpChecker, plugin_rows, same_detection
from scl_slam_amd.synth import synth_scan

PLUGINS = ("m2dp", "fpfh", "grsd")
BATCHES = (1, 15, 16, 17, 100, 1000)
OUT_OF_RANGE = -4
M2DP_KEYS = ("dist_thres", "num_exclude_recent", "robot_num", "this_id")


def _kw(plugin, kw):
    if plugin == "m2dp":
        return {k: v for k, v in kw.items() if k in M2DP_KEYS}
    if plugin == "grsd":
        return {k: v for k, v in kw.items() if k != "report_dims"}
    return dict(kw)


def _engine(plugin, **kw):
    import scl_slam_amd
    cls = {"m2dp": scl_slam_amd.M2dpEngine, "fpfh": scl_slam_amd.FpfhEngine, "grsd": scl_slam_amd.GrsdEngine}[plugin]
    return cls(**_kw(plugin, kw))


def _checker(plugin, **kw):
    kw = _kw(plugin, kw)
    return M2dpChecker(vectorised=True, **kw) if plugin == "m2dp" else (FpfhChecker(**kw) if plugin == "fpfh" else GrsdChecker(**kw))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _fill(handles, rows, robot_num, first=0):
    """rows from the wire one by one, robot = key % robot_num (interleaved arrival), index = 7 * key"""
    for i, v in enumerate(rows):
        k = first + i
        for h in handles:
            if hasattr(h, "save_from_wire"):
                h.save_from_wire(v, k % robot_num, 7 * k)
            else:
                h.save(v, k % robot_num, 7 * k)


def _orders(n_avail, size, seed):
    """`size` queries of [0, n_avail): ascending, descending, and a few values repeated"""
    rs = np.random.RandomState(seed)
    asc = np.sort(rs.randint(0, n_avail, size=size))
    asc[-1] = n_avail - 1                                                       # the newest keyframe is always asked
    few = rs.randint(0, n_avail, size=min(3, size))
    return {"ascending": asc, "descending": asc[::-1].copy(), "repeated": few[rs.randint(0, few.size, size=size)]}


def _same_batch(form, a, others, curs, nan_ok=False):
    """handle a's batch call against single calls on every one of `others` in array order; returns a's answers"""
    loops, dists = getattr(a, f"detect_{form}_many")(curs)
    assert loops.dtype == np.int32 and dists.dtype == np.float32 and loops.size == dists.size == len(curs)
    for o in others:
        for i, cur in enumerate(curs):
            want = getattr(o, f"detect_{form}")(int(cur))
            assert same_detection((loops[i], dists[i]), want, nan_ok), (form, type(o).__name__, i, int(cur), (loops[i], dists[i]), want)
    return loops, dists


# ---- batched against single calls and against the CPU checkers ------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("robots", ((1, 0), (3, 0), (3, 1)), ids=("one_robot", "three_robots_id0", "three_robots_id1"))
@pytest.mark.parametrize("n", (31, 256, 257, 2000, 10000))
@pytest.mark.parametrize("plugin", PLUGINS)
def test_batches_equal_single_calls(plugin, n, robots):
    """batch sizes 1, 15, 16, 17, 100 and 1 000, queries ascending, descending and repeated, intra and inter (FPFH and GRSD in the
    reference's inter mode: the counter and the snapshot walk through every batch): handle A's batch answers equal handle B's
    single calls and, up to 2 000 keys, the CPU checker's"""
    robot_num, this_id = robots
    kw = dict(num_exclude_recent=10, robot_num=robot_num, this_id=this_id, tree_making_period=7)
    rows = plugin_rows(plugin, n, seed=1000 + n)
    a, b = _engine(plugin, **kw), _engine(plugin, **kw)
    others = [b] + ([_checker(plugin, **kw)] if n <= 2000 else [])
    try:
        _fill([a] + others, rows, robot_num)
        mine = a.get_size(this_id)
        found = 0
        for size in BATCHES:
            for form, n_avail in (("intra", mine), ("inter", n)):
                for name, curs in _orders(n_avail, size, seed=size + n).items():
                    loops, _ = _same_batch(form, a, others, curs)
                    found += int((loops >= 0).sum())
        assert found > 0 or n < 256, "the drawn rows hold loops"
        for cur in (0, n - 1):                                                  # the handles' states are equal afterwards
            assert same_detection(a.detect_inter(cur), b.detect_inter(cur)), cur
    finally:
        a.close(); b.close()


# ---- the reference's inter mode: counter and snapshot ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("period", (1, 3, 10))
@pytest.mark.parametrize("plugin", ("fpfh", "grsd"))
def test_reference_inter_mode_state(plugin, period):
    """inter_mode = 0: batches interleaved with appends and with single calls on both handles.  A batch below num_exclude_recent + 1
    keyframes answers (-1, 0) and leaves the counter alone; afterwards a single call on A and on B answers the same"""
    kw = dict(num_exclude_recent=5, tree_making_period=period, inter_mode=0, robot_num=2, this_id=0)
    rows = plugin_rows(plugin, 400, seed=77)
    a, b, c = _engine(plugin, **kw), _engine(plugin, **kw), _checker(plugin, **kw)
    try:
        _fill([a, b, c], rows[:4], 2)
        loops, dists = _same_batch("inter", a, [b, c], np.array([0, 3, 1, 2, 0]))
        assert (loops == -1).all() and (_bits(dists) == 0).all()
        at = 4
        for upto, size, seed in ((6, 4, 1), (40, 7, 2), (41, 17, 3), (140, 100, 4), (141, 1, 5), (400, 33, 6)):
            _fill([a, b, c], rows[at:upto], 2, first=at)
            at = upto
            rs = np.random.RandomState(seed)
            _same_batch("inter", a, [b, c], rs.randint(0, at, size=size))
            for cur in rs.randint(0, at, size=2):                               # single calls on every handle in between
                g = a.detect_inter(int(cur))
                assert same_detection(g, b.detect_inter(int(cur))) and same_detection(g, c.detect_inter(int(cur)))
        for cur in range(0, 400, 37):                                           # more than one period of further single calls
            assert same_detection(a.detect_inter(cur), b.detect_inter(cur)), cur
    finally:
        a.close(); b.close()


# ---- M2DP's inter rule: two lists -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("plugin", PLUGINS)
def test_inter_batches_over_both_lists(plugin):
    """inter_mode = 1 (M2DP's only rule): batches that mix keys of this robot (they search the other robots' keys) with received
    ones (they search this robot's), three robots, this_id 1; and a handle that holds no other robot's keyframes: (-1, +inf)"""
    kw = dict(num_exclude_recent=10, inter_mode=1, robot_num=3, this_id=1)
    rows = plugin_rows(plugin, 700, seed=31)
    a, b, c = _engine(plugin, **kw), _engine(plugin, **kw), _checker(plugin, **kw)
    try:
        _fill([a, b, c], rows, 3)
        rs = np.random.RandomState(32)
        for size in (2, 16, 17, 50, 333):
            curs = rs.randint(0, 700, size=size)
            assert len({int(k) % 3 == 1 for k in curs}) == 2 or size == 2        # both lists in one batch
            _same_batch("inter", a, [b, c], curs)
        _same_batch("inter", a, [b, c], np.array([1, 4, 7]))                     # this robot's keys only
        _same_batch("inter", a, [b, c], np.array([0, 2, 699]))                   # received keys only
    finally:
        a.close(); b.close()
    alone, twin = _engine(plugin, **kw), _engine(plugin, **kw)
    try:
        for k in range(40):
            alone.save_from_wire(rows[k], 1, k); twin.save_from_wire(rows[k], 1, k)
        loops, dists = _same_batch("inter", alone, [twin], np.arange(40))
        assert (loops == -1).all() and np.isposinf(dists).all()
    finally:
        alone.close(); twin.close()


# ---- edge rules -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("plugin", PLUGINS)
def test_edge_rules(plugin):
    """cur < num_exclude_recent answers (-1, +inf) inside a batch that also holds searching queries; equal rows in different tiles
    of 64 candidates (each its own workgroup): the lowest key wins; num_exclude_recent = 0"""
    kw = dict(num_exclude_recent=12, inter_mode=1, robot_num=1, this_id=0)
    rows = plugin_rows(plugin, 1000, seed=41)
    rows[1:] += np.float32(1.0) * (rows[1:] == rows[0])                           # no drawn copy of row 0 is left
    for k in (5, 70, 700, 900):
        rows[k] = rows[0] + np.float32(0.5)
    rows[0] += np.float32(2.0)
    a, b, c = _engine(plugin, **kw), _engine(plugin, **kw), _checker(plugin, **kw)
    try:
        _fill([a, b, c], rows, 1)
        curs = np.array([0, 11, 12, 13, 500, 3, 900, 999, 12])
        loops, dists = _same_batch("intra", a, [b, c], curs)
        for i in (0, 1, 2, 5, 8):
            assert loops[i] == -1 and np.isposinf(dists[i]), i
        assert loops[6] == 5 and dists[6] == 0.0                                  # copies at 5, 70 and 700: three workgroups
    finally:
        a.close(); b.close()
    kw["num_exclude_recent"] = 0
    a, b, c = _engine(plugin, **kw), _engine(plugin, **kw), _checker(plugin, **kw)
    try:
        _fill([a, b, c], rows[:200], 1)
        loops, dists = _same_batch("intra", a, [b, c], np.arange(200))
        assert loops[0] == -1 and np.isposinf(dists[0]) and np.isfinite(dists[1:]).all()
    finally:
        a.close(); b.close()


# ---- non-finite rows ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("plugin, report_dims", (("m2dp", None), ("fpfh", 21), ("fpfh", 33), ("grsd", None)))
def test_non_finite_rows(plugin, report_dims):
    """a NaN candidate row never wins; a NaN query row answers (-1, NaN) (FPFH with report_dims 21 and 33: one NaN sits beyond the
    21st float); an inf row behaves as in the single calls"""
    kw = dict(num_exclude_recent=3, inter_mode=1, robot_num=2, this_id=0)
    if report_dims:
        kw["report_dims"] = report_dims
    rows = plugin_rows(plugin, 300, seed=51)
    dim = rows.shape[1]
    rows[20, dim - 1] = np.nan; rows[21, 0] = np.nan; rows[150, 2] = np.nan       # keys 20 and 150: this robot's, 21: received
    rows[40, 1] = np.inf; rows[41, dim - 2] = -np.inf
    rows[200] = rows[20]; rows[201] = rows[21]
    a, b, c = _engine(plugin, **kw), _engine(plugin, **kw), _checker(plugin, **kw)
    try:
        _fill([a, b, c], rows, 2)
        for form, curs in (("intra", np.arange(150)), ("inter", np.arange(300))):
            loops, dists = _same_batch(form, a, [b, c], curs, nan_ok=True)
            nan_rows = (10, 75, 100) if form == "intra" else (20, 21, 150, 200, 201)
            for i in range(len(curs)):
                if i in nan_rows:
                    assert loops[i] == -1 and np.isnan(dists[i]), (form, i)
                else:
                    assert not np.isnan(dists[i]), (form, i)
                    assert loops[i] not in nan_rows, (form, i)
    finally:
        a.close(); b.close()


# ---- errors ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("plugin", PLUGINS)
def test_errors_change_nothing(plugin):
    """one out-of-range cur in the middle of a batch: SCL_ERR_OUT_OF_RANGE, the outputs keep their sentinels, and a following single
    detect_inter answers as on a handle that never saw the batch (the reference's inter mode: its counter is where it was);
    count = 0 is fine; dists = NULL is accepted"""
    kw = dict(num_exclude_recent=5, tree_making_period=2, inter_mode=0, robot_num=2, this_id=0)
    rows = plugin_rows(plugin, 120, seed=61)
    a, b = _engine(plugin, **kw), _engine(plugin, **kw)
    try:
        _fill([a, b], rows, 2)
        assert same_detection(a.detect_inter(7), b.detect_inter(7))              # the counter is odd now: no rebuild at the next call
        _fill([a, b], rows[:9], 2, first=120)
        for form, bad in (("inter", 129), ("inter", -1), ("intra", a.get_size(0)), ("intra", -3)):
            curs = np.array([1, 2, 3, bad, 4, 5] * 4)
            loops, dists = np.full(curs.size, -7, np.int32), np.full(curs.size, 123.0, np.float32)
            with pytest.raises(type(a).ERROR) as err:
                getattr(a, f"detect_{form}_many")(curs, loops=loops, dists=dists)
            assert err.value.status == OUT_OF_RANGE
            assert (loops == -7).all() and (dists == 123.0).all()
        for cur in (128, 0, 64):
            assert same_detection(a.detect_inter(cur), b.detect_inter(cur)), cur
        for form in ("intra", "inter"):
            loops, dists = getattr(a, f"detect_{form}_many")(np.zeros(0, np.int32))
            assert loops.size == 0 and dists.size == 0
        curs = np.arange(0, 60)
        loops, none = a.detect_intra_many(curs, want_dists=False)
        assert none is None
        assert [int(x) for x in loops] == [b.detect_intra(int(cur))[0] for cur in curs]
        loops, none = a.detect_inter_many(curs, want_dists=False)
        assert none is None
        assert [int(x) for x in loops] == [b.detect_inter(int(cur))[0] for cur in curs]
    finally:
        a.close(); b.close()


# ---- save_from_wire_many --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("plugin", PLUGINS)
def test_save_from_wire_many(plugin):
    """255 rows, then 300 rows (across the capacity doublings at 256 and 512): every row, the registry and all detections equal
    the handle fed one by one; a bad robot id anywhere stores nothing"""
    kw = dict(num_exclude_recent=10, inter_mode=1, robot_num=3, this_id=2)
    rows = plugin_rows(plugin, 555, seed=71)
    robots, indexs = np.arange(555) % 3, 7 * np.arange(555)
    a, b = _engine(plugin, **kw), _engine(plugin, **kw)
    try:
        _fill([b], rows, 3)
        a.save_from_wire_many(rows[:0], robots[:0], indexs[:0])
        assert a.get_size() == 0
        a.save_from_wire_many(rows[:255], robots[:255], indexs[:255])
        assert a.get_size() == 255
        wrong = robots[255:].copy(); wrong[150] = 3
        with pytest.raises(type(a).ERROR):
            a.save_from_wire_many(rows[255:], wrong, indexs[255:])
        assert a.get_size() == 255 and [a.get_size(r) for r in range(3)] == [85, 85, 85]
        a.save_from_wire_many(rows[255:], robots[255:], indexs[255:])
        assert a.get_size() == 555
        for k in range(555):
            assert np.array_equal(_bits(a.get_signature(k)), _bits(rows[k])), k
            assert a.get_index(k) == b.get_index(k) == (k % 3, 7 * k)
            assert a.local_to_global(k % 3, k // 3) == k
        _same_batch("intra", a, [b], np.arange(a.get_size(2)))
        _same_batch("inter", a, [b], np.arange(555))
        for cur in range(0, 555, 11):
            assert same_detection(a.detect_inter(cur), b.detect_inter(cur)), cur
    finally:
        a.close(); b.close()


# ---- make_save_and_detect -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("plugin", PLUGINS)
def test_make_save_and_detect(plugin):
    """40 synthetic keyframes in calls of 1, 16 and 23 clouds, num_exclude_recent = 5, every fifth of another robot: the values, the
    database and the detections equal make_and_save_many plus single detect_intra calls on the twin handle; another robot's entries
    answer (-1, +inf); a call holding a cloud with a NaN coordinate stores nothing and leaves the outputs untouched"""
    kw = dict(num_exclude_recent=5, robot_num=2, this_id=0, dist_thres=1.0e9)
    clouds = [synth_scan(1500 + 40 * (i % 9), seed=300 + i % 9) for i in range(40)]      # every scene comes back: loops
    robots = [1 if i % 5 == 4 else 0 for i in range(40)]
    a, b = _engine(plugin, **kw), _engine(plugin, **kw)
    try:
        at = 0
        for size in (1, 16, 23):
            sl = slice(at, at + size)
            if size == 23:
                spoiled = [c.copy() for c in clouds[sl]]
                spoiled[11][7, 1] = np.nan
                loops, dists = np.full(size, -7, np.int32), np.full(size, 123.0, np.float32)
                with pytest.raises(type(a).ERROR):
                    a.make_save_and_detect(spoiled, robots[sl], list(range(at, at + size)), loops=loops, dists=dists)
                assert a.get_size() == at and (loops == -7).all() and (dists == 123.0).all()
            loops, dists, values = a.make_save_and_detect(clouds[sl], robots[sl], list(range(at, at + size)))
            want = b.make_and_save_many(clouds[sl], robots[sl], list(range(at, at + size)))
            assert np.array_equal(_bits(values), _bits(want))
            local = b.get_size(0) - sum(1 for r in robots[sl] if r == 0)
            for i in range(size):
                if robots[at + i] == 0:
                    assert same_detection((loops[i], dists[i]), b.detect_intra(local)), (at + i, local)
                    local += 1
                else:
                    assert loops[i] == -1 and np.isposinf(dists[i]), at + i
            at += size
        assert a.get_size() == b.get_size() == 40
        for k in range(40):
            assert np.array_equal(_bits(a.get_signature(k)), _bits(b.get_signature(k))) and a.get_index(k) == b.get_index(k), k
        loops, _ = _same_batch("intra", a, [b], np.arange(a.get_size(0)))
        assert (loops >= 0).any(), "the returning scenes are found"
    finally:
        a.close(); b.close()


# ---- regrown work buffers -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("plugin", PLUGINS)
def test_work_buffers_regrow(plugin):
    """a batch of 16, then 1 000 (the query buffers grow), then 16 again on one handle, the database growing in between (the list
    buffer grows)"""
    kw = dict(num_exclude_recent=10, inter_mode=1, robot_num=2, this_id=0)
    rows = plugin_rows(plugin, 3000, seed=81)
    a, b = _engine(plugin, **kw), _engine(plugin, **kw)
    try:
        _fill([a, b], rows[:300], 2)
        rs = np.random.RandomState(82)
        _same_batch("intra", a, [b], rs.randint(0, 150, size=16))
        _fill([a, b], rows[300:], 2, first=300)
        for size in (1000, 16):
            _same_batch("intra", a, [b], rs.randint(0, 1500, size=size))
            _same_batch("inter", a, [b], rs.randint(0, 3000, size=size))
    finally:
        a.close(); b.close()
