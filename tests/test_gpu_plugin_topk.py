"""The candidate lists of the M2DP, FPFH and GRSD plugins (detect_intra_topk, detect_inter_topk; nn_l2_topk_kernel,
nn_topk_merge_kernel and nearest_topk_many_locked in scl_slam_amd/csrc/plugin_host.hpp) against the checker top-k and the handle
model of tests/plugin_topk_cases.py: ids and n_found equal, the reported distances equal by their uint32 pattern; entry 0 against the
_many form on a twin handle, which also shows that the handles' states stay equal.  Rows arrive through save_from_wire_many."""
import json
import os
from ctypes import POINTER, c_float, c_int

import numpy as np
import pytest

from golden.gen_plugin_topk_golden import CASES, K, golden_keys, golden_queries
from plugin_cases import same_detection
from plugin_topk_cases import DIMS, TopkModel, plugin_rows, same_lists

ROOT = os.path.dirname(os.path.abspath(__file__))
# every plugin, FPFH and GRSD in both inter modes (M2DP has the lists only)
VARIANTS = (("m2dp", 1), ("fpfh", 0), ("fpfh", 1), ("grsd", 0), ("grsd", 1))
IDS = tuple(f"{p}_mode{m}" for p, m in VARIANTS)
KS = (1, 2, 10, 32)
INVALID_ARG, OUT_OF_RANGE = -1, -4


def _engine(plugin, **kw):
    import scl_slam_amd
    cls = {"m2dp": scl_slam_amd.M2dpEngine, "fpfh": scl_slam_amd.FpfhEngine, "grsd": scl_slam_amd.GrsdEngine}[plugin]
    if plugin == "m2dp":
        kw = {k: v for k, v in kw.items() if k in ("dist_thres", "num_exclude_recent", "robot_num", "this_id")}
    elif plugin == "grsd":
        kw = {k: v for k, v in kw.items() if k != "report_dims"}
    return cls(**kw)


def _model(plugin, **kw):
    kw.pop("dist_thres", None)
    return TopkModel(plugin, **kw)


def _fill(handles, model, rows, robots):
    for h in handles:
        h.save_from_wire_many(rows, robots, 7 * np.arange(len(rows)))
    model.save_many(rows, robots)


def _same_as_model(form, a, model, curs, k):
    got = getattr(a, f"detect_{form}_topk")(curs, k)
    assert got[0].shape == got[1].shape == (len(curs), k) and got[0].dtype == np.int32 and got[1].dtype == np.float32
    want = model.topk(form, curs, k)
    assert same_lists(got, want), (form, k, list(curs), got[0][:3], want[0][:3], got[2], want[2])
    return got


def _entry0_is_the_many_form(form, got, twin, curs):
    """the twin handle's _many form (dist_thres far above every distance: a found nearest is a loop): entry 0's id and distance bits"""
    loops, dists = getattr(twin, f"detect_{form}_many")(curs)
    ids, cd, found = got
    for i in range(len(curs)):
        if found[i] > 0:
            assert same_detection((ids[i, 0], cd[i, 0]), (loops[i], dists[i])), (form, i, int(curs[i]))
        else:
            assert loops[i] == -1 and ids[i, 0] == -1 and np.isposinf(cd[i, 0]), (form, i)


# ---- search-set sizes -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("plugin, mode", VARIANTS, ids=IDS)
def test_search_set_sizes(plugin, mode):
    """the handle grows so that the inter search set (the snapshot n - num_exclude_recent for mode 0, this robot's keys for a received
    query in mode 1) is 0, 1, k - 1, k, k + 1, 63, 64, 65, 129 and 1 000 keys for k = 1, 2, 10 and 32, and the intra sets lie
    around them; three queries per call, so the prefixes of one launch group differ"""
    kw = dict(num_exclude_recent=2, tree_making_period=2, inter_mode=mode, robot_num=2, this_id=0, dist_thres=1.0e9)
    sizes = sorted({s for k in KS for s in (0, 1, k - 1, k, k + 1, 63, 64, 65, 129, 1000)})
    rows = plugin_rows(plugin, 1002, seed=11)
    a, b, m = _engine(plugin, **kw), _engine(plugin, **kw), _model(plugin, **kw)
    try:
        _fill([a, b], m, rows[:2], [1, 1])                                       # keys 0 and 1: received, they query this robot's
        at = 2
        for size in sizes:
            _fill([a, b], m, rows[at:size + 2], np.zeros(size + 2 - at, np.int8))
            at = size + 2
            assert a.get_size(0) == size
            for k in KS:
                curs = np.array([0, 1, at - 1])
                got = _same_as_model("inter", a, m, curs, k)
                assert mode == 0 or (got[2][:2] == min(k, size)).all()
                _entry0_is_the_many_form("inter", got, b, curs)
                if size:
                    curs = np.array([size - 1, size // 2, 0, min(size - 1, k + 2)])
                    got = _same_as_model("intra", a, m, curs, k)
                    assert got[2][0] == min(k, max(0, size - 3)) and got[2][2] == 0
                    _entry0_is_the_many_form("intra", got, b, curs)
        for cur in (0, 1, 500):                                                  # the handles' states are equal afterwards
            assert same_detection(a.detect_inter(cur), b.detect_inter(cur)), cur
    finally:
        a.close(); b.close()


# ---- counts, prefixes inside one group, mixed call sequences --------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("plugin, mode", VARIANTS, ids=IDS)
def test_counts_and_mixed_sequences(plugin, mode):
    """1, 16, 17 and 33 queries per call (one launch group, a full one, two and three), drawn over 500 keys of three robots so that
    every group holds different prefixes and, in mode 1, both lists; candidate-list calls on handle A interleaved with appends and
    single calls, the _many form with the same curs on the twin: the lists equal the model's, entry 0 equals the twin's answer, and
    at the end both handles answer single calls alike (the counter and the snapshot of mode 0 walked the same way)"""
    kw = dict(num_exclude_recent=7, tree_making_period=3, inter_mode=mode, robot_num=3, this_id=1, dist_thres=1.0e9)
    rows = plugin_rows(plugin, 500, seed=21)
    robots = np.arange(500) % 3
    a, b, m = _engine(plugin, **kw), _engine(plugin, **kw), _model(plugin, **kw)
    try:
        at = 0
        rs = np.random.RandomState(22)
        for upto, count, k in ((5, 1, 10), (90, 16, 1), (200, 17, 10), (201, 33, 32), (500, 33, 2), (500, 17, 32), (500, 16, 10)):
            _fill([a, b], m, rows[at:upto], robots[at:upto])
            at = upto
            curs = rs.randint(0, at, size=count)
            _entry0_is_the_many_form("inter", _same_as_model("inter", a, m, curs, k), b, curs)
            curs = rs.randint(0, a.get_size(1), size=count)
            _entry0_is_the_many_form("intra", _same_as_model("intra", a, m, curs, k), b, curs)
            cur = int(rs.randint(0, at))                                         # a single call on both in between
            assert same_detection(a.detect_inter(cur), b.detect_inter(cur)), cur
            m.sets("inter", [cur])
        for cur in range(0, 500, 61):
            assert same_detection(a.detect_inter(cur), b.detect_inter(cur)), cur
    finally:
        a.close(); b.close()


# ---- ties -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("plugin", ("m2dp", "fpfh", "grsd"))
def test_ties_across_tiles(plugin):
    """the drawn rows hold exact copies (10 to 15 %), so equal sums sit in different tiles of 64 candidates; and planted copies of the
    query row at 5, 70, 130 and 200 -- four tiles -- lead the list in that order at distance 0: the lowest position comes first"""
    kw = dict(num_exclude_recent=0, inter_mode=1, robot_num=1, this_id=0)
    rows = plugin_rows(plugin, 300, seed=31)
    for p in (5, 70, 130, 200, 299):
        rows[p] = rows[150] + np.float32(0.25)
    a, m = _engine(plugin, **kw), _model(plugin, **kw)
    try:
        _fill([a], m, rows, np.zeros(300, np.int8))
        for k in (2, 10, 32):
            ids, dists, found = _same_as_model("intra", a, m, np.array([299, 298, 64, 65, 129]), k)
            assert list(ids[0, :4]) == [5, 70, 130, 200][:k] and (dists[0, :min(k, 4)] == 0.0).all()
    finally:
        a.close()


# ---- non-finite rows ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("plugin, report_dims", (("m2dp", None), ("fpfh", 21), ("fpfh", 33), ("grsd", None)))
def test_non_finite_rows(plugin, report_dims):
    """NaN rows are never listed (a set of 12 with two of them: n_found = 10 of k = 32), +inf rows are candidates and come last (a
    set of 22 with two NaN and two inf rows: n_found = 20, the inf rows at 18 and 19), a NaN query row finds nothing (FPFH: one NaN
    sits beyond the 21 reported floats)"""
    kw = dict(num_exclude_recent=3, inter_mode=1, robot_num=2, this_id=0)
    if report_dims:
        kw["report_dims"] = report_dims
    rows = plugin_rows(plugin, 300, seed=51)
    dim = rows.shape[1]
    rows[4, dim - 1] = np.nan; rows[21, 0] = np.nan; rows[16, 2] = np.nan         # keys 4 and 16: this robot's (local 2, 8), 21: received
    rows[40, 1] = np.inf; rows[41, dim - 2] = np.inf; rows[42, 0] = -np.inf
    rows[200] = rows[4]; rows[201] = rows[21]
    a, m = _engine(plugin, **kw), _model(plugin, **kw)
    try:
        _fill([a], m, rows, np.arange(300) % 2)
        for k in (1, 10, 32):
            ids, dists, found = _same_as_model("intra", a, m, np.array([15, 149, 2, 8, 100, 20, 25]), k)
            assert found[0] == min(k, 10) and found[1] == k and found[2] == found[3] == found[4] == 0 and found[6] == min(k, 20)
            if k == 32:
                assert set(ids[6, 18:20]) == {20, 21} and np.isposinf(dists[6, 18:20]).all() and np.isfinite(dists[6, :18]).all()
            assert not np.isin(ids, (2, 8)).any() and not np.isnan(dists).any()
            ids, dists, found = _same_as_model("inter", a, m, np.arange(0, 300, 7), k)
            assert not np.isin(ids, (4, 16, 21, 200, 201)).any()
            ids, dists, found = _same_as_model("inter", a, m, np.array([4, 16, 21, 200, 201]), k)
            assert (found == 0).all() and (ids == -1).all() and np.isposinf(dists).all()
        ids, dists, found = a.detect_inter_topk([1], 32)                           # key 1 (received) searches the 150 keys of this robot
        assert found[0] == 32
    finally:
        a.close()


# ---- scale ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_ten_thousand_m2dp_rows():
    """10 000 rows: 156 tiles of partial lists per query, merged in more than one round at k = 32; 20 queries (two launch groups), the
    last ten keys are another robot's and search all 9 990 of this one"""
    kw = dict(num_exclude_recent=30, robot_num=2, this_id=0)
    rows = plugin_rows("m2dp", 10000, seed=61)
    robots = (np.arange(10000) >= 9990).astype(np.int8)
    a, m = _engine("m2dp", **kw), _model("m2dp", **kw)
    try:
        _fill([a], m, rows, robots)
        rs = np.random.RandomState(62)
        for k in (10, 32):
            _same_as_model("intra", a, m, np.concatenate(([9989, 9988], rs.randint(0, 9990, size=18))), k)
            _same_as_model("inter", a, m, np.concatenate((np.arange(9990, 10000), rs.randint(0, 9990, size=10))), k)
    finally:
        a.close()


# ---- the reference's order ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_lists_are_in_nanoflann_order():
    """tests/golden/plugin_topk_golden.json (the reference's own nanoflann, k = 10, queries with ties left out): the keys and then the
    queries from the wire as another robot's keyframes, each query's inter list -- this robot's keys -- is nanoflann's, and the reported
    distance is sqrtf of its squared distance over the reported floats (all of them for M2DP and GRSD, FPFH with report_dims = 33)"""
    gold = json.load(open(os.path.join(ROOT, "golden", "plugin_topk_golden.json")))
    plugin_of = {192: "m2dp", 33: "fpfh", 21: "grsd"}
    for name, dim, N, seed, nq in CASES:
        keys = golden_keys(dim, N, seed)
        queries = golden_queries(keys, seed, nq)
        a = _engine(plugin_of[dim], num_exclude_recent=0, inter_mode=1, robot_num=2, this_id=0, report_dims=33)
        try:
            a.save_from_wire_many(np.concatenate((keys, queries)), np.concatenate((np.zeros(N), np.ones(nq))))
            ids, dists, found = a.detect_inter_topk(np.arange(N, N + nq), K)
            for i, want in enumerate(gold["cases"][name]["results"]):
                if want.get("tie"):
                    continue
                assert found[i] == want["found"] and [int(x) for x in ids[i, :found[i]]] == want["idx"], (name, i)
                d2 = np.array(want["d2_bits"], np.uint32).view(np.float32)
                assert np.array_equal(dists[i, :found[i]].view(np.uint32), np.sqrt(d2).view(np.uint32)), (name, i)
        finally:
            a.close()


# ---- errors ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("plugin", ("m2dp", "fpfh", "grsd"))
def test_errors_change_nothing(plugin):
    """k = 0 and k = 33: SCL_ERR_INVALID_ARG; one cur out of range in the middle: SCL_ERR_OUT_OF_RANGE; the outputs keep their
    sentinels and a following single detect_inter answers as on a handle that never saw the calls (the reference's inter mode: its
    counter is where it was).  count = 0 is fine; cand_dists and n_found may be NULL"""
    kw = dict(num_exclude_recent=5, tree_making_period=2, inter_mode=0, robot_num=2, this_id=0)
    rows = plugin_rows(plugin, 129, seed=71)
    a, b, m = _engine(plugin, **kw), _engine(plugin, **kw), _model(plugin, **kw)
    try:
        _fill([a, b], m, rows[:120], np.arange(120) % 2)
        assert same_detection(a.detect_inter(7), b.detect_inter(7))              # the counter is odd now: no rebuild at the next call
        m.sets("inter", [7])
        _fill([a, b], m, rows[120:], np.arange(120, 129) % 2)
        good = np.array([1, 2, 3, 4, 5, 6] * 4)
        for form, curs, k, status in (("inter", good, 0, INVALID_ARG), ("intra", good, 33, INVALID_ARG), ("inter", good, -1, INVALID_ARG),
                                      ("inter", np.where(good == 4, 129, good), 10, OUT_OF_RANGE), ("inter", np.where(good == 4, -1, good), 10, OUT_OF_RANGE),
                                      ("intra", np.where(good == 4, a.get_size(0), good), 10, OUT_OF_RANGE), ("intra", np.where(good == 4, -3, good), 1, OUT_OF_RANGE)):
            rows_k = max(k, 0)
            ids, dists = np.full((curs.size, rows_k), -7, np.int32), np.full((curs.size, rows_k), 123.0, np.float32)
            found = np.full(curs.size, -9, np.int32)
            with pytest.raises(type(a).ERROR) as err:
                getattr(a, f"detect_{form}_topk")(curs, k, ids=ids, dists=dists, n_found=found)
            assert err.value.status == status, (form, k)
            assert (ids == -7).all() and (dists == 123.0).all() and (found == -9).all()
        for cur in (128, 0, 64):
            assert same_detection(a.detect_inter(cur), b.detect_inter(cur)), cur
            m.sets("inter", [cur])
        for form in ("intra", "inter"):
            ids, dists, found = getattr(a, f"detect_{form}_topk")(np.zeros(0, np.int32), 10)
            assert ids.shape == (0, 10) and found.size == 0
        curs = np.arange(10, 40, dtype=np.int32)
        want = m.topk("inter", curs, 10)
        ids = np.full((curs.size, 10), -7, np.int32)
        fn = getattr(a.L, f"scl_{plugin}_detect_inter_topk")
        assert fn(a.h, curs.ctypes.data_as(POINTER(c_int)), curs.size, 10, ids.ctypes.data_as(POINTER(c_int)), POINTER(c_float)(), POINTER(c_int)()) == 0
        assert np.array_equal(ids, want[0])
        b.detect_inter_many(curs)
        assert same_detection(a.detect_inter(77), b.detect_inter(77))
    finally:
        a.close(); b.close()


# ---- regrown work buffers -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("plugin", ("m2dp", "fpfh", "grsd"))
def test_work_buffers_regrow(plugin):
    """16 queries at k = 2, then the database grows tenfold and 600 queries at k = 32 (the query, partial-list, result and list buffers
    all grow), then 16 at k = 2 and 40 at k = 10 again on the same handle"""
    kw = dict(num_exclude_recent=10, inter_mode=1, robot_num=2, this_id=0)
    rows = plugin_rows(plugin, 3000, seed=81)
    assert rows.shape[1] == DIMS[plugin]
    robots = np.arange(3000) % 2
    a, m = _engine(plugin, **kw), _model(plugin, **kw)
    try:
        _fill([a], m, rows[:300], robots[:300])
        rs = np.random.RandomState(82)
        _same_as_model("intra", a, m, rs.randint(0, 150, size=16), 2)
        _same_as_model("inter", a, m, rs.randint(0, 300, size=16), 2)
        _fill([a], m, rows[300:], robots[300:])
        for count, k in ((600, 32), (16, 2), (40, 10)):
            _same_as_model("intra", a, m, rs.randint(0, 1500, size=count), k)
            _same_as_model("inter", a, m, rs.randint(0, 3000, size=count), k)
    finally:
        a.close()
