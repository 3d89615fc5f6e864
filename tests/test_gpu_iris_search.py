"""The exhaustive ranked search of the LiDAR-Iris plugin (scl_iris_search_intra / scl_iris_search_inter) against the CPU checker
(tests/iris_search_cases.py: iriso_hamming_all per pair, a Python sort) and against scl_iris_hamming_all_shifts over the same sets
on a twin handle.  Every id, shift, score and n_found is compared by bit pattern.

The keyframes are random clouds (synth_scan, as tests/test_gpu_iris_batch.py draws them) turned into wire vectors by the CPU
restatement and stored with save_from_wire_many (wire_decode = 1).  A world draws its keyframes from a small pool of distinct clouds,
so equal scores at different positions are everywhere and the checker scores a pair of clouds once.

What the kernels can get wrong, and where it is reached: iris_search_score_kernel runs one workgroup per candidate, one lane per
shift (one wave at 23 and 1 columns, two at 72, six at 360, passes of 512 lanes at 520 columns), four queries per candidate word
(query counts 1, 15, 16, 17, 33), the staged candidate in LDS or, past 65 280 bytes (160 x 200), read from global memory;
iris_select_kernel strides over a query's scores by 256 (sets of 255, 256, 257).
"""
from ctypes import POINTER, c_float, c_int

import numpy as np
import pytest

from iris_search_cases import World, assert_same_lists
from scl_slam_amd.synth import synth_scan

pytestmark = pytest.mark.gpu

SMALL = dict(rows=16, cols=72, nscan=16, nscale=2)
INVALID_ARG, OUT_OF_RANGE = -1, -4                                                    # include/scl_engine.h
KS = (1, 2, 31, 32)


def _engine(conf, w, **kw):
    from scl_slam_amd.iris import IrisEngine
    kw.setdefault("wire_decode", 1)
    return IrisEngine(robot_num=w.robot_num, this_id=w.this_id, num_exclude_recent=w.num_exclude_recent, **conf, **kw)


def _scan(seed, n, reach):
    return np.ascontiguousarray(synth_scan(n, seed=seed, max_range=reach + 5.0)[:, :8])


def _pool(w, count, n_points=3000, seed0=4100):
    for i in range(count):
        w.add_cloud(i, _scan(seed0 + i, n_points + 61 * (i % 17), float(w.cfg.rows)))
    w.add_blank("blank")


def _fill(e, w, first=0):
    e.save_from_wire_many(*w.wire_rows(first))


def _twin_scores(twin):
    return lambda qkey, keys: twin.hamming_all_shifts(qkey, keys)


def _check(e, twin, w, mode, curs, k, what=""):
    got = getattr(e, f"search_{mode}")(curs, k)
    assert_same_lists(got, w.expected(mode, curs, k), (what, mode, k, "checker"))
    if twin is not None:
        assert_same_lists(got, w.expected(mode, curs, k, _twin_scores(twin)), (what, mode, k, "hamming_all_shifts"))
    return got


# ---- the small shape: one world and two handles for the whole module ------------------------------------------------------------
EXCL = 3


@pytest.fixture(scope="module")
def small():
    """320 keyframes, robot 1's every fifth: robot 0 has 256, so that its sets reach 253 = 256 - EXCL; the same cloud at local
    indices 254 and 255, blank keyframes among both robots' and as queries"""
    w = World(SMALL, robot_num=2, this_id=0, num_exclude_recent=EXCL)
    _pool(w, 40)
    rs = np.random.RandomState(7)
    for key in range(320):
        robot = 1 if key % 5 == 4 else 0
        wid = int(rs.randint(0, 40))
        if key in (11, 14, 200):
            wid = "blank"
        w.push(wid, robot)
    e, twin = _engine(SMALL, w), _engine(SMALL, w, shift_search=1, match_num=0, num_candidates=3, knn_exclude_eps=0.0)
    _fill(e, w); _fill(twin, w)
    yield w, e, twin
    e.close(); twin.close()


@pytest.mark.parametrize("k", KS)
def test_set_sizes_around_k_and_empty_sets(small, k):
    w, e, twin = small
    sizes = sorted({0, 1, max(k - 1, 0), k, k + 1})
    curs = [0, 1, EXCL] + [EXCL + s for s in sizes]                     # cur <= EXCL: an empty set
    got = _check(e, twin, w, "intra", curs, k)
    assert got[3][:3].tolist() == [0, 0, 0] and np.all(got[0][:3] == -1) and np.all(np.isinf(got[2][:3])) and not got[1][:3].any()


@pytest.mark.parametrize("count", (1, 15, 16, 17, 33))
def test_query_counts_around_the_launch_group_with_different_limits(small, count):
    w, e, twin = small
    mine = len(w.keys_of[0])
    curs = [(mine - 1 - 37 * i) % mine for i in range(count)]          # limits from 0 to 252, unordered
    if count > 2:
        curs[2] = curs[0]                                               # a query repeated within the call
    _check(e, twin, w, "intra", curs, 5, count)


def test_an_inter_batch_mixing_own_and_received_keyframes(small):
    w, e, twin = small
    curs = [0, 4, 9, 1, 319, 318, 4, 11, 14, 200, 199] + list(range(100, 112))    # both lists in one call; blank queries 11, 14 (robot 1's), 200
    for k in (2, 32):
        got = _check(e, twin, w, "inter", curs, k)
        assert got[3][7] == 0 and got[3][8] == 0 and got[3][9] == 0    # a fully masked query lists nothing
    assert w.robots[14] == 1 and w.robots[11] == 0


def test_blank_keyframes_are_never_listed_and_duplicates_keep_their_order(small):
    w, e, twin = small
    mine = w.keys_of[0]
    blanks = [i for i, key in enumerate(mine) if w.wids[key] == "blank"]
    assert len(blanks) >= 2
    got = _check(e, twin, w, "intra", [255, 200, 100, blanks[1]], 32)
    for row, found in zip(got[0], got[3]):
        assert not set(row[:found].tolist()) & set(blanks)
    assert got[3][3] == 0
    # equal scores come back in position order: within a list, ids of one score ascend
    for ids, dists, found in zip(got[0], got[2], got[3]):
        for a in range(1, found):
            assert dists[a - 1] < dists[a] or (dists[a - 1] == dists[a] and ids[a - 1] < ids[a])


def test_argument_errors_leave_the_outputs_untouched(small):
    from scl_slam_amd.iris import IrisError
    w, e, _ = small
    n, mine = len(w.wids), len(w.keys_of[0])
    for mode, curs, k, status in (("intra", [5, 6], 0, INVALID_ARG), ("inter", [5, 6], 33, INVALID_ARG), ("intra", [5, -1], -3, INVALID_ARG),
                                  ("intra", [5, mine, 6], 4, OUT_OF_RANGE), ("intra", [-1], 4, OUT_OF_RANGE), ("inter", [0, n], 4, OUT_OF_RANGE),
                                  ("inter", [5, -1, 6], 32, OUT_OF_RANGE)):
        rows = max(k, 1)
        ids = np.full((len(curs), rows), -77, np.int32); biases = np.full((len(curs), rows), -77.0, np.float32)
        dists = np.full((len(curs), rows), -77.0, np.float32); found = np.full(len(curs), -77, np.int32)
        c = np.ascontiguousarray(curs, np.int32)
        rc = getattr(e.L, f"scl_iris_search_{mode}")(e.h, c.ctypes.data_as(POINTER(c_int)), c.size, k, ids.ctypes.data_as(POINTER(c_int)),
                                                     biases.ctypes.data_as(POINTER(c_float)), dists.ctypes.data_as(POINTER(c_float)),
                                                     found.ctypes.data_as(POINTER(c_int)))
        assert rc == status, (mode, curs, k, rc)
        assert np.all(ids == -77) and np.all(biases == -77.0) and np.all(dists == -77.0) and np.all(found == -77)
    with pytest.raises(IrisError) as ei:
        e.search_intra([0], 33)
    assert ei.value.status == INVALID_ARG
    # count == 0 is SCL_OK, and the optional outputs may be NULL
    assert e.search_intra([], 4)[3].size == 0
    c = np.array([255], np.int32); ids = np.empty(4, np.int32)
    assert e.L.scl_iris_search_intra(e.h, c.ctypes.data_as(POINTER(c_int)), 1, 4, ids.ctypes.data_as(POINTER(c_int)), None, None, None) == 0
    assert ids.tolist() == w.expected("intra", [255], 4)[0][0].tolist()


def test_a_search_between_two_detections_changes_neither(small):
    w, e, twin = small
    # `twin` detects with shift_search = 1; a third handle with the same configuration never searches
    ref = _engine(SMALL, w, shift_search=1, match_num=0, num_candidates=3, knn_exclude_eps=0.0)
    _fill(ref, w)
    intra, inter = [255, 254, 100, 40, 3], [319, 4, 0, 150, 151]
    want = (ref.detect_intra_many(intra), ref.detect_inter_many(inter))
    before = (twin.detect_intra_many(intra), twin.detect_inter_many(inter))
    got = (twin.search_intra(intra, 7), twin.search_inter(inter, 32))
    after = (twin.detect_intra_many(intra), twin.detect_inter_many(inter))
    for a, b, c in zip(want, before, after):
        for x, y, z in zip(a, b, c):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)) and np.array_equal(x.view(np.uint32), z.view(np.uint32))
    # the twin's configuration (shift_search, match_num, num_candidates, knn_exclude_eps) does not show in the lists
    assert_same_lists(got[0], e.search_intra(intra, 7), "twin intra")
    assert_same_lists(got[1], e.search_inter(inter, 32), "twin inter")
    assert_same_lists(got[0], w.expected("intra", intra, 7), "twin intra, checker")
    assert twin.detect_intra(255) == ref.detect_intra(255)             # nor do the single calls' buffers
    ref.close()


def test_growth_inside_the_test_and_sets_around_256(small):
    """a handle of its own: 250 keyframes, a search, 15 more (the capacity of 256 is passed), then sets of 255, 256 and 257 and
    smaller calls again on the same work buffers"""
    w0, _, _ = small
    w = World(SMALL, robot_num=1, this_id=0, num_exclude_recent=1)
    w.feats, w.wires, w._scores = w0.feats, w0.wires, w0._scores        # the pool and its scores are shared, nothing is changed
    rs = np.random.RandomState(11)
    for _ in range(250):
        w.push(int(rs.randint(0, 40)))
    e, twin = _engine(SMALL, w), _engine(SMALL, w)
    _fill(e, w); _fill(twin, w)
    _check(e, twin, w, "intra", [249, 10], 2, "before growth")
    for key in range(250, 265):
        w.push("blank" if key == 256 else int(rs.randint(0, 40)))
    w.wids[255], w.wids[257] = w.wids[254], w.wids[254]                 # one cloud at positions 254, 255 and 257
    _fill(e, w, 250); _fill(twin, w, 250)
    _check(e, twin, w, "intra", [256, 257, 258, 264, 2, 1], 32, "after growth")      # sets of 255, 256, 257, 263, 1 and 0
    _check(e, twin, w, "intra", [258], 1, "smaller call")
    _check(e, twin, w, "inter", [0, 264], 3, "one robot: nothing to search")
    e.close(); twin.close()


def test_a_few_thousand_keyframes(small):
    w0, _, _ = small
    w = World(SMALL, robot_num=2, this_id=1, num_exclude_recent=50)
    w.feats, w.wires, w._scores = w0.feats, w0.wires, w0._scores
    rs = np.random.RandomState(13)
    for key in range(2600):
        w.push("blank" if key % 701 == 5 else int(rs.randint(0, 40)), 0 if key % 13 == 0 else 1)
    e, twin = _engine(SMALL, w), _engine(SMALL, w)
    _fill(e, w); _fill(twin, w)
    mine = len(w.keys_of[1])
    _check(e, twin, w, "intra", [mine - 1, mine - 2, 1000, 60, mine - 1], 32, "thousands")
    _check(e, None, w, "inter", [0, 13, 1, 2599], 31, "thousands")
    e.close(); twin.close()


# ---- the other shapes ------------------------------------------------------------------------------------------------------------
def _shape_case(conf, n_keys, n_points, intra, inter, ks, pool=None, excl=1):
    w = World(conf, robot_num=2, this_id=0, num_exclude_recent=excl)
    _pool(w, pool or n_keys, n_points)
    for key in range(n_keys):
        w.push("blank" if key == 3 else key % (pool or n_keys), 1 if key % 4 == 2 else 0)
    e, twin = _engine(conf, w), _engine(conf, w)
    _fill(e, w); _fill(twin, w)
    for k in ks:
        got_a = _check(e, twin, w, "intra", intra, k, conf)
        got_b = _check(e, twin, w, "inter", inter, k, conf)
    e.close(); twin.close()
    return got_a, got_b


def test_the_defaults_80_x_360():
    a, b = _shape_case(dict(rows=80, cols=360, nscan=64, nscale=4), 12, 20000, intra=[8, 5], inter=[2, 11], ks=(32,), pool=12)
    assert a[3].tolist() == [6, 3] and b[3].tolist() == [8, 3]        # robot 0: keys 0, 1, 3 (blank), 4, 5, 7, 8, 9, 11; robot 1: 2, 6, 10


def test_odd_rows_and_cols_5_x_23():
    """trows = 40: the second word of a column holds 8 template bits and 24 padding bits; shift_search = 0 is left on, and the search
    does not return SCL_ERR_UNSUPPORTED as the detections do without the FFT estimate"""
    a, _ = _shape_case(dict(rows=5, cols=23, nscan=16, nscale=4), 40, 1500, intra=[29, 17, 2, 29], inter=[2, 0, 38, 39], ks=(1, 32), pool=20)
    assert a[3][0] > 20


def test_one_column():
    """cols = 1: the log-Gabor filter of one sample is zero, every template bit is masked and every pair is NaN"""
    a, b = _shape_case(dict(rows=4, cols=1, nscan=16, nscale=2), 9, 500, intra=[6, 1], inter=[2, 0], ks=(2,), pool=4)
    assert not a[3].any() and not b[3].any()


def test_more_shifts_than_lanes_2_x_520():
    _shape_case(dict(rows=2, cols=520, nscan=64, nscale=1), 9, 4000, intra=[6, 5], inter=[2, 0], ks=(4,), pool=6)


def test_a_template_past_the_lds_budget_160_x_200():
    """trows = 1 280, 40 words a column: 200 x 41 x 8 = 65 600 bytes do not fit the staged form, the candidate is read from global memory"""
    _shape_case(dict(rows=160, cols=200, nscan=64, nscale=4), 6, 30000, intra=[4, 2], inter=[2], ks=(3,), pool=5)
