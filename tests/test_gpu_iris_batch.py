"""The batch forms of the LiDAR-Iris plugin (scl_iris.h "THE BATCH FORMS": make_and_save_many, save_from_wire_many,
detect_intra_many, detect_inter_many, make_save_and_detect) against the single calls of the same library and the CPU restatement.

Every test builds two handles with one configuration: A is driven by single calls, B by batch calls.  Outputs are compared by bit
pattern (uint32 views of the floats), the stored state key by key: get_image, the row key's bits, get_feature, get_size, get_index,
local_to_global.  No tolerance anywhere: the reference points are the single-call path and oracle/iris_plugin_oracle.py.

Working configuration 16 x 72 x 2 scales with scans of 2 000 - 4 000 points: a launch group of 16, the group boundary, the initial
capacity of 256 and every rule of the candidate selection are reached within 40 - 60 keyframes.
"""
import math

import numpy as np
import pytest

import oracle_binding as ob
import oracle_iris_binding as oi
from oracle.iris_plugin_oracle import IrisPluginOracle
from scl_slam_amd.synth import synth_scan

CONF = dict(rows=16, cols=72, nscan=64, nscale=2)
FLT_EPSILON = float(np.finfo(np.float32).eps)
NO_SEARCH = (-1, 0.0, 10000000.0)
BYTE_RULE = [-300.7, -1.5, -0.4, 0.4, 255.9, 256.2, 1e12, -1e12, np.nan, np.inf]      # the values of tests/test_iris_plugin.py
OUT_OF_RANGE, INVALID_ARG, UNSUPPORTED = -4, -1, -6                                  # include/scl_engine.h


def _engine(**kw):
    from scl_slam_amd.iris import IrisEngine
    return IrisEngine(**kw)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _scan(seed, n=3000, reach=16.0, width=8):
    return np.ascontiguousarray(synth_scan(n, seed=seed, max_range=reach + 5.0)[:, :width])


def _place(seed, n=3000):
    """a place of its own for the 16 x 72 geometry, whose columns are the yaws -180 ... -108 degrees (getIris takes a column per
    degree and a row per metre whatever the image size; every other yaw clamps into the last column): a wall per 3-degree sector
    inside that span, at a drawn range in the middle of a row and up to a drawn height, so that two places share little and a
    revisit under a few degrees of yaw is a clean column shift"""
    rs = np.random.RandomState(seed)
    wall = rs.randint(2, 15, 18) + 0.5; top = rs.uniform(-1.0, 3.5, 18)
    yaw_deg = rs.uniform(-172.0, -118.0, n)
    sector = np.minimum(((yaw_deg + 172.0) / 3.0).astype(int), 17)
    d = wall[sector] + rs.uniform(-0.15, 0.15, n)
    yaw = np.radians(yaw_deg)
    c = np.zeros((n, 8), np.float32)
    c[:, 0], c[:, 1], c[:, 2] = d * np.cos(yaw), d * np.sin(yaw), rs.uniform(-1.6, top[sector])
    return c


def _moved(cloud, yaw_deg, dx, dy, seed):
    """a revisit as tests/test_iris_plugin.py plants it: another heading, a little off the first track, range noise"""
    rs = np.random.RandomState(seed)
    th = math.radians(yaw_deg)
    out = cloud.copy()
    x, y = cloud[:, 0] - dx, cloud[:, 1] - dy
    out[:, 0] = math.cos(th) * x - math.sin(th) * y + 0.01 * rs.standard_normal(len(x))
    out[:, 1] = math.sin(th) * x + math.cos(th) * y + 0.01 * rs.standard_normal(len(x))
    return out


def _fan(reach, seed, n=2500):
    """elevations -20 ... +20 degrees at every yaw, ranges past `reach` (tests/test_gpu_iris_configs.py)"""
    rs = np.random.RandomState(seed)
    el = np.radians(rs.uniform(-20.0, 20.0, n)); yaw = rs.uniform(-math.pi, math.pi, n); d = rs.uniform(0.2, reach * 1.2, n)
    c = np.zeros((n, 8), np.float32)
    c[:, :3] = np.stack([d * np.cos(yaw), d * np.sin(yaw), d * np.tan(el)], axis=1)
    return c


def assert_same_state(a, b, robot_num, first_key=0):
    """the stored state of two handles, key by key from first_key on"""
    n = a.get_size()
    assert n == b.get_size()
    for r in range(robot_num):
        assert a.get_size(r) == b.get_size(r), r
        for local in range(a.get_size(r)):
            assert a.local_to_global(r, local) == b.local_to_global(r, local), (r, local)
    for key in range(first_key, n):
        assert a.get_index(key) == b.get_index(key), key
        (ia, ka), (ib, kb) = a.get_image(key), b.get_image(key)
        assert np.array_equal(ia, ib) and np.array_equal(_bits(ka), _bits(kb)), key
        (ta, ma), (tb, mb) = a.get_feature(key), b.get_feature(key)
        assert np.array_equal(ta, tb) and np.array_equal(ma, mb), key


def assert_state_equals_oracle(e, po):
    assert e.get_size() == po.get_size()
    for key in range(po.get_size()):
        robot, _ = po.get_index(key)
        assert e.get_index(key) == po.get_index(key)
        local = po.local2global[robot].index(key)
        img, rk = e.get_image(key)
        T, M = e.get_feature(key)
        f = po.features[robot][local]
        assert np.array_equal(img, f[0]) and np.array_equal(_bits(rk), _bits(po.rowkeys[robot][local])), key
        assert np.array_equal(T, f[1]) and np.array_equal(M, f[2]), key


def singles(fn, curs):
    """(loops, biases, dists) of the single call fn over curs, as the batch returns them"""
    r = [fn(int(c)) for c in curs]
    return (np.array([x[0] for x in r], np.int32), np.array([x[1] for x in r], np.float32), np.array([x[2] for x in r], np.float32))


def assert_same_answers(got, want, what=""):
    assert np.array_equal(got[0], want[0]), (what, got[0], want[0])
    assert np.array_equal(_bits(got[1]), _bits(want[1])), (what, got[1], want[1])
    assert np.array_equal(_bits(got[2]), _bits(want[2])), (what, got[2], want[2])


def _wire_of(cfg, cloud):
    img, key = oi.make_image(cfg, cloud)
    return np.concatenate([img.reshape(-1).astype(np.float32), key])


def _edge_clouds(width, reach, seed):
    """the clouds a builder must not trip over: empty, one point, NaN / inf coordinates, the elevation fan"""
    special = np.zeros((6, width), np.float32)
    special[:, :3] = [[3, 4, np.nan], [np.inf, 1, 1], [np.nan, np.nan, 1], [1, -np.inf, 2], [2, 2, 0.5], [-3, 1, 1.5]]
    one = np.zeros((1, width), np.float32); one[0, :3] = [2.5, -1.0, 0.7]
    return [np.zeros((0, width), np.float32), one, special, np.ascontiguousarray(_fan(reach, seed)[:, :width])]


# ---- 1. builders over the group boundary ---------------------------------------------------------------------------------------
def _builders(conf, calls, n_points):
    """calls: [(count, record width in floats)]; A by single calls, B by one make_and_save_many per entry"""
    rows = conf["rows"]
    cfg = oi.config(**conf)
    A, B = _engine(robot_num=2, **conf), _engine(robot_num=2, **conf)
    seed = 0
    for count, width in calls:
        clouds = [_scan(900 + seed + k, n=n_points + 61 * (k % 17), reach=float(rows), width=width) for k in range(count)]
        edge = _edge_clouds(width, float(rows), seed)
        for k, c in enumerate(edge[:count]):
            clouds[(3 * k + 1) % count] = c
        seed += count
        robots = [k % 2 for k in range(count)]; indexs = [100 + k for k in range(count)]
        want = [A.make_and_save(c, robots[k], indexs[k]) for k, c in enumerate(clouds)]
        got = B.make_and_save_many(clouds, robots, indexs)
        assert got.shape == (count, rows * conf["cols"] + rows)
        for k, c in enumerate(clouds):
            assert np.array_equal(_bits(got[k]), _bits(want[k])), (count, width, k)
            assert np.array_equal(_bits(got[k]), _bits(_wire_of(cfg, c))), (count, width, k)
        again = min(2, count)
        assert B.make_and_save_many(clouds[:again], robots[:again], indexs[:again], want_values=False) is None      # out_values may be NULL
        for k in range(again):
            A.make_and_save(clouds[k], robots[k], indexs[k])
    assert B.make_and_save_many([], [], []).shape[0] == 0                                               # count == 0 is OK
    assert_same_state(A, B, 2)
    A.close(); B.close()


@pytest.mark.gpu
@pytest.mark.parametrize("conf", [CONF, dict(rows=10, cols=100, nscan=64, nscale=3)], ids=["16x72x2", "10x100x3"])
def test_builders_over_the_group_boundary(conf):
    """counts 1, 16, 17 and 33 in successive calls, strides 32 / 12 / 16 / 32, with an empty cloud, a one-point cloud, NaN and inf
    coordinates and the fan among them; 10 x 100 x 3 has 60 template rows: padding bits in the last word"""
    _builders(conf, [(1, 8), (16, 3), (17, 4), (33, 8)], 2000)


@pytest.mark.gpu
@pytest.mark.parametrize("nscan", [64, 16])
def test_builders_at_the_defaults(nscan):
    """80 x 360 x 4 scales, 17 scans: the whole image in LDS, two launch groups"""
    _builders(dict(rows=80, cols=360, nscan=nscan, nscale=4), [(17, 8)], 4000)


@pytest.mark.gpu
def test_builders_leave_other_beam_counts_empty():
    """nscan other than 16 / 64 leaves the image empty (D.h:538 / 560), in the batch as in the single call"""
    conf = dict(CONF, nscan=32)
    A, B = _engine(**conf), _engine(**conf)
    clouds = [_scan(40 + k) for k in range(3)]
    want = [A.make_and_save(c, 0, k) for k, c in enumerate(clouds)]
    got = B.make_and_save_many(clouds)
    assert np.array_equal(_bits(got), _bits(np.stack(want))) and not got.any()
    assert_same_state(A, B, 1)
    A.close(); B.close()


# ---- 2. growth inside a call ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_growth_inside_a_call():
    """250 single appends, then one batch of 20 across the initial capacity of 256: every earlier and new key compares equal"""
    rs = np.random.RandomState(11)
    A, B = _engine(**CONF), _engine(**CONF)
    for k in range(250):
        img = (rs.randint(1, 256, (16, 72)) * (rs.rand(16, 72) < 0.3)).astype(np.uint8)
        key = rs.uniform(0, 2, 16).astype(np.float32)
        A.save_image(img, key, 0, k); B.save_image(img, key, 0, k)
    clouds = [_scan(2000 + k, n=2000 + 100 * k) for k in range(20)]
    want = np.stack([A.make_and_save(c, 0, 250 + k) for k, c in enumerate(clouds)])
    got = B.make_and_save_many(clouds, indexs=np.arange(250, 270))
    assert np.array_equal(_bits(got), _bits(want))
    assert A.get_size() == 270
    assert_same_state(A, B, 1)
    A.close(); B.close()


# ---- 3. wire batch -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("decode", [0, 1])
def test_wire_batch(decode):
    """19 vectors with the byte rule's values in image cells and row keys: equal to the singles and to the restatement; one bad
    robot id anywhere stores nothing"""
    from scl_slam_amd.iris import IrisError
    rows, cols = CONF["rows"], CONF["cols"]
    kw = dict(robot_num=3, this_id=0, wire_decode=decode, **CONF)
    cfg = oi.config(**CONF)
    vecs = np.stack([_wire_of(cfg, _scan(3000 + k)) for k in range(19)])
    rs = np.random.RandomState(5)
    for k in range(19):
        cells = rs.choice(rows * cols, size=40, replace=False)
        vecs[k, cells] = np.resize(np.roll(BYTE_RULE, k), 40)
        if k % 3 == 0:
            vecs[k, rows * cols + (np.arange(10) + k) % rows] = BYTE_RULE
    vecs[4, :rows * cols] = 0.0                                                        # an empty image from the wire
    robots = [1 + k % 2 for k in range(19)]; indexs = [7 * k for k in range(19)]
    A, B, po = _engine(**kw), _engine(**kw), IrisPluginOracle(oi, ob, **kw)
    for k in range(19):
        A.save_from_wire(vecs[k], robots[k], indexs[k]); po.save_from_wire(vecs[k], robots[k], indexs[k])
    B.save_from_wire_many(vecs, robots, indexs)
    assert_same_state(A, B, 3)
    assert_state_equals_oracle(B, po)
    for bad_at in (0, 9, 18):
        bad = list(robots); bad[bad_at] = 3
        with pytest.raises(IrisError) as ei:
            B.save_from_wire_many(vecs, bad, indexs)
        assert ei.value.status == INVALID_ARG and B.get_size() == 19
    B.save_from_wire_many(np.zeros((0, rows * cols + rows), np.float32), [], [])        # count == 0
    B.save_from_wire_many(vecs[:2], robots[:2], indexs[:2]); A.save_from_wire(vecs[0], robots[0], indexs[0]); A.save_from_wire(vecs[1], robots[1], indexs[1])
    assert_same_state(A, B, 3, first_key=17)
    A.close(); B.close()


# ---- 4. detections: batch = singles = restatement ------------------------------------------------------------------------------
DETECT_KW = dict(num_exclude_recent=5, num_candidates=3, robot_num=3, this_id=0, wire_decode=1, **CONF)
_scenario_cache = {}


def detection_scenario():
    """44 keyframes of this robot with two planted revisits (30 sees place 3, 40 sees place 12), 8 received from robot 1 (its 3 sees
    this robot's place 9) and 4 from robot 2, in interleaved arrival.  [(robot, index, cloud or None, wire vector)], made once"""
    if not _scenario_cache:
        cfg = oi.config(**CONF)
        scans = [_place(300 + k, n=2000 + 50 * (k % 40)) for k in range(44)]
        scans[30] = _moved(scans[3], 4.0, 0.05, -0.03, 1)
        scans[40] = _moved(scans[12], -3.0, -0.04, 0.05, 4)
        remote = [_place(500 + k) for k in range(8)]
        remote[3] = _moved(scans[9], 5.0, 0.03, 0.04, 3)
        third = [_place(600 + k) for k in range(4)]
        order = [(0, k) for k in range(10)] + [(1, k) for k in range(4)] + [(0, k) for k in range(10, 25)] + [(2, k) for k in range(2)] + \
                [(0, k) for k in range(25, 40)] + [(1, k) for k in range(4, 8)] + [(2, k) for k in range(2, 4)] + [(0, k) for k in range(40, 44)]
        arrivals = []
        for robot, k in order:
            cloud = (scans, remote, third)[robot][k]
            arrivals.append((robot, k, cloud if robot == 0 else None, _wire_of(cfg, cloud)))
        _scenario_cache["arrivals"] = arrivals
        po = IrisPluginOracle(oi, ob, **DETECT_KW)
        for robot, k, cloud, wire in arrivals:
            po.make_and_save(cloud, robot, k) if cloud is not None else po.save_from_wire(wire, robot, k)
        _scenario_cache["oracle"] = po
    return _scenario_cache["arrivals"], _scenario_cache["oracle"]


def _load_singles(e, arrivals):
    for robot, k, cloud, wire in arrivals:
        e.make_and_save(cloud, robot, k) if cloud is not None else e.save_from_wire(wire, robot, k)


def _load_batches(e, arrivals):
    """runs of one robot's arrivals in one batch call each"""
    i = 0
    while i < len(arrivals):
        j = i
        while j < len(arrivals) and (arrivals[j][2] is None) == (arrivals[i][2] is None):
            j += 1
        run = arrivals[i:j]
        if run[0][2] is not None:
            e.make_and_save_many([a[2] for a in run], [a[0] for a in run], [a[1] for a in run], want_values=False)
        else:
            e.save_from_wire_many(np.stack([a[3] for a in run]), [a[0] for a in run], [a[1] for a in run])
        i = j


@pytest.mark.gpu
@pytest.mark.parametrize("shift_search,match_num", [(0, 2), (0, 0), (0, 1), (1, 2)])
def test_detections_equal_singles_and_restatement(shift_search, match_num):
    arrivals, po = detection_scenario()
    po.match_num, po.shift_search = match_num, shift_search
    kw = dict(DETECT_KW, match_num=match_num, shift_search=shift_search)
    A, B = _engine(**kw), _engine(**kw)
    _load_singles(A, arrivals); _load_batches(B, arrivals)
    assert_same_state(A, B, 3)
    n, mine = A.get_size(), A.get_size(0)
    assert (n, mine) == (56, 44)
    # intra: every local index in one call (three launch groups), then shuffled with repeats
    curs = np.arange(mine)
    want = singles(A.detect_intra, curs)
    assert_same_answers(B.detect_intra_many(curs), want, "intra")
    assert_same_answers(want, singles(po.detect_intra, curs), "intra restatement")
    assert want[0][30] == 3 and want[0][40] == 12, want[0]                             # the planted revisits
    assert tuple(x[4] for x in want) == NO_SEARCH and (want[2][:9] == 10000000.0).all() and want[2][9] < 10000000.0     # early-outs mixed in
    rs = np.random.RandomState(8)
    shuffled = np.concatenate([rs.permutation(mine), rs.randint(0, mine, 21), [30, 30, 0]])
    got = B.detect_intra_many(shuffled)
    assert_same_answers(got, tuple(w[shuffled] for w in want), "intra shuffled")
    loops_only = B.detect_intra_many(shuffled, want_dists=False)
    assert loops_only[2] is None and np.array_equal(loops_only[0], got[0]) and np.array_equal(_bits(loops_only[1]), _bits(got[1]))
    # inter: every global key, own and received queries mixed -- both lists within one launch group
    keys = np.arange(n)
    want = singles(A.detect_inter, keys)
    assert_same_answers(B.detect_inter_many(keys), want, "inter")
    assert_same_answers(want, singles(po.detect_inter, keys), "inter restatement")
    k_r3, k_own9 = po.local2global[1][3], po.local2global[0][9]
    assert want[0][k_r3] == k_own9 and want[0][k_own9] == k_r3, (want[0][k_r3], want[0][k_own9])      # the planted inter-robot revisit, both ways
    back = keys[::-1].copy()
    assert_same_answers(B.detect_inter_many(back), tuple(w[back] for w in want), "inter reversed")
    assert B.detect_intra_many([])[0].size == 0
    assert_same_state(A, B, 3, first_key=n - 1)
    A.close(); B.close()


# ---- 5. the selection's corner rules -------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("eps", [0.0, FLT_EPSILON])
def test_equal_row_keys_and_ties_by_position(eps):
    """identical images under equal row keys, saved several times: equal squared distances (0 among the copies), ties by position;
    with eps > 0 the copies at distance 0 are skipped"""
    kw = dict(num_exclude_recent=2, num_candidates=3, knn_exclude_eps=eps, **CONF)
    cfg = oi.config(**CONF)
    base = [oi.make_image(cfg, _scan(700 + k)) for k in range(4)]
    plan = [0, 1, 0, 0, 2, 1, 1, 3, 0, 2, 2, 0, 1, 3, 0, 0]                             # which base image / key every keyframe repeats
    A, B, po = _engine(**kw), _engine(**kw), IrisPluginOracle(oi, ob, **kw)
    for k, p in enumerate(plan):
        img = np.roll(base[p][0], 3 * (k % 5), axis=1)
        for e in (A, B):
            e.save_image(img, base[p][1], 0, k)
        po.save(img, base[p][1], 0, k)
    curs = np.arange(len(plan))
    want = singles(A.detect_intra, curs)
    assert_same_answers(B.detect_intra_many(curs), want)
    assert_same_answers(want, singles(po.detect_intra, curs), "restatement")
    if eps == 0.0:
        assert want[2][11] == 0.0 and want[0][11] == 0, (want[0][11], want[2][11])     # keyframe 11 = 0 unrolled: the FIRST of its copies wins
    else:
        assert (want[2][6:] > 0.0).all()
    A.close(); B.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shift_search", [0, 1])
def test_non_finite_row_keys_and_masked_candidates(shift_search):
    """received row keys holding NaN / inf: fewer than num_candidates qualify for this robot's queries, none for a received query whose
    own key is NaN -- (-1, 0, 10000000); all-zero images among the candidates: fully masked, a NaN distance takes part and never wins"""
    rows, cols = CONF["rows"], CONF["cols"]
    kw = dict(num_exclude_recent=2, num_candidates=3, robot_num=2, this_id=0, wire_decode=1, shift_search=shift_search, **CONF)
    cfg = oi.config(**CONF)
    A, B = _engine(**kw), _engine(**kw)
    own = [oi.make_image(cfg, _scan(800 + k)) for k in range(9)]
    own[2] = (np.zeros((rows, cols), np.uint8), own[2][1]); own[4] = (np.zeros((rows, cols), np.uint8), own[4][1])
    for k, (img, key) in enumerate(own):
        for e in (A, B):
            e.save_image(img, key, 0, k)
    vecs = np.stack([_wire_of(cfg, _scan(850 + k)) for k in range(6)])
    vecs[0, rows * cols + 3] = np.nan; vecs[1, rows * cols] = np.inf; vecs[2, rows * cols + 15] = -np.inf; vecs[5, rows * cols + 7] = np.nan
    vecs[3] = _wire_of(cfg, _moved(_scan(803), 15.0, 0.1, 0.0, 2))
    for k in range(6):
        A.save_from_wire(vecs[k], 1, k)
    B.save_from_wire_many(vecs, np.ones(6, np.int8), np.arange(6))
    assert_same_state(A, B, 2)
    keys = np.arange(15)
    want = singles(A.detect_inter, keys)
    got = B.detect_inter_many(keys)
    assert_same_answers(got, want, "inter")
    # received 0 and 5 carry a NaN in their own key: every distance NaN, nothing qualifies
    for k in (9, 14):
        assert tuple(x[k] for x in got) == NO_SEARCH
    # this robot's queries: two finite received keys of six -- two candidates for three slots, and they are compared
    assert (got[2][[0, 1, 3, 5, 6, 7, 8]] < 10000000.0).all()                          # (2 and 4 are the all-zero images: masked against everything)
    curs = np.arange(9)
    want = singles(A.detect_intra, curs)
    assert_same_answers(B.detect_intra_many(curs), want, "intra")
    if shift_search == 1:
        po = IrisPluginOracle(oi, ob, **kw)
        for k, (img, key) in enumerate(own):
            po.save(img, key, 0, k)
        assert_same_answers(want, singles(po.detect_intra, curs), "intra restatement")
    # a query that sees masked candidates only: keyframes 2 and 4 zero, and a third zero image in front
    C, D = _engine(**dict(kw, num_candidates=2)), _engine(**dict(kw, num_candidates=2))
    for k in range(8):
        img = own[0][0] if k >= 6 else np.zeros((rows, cols), np.uint8)
        for e in (C, D):
            e.save_image(img, own[k][1], 0, k)
    want = singles(C.detect_intra, np.arange(8))
    got = D.detect_intra_many(np.arange(8))
    assert_same_answers(got, want, "masked")
    assert tuple(x[7] for x in got) == NO_SEARCH and tuple(x[6] for x in got) == NO_SEARCH
    for e in (A, B, C, D):
        e.close()


@pytest.mark.gpu
def test_more_candidates_than_keyframes():
    kw = dict(num_exclude_recent=3, num_candidates=64, robot_num=2, **CONF)
    A, B = _engine(**kw), _engine(**kw)
    clouds = [_scan(60 + k) for k in range(20)]
    robots = [k % 2 for k in range(20)]
    for k, c in enumerate(clouds):
        A.make_and_save(c, robots[k], k)
    loops, biases, dists, _ = B.make_save_and_detect(clouds, robots, np.arange(20), want_values=False)
    assert (loops == -1).all() and (biases == 0.0).all() and (dists == 10000000.0).all()
    for curs, fa, fb in ((np.arange(10), A.detect_intra, B.detect_intra_many), (np.arange(20), A.detect_inter, B.detect_inter_many)):
        got = fb(curs)
        assert_same_answers(got, singles(fa, curs))
        assert (got[0] == -1).all() and (got[2] == 10000000.0).all()
    A.close(); B.close()


# ---- 6. errors leave no trace --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_errors_leave_no_trace():
    from scl_slam_amd.iris import IrisError
    arrivals, _ = detection_scenario()
    kw = dict(DETECT_KW)
    A, B = _engine(**kw), _engine(**kw)
    _load_singles(A, arrivals[:30]); _load_batches(B, arrivals[:30])
    mine, n = A.get_size(0), A.get_size()
    for fn, limit in ((B.detect_intra_many, mine), (B.detect_inter_many, n)):
        for bad in (limit, -1):
            curs = np.arange(limit); curs[limit // 2] = bad
            loops = np.full(limit, -77, np.int32); biases = np.full(limit, -7.5, np.float32); dists = np.full(limit, -3.25, np.float32)
            with pytest.raises(IrisError) as ei:
                fn(curs, loops, biases, dists)
            assert ei.value.status == OUT_OF_RANGE
            assert (loops == -77).all() and (biases == -7.5).all() and (dists == -3.25).all()
    assert_same_answers(B.detect_intra_many(np.arange(mine)), singles(A.detect_intra, np.arange(mine)))
    assert_same_answers(B.detect_inter_many(np.arange(n)), singles(A.detect_inter, np.arange(n)))
    A.close(); B.close()


@pytest.mark.gpu
def test_odd_sizes_answer_as_the_single_calls():
    """7 x 45: the FFT estimate refuses odd sizes.  With shift_search = 0 the batch returns the single call's status where a single
    call in order would reach it, and SCL_OK where none does; with shift_search = 1 it works and equals the singles"""
    from scl_slam_amd.iris import IrisError
    conf = dict(rows=7, cols=45, nscan=64, nscale=2, num_exclude_recent=3, num_candidates=2)
    clouds = [synth_scan(3000, seed=170 + k, max_range=12.0) for k in range(9)]
    for shift_search in (0, 1):
        A, B = _engine(shift_search=shift_search, **conf), _engine(shift_search=shift_search, **conf)
        for k, c in enumerate(clouds):
            A.make_and_save(c, 0, k)
        B.make_and_save_many(clouds)
        assert_same_state(A, B, 1)
        if shift_search == 1:
            assert_same_answers(B.detect_intra_many(np.arange(9)), singles(A.detect_intra, np.arange(9)))
            continue
        early = np.arange(6)                                                           # below 3 + 2 + 1: no single call searches
        assert_same_answers(B.detect_intra_many(early), singles(A.detect_intra, early))
        with pytest.raises(IrisError) as single:
            A.detect_intra(8)
        loops = np.full(9, -77, np.int32); biases = np.full(9, -7.5, np.float32)
        with pytest.raises(IrisError) as batch:
            B.detect_intra_many(np.arange(9), loops, biases)
        assert batch.value.status == single.value.status == UNSUPPORTED and "even" in str(batch.value)
        assert (loops == -77).all() and (biases == -7.5).all()
        assert B.get_size() == 9
        A.close(); B.close()


# ---- 7. make_save_and_detect ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shift_search", [0, 1])
def test_make_save_and_detect(shift_search):
    """against the loop make_and_save, detect_intra; interleaved robots; later scans of a batch revisit places stored earlier in
    the same batch; an invalid cloud or robot id stores nothing and leaves the outputs untouched"""
    from scl_slam_amd.iris import IrisError
    kw = dict(num_exclude_recent=3, num_candidates=2, robot_num=2, this_id=0, shift_search=shift_search, **CONF)
    A, B = _engine(**kw), _engine(**kw)
    places = [_scan(1200 + k) for k in range(14)]
    clouds, robots = [], []
    for k in range(40):
        if k in (17, 21, 30, 38):                                                      # revisits of places stored earlier in the same batch
            clouds.append(_moved(places[{17: 2, 21: 5, 30: 9, 38: 12}[k]], 10.0 * (k % 7) - 30.0, 0.1, -0.1, k))
        else:
            clouds.append(places[k % 14] if k < 14 else _scan(1300 + k))
        robots.append(1 if k % 5 == 4 else 0)
    at, mine, found = 0, 0, []
    for count in (1, 22, 17):
        batch, rb = clouds[at:at + count], robots[at:at + count]
        want = []
        for k, c in enumerate(batch):
            v = A.make_and_save(c, rb[k], at + k)
            if rb[k] == 0:
                want.append((A.detect_intra(mine), v)); mine += 1
            else:
                want.append((NO_SEARCH, v))
        loops, biases, dists, values = B.make_save_and_detect(batch, rb, np.arange(at, at + count))
        w = (np.array([x[0][0] for x in want], np.int32), np.array([x[0][1] for x in want], np.float32), np.array([x[0][2] for x in want], np.float32))
        assert_same_answers((loops, biases, dists), w, count)
        assert np.array_equal(_bits(values), _bits(np.stack([x[1] for x in want])))
        found += [int(x) for x in loops if x >= 0]
        at += count
    assert found, "no revisit found inside a batch: the test would pass on 'no loop anywhere'"
    assert_same_state(A, B, 2)
    n = B.get_size()
    sentinel = lambda: (np.full(3, -77, np.int32), np.full(3, -7.5, np.float32), np.full(3, -3.25, np.float32))      # noqa: E731
    for bad_clouds, bad_robots in (([c[:, :2] for c in clouds[:3]], [0, 0, 0]), (clouds[:3], [0, 2, 0])):             # stride 8; robot id 2 of 2
        loops, biases, dists = sentinel()
        with pytest.raises(IrisError) as ei:
            B.make_save_and_detect(bad_clouds, bad_robots, [0, 1, 2], loops=loops, biases=biases, dists=dists)
        assert ei.value.status == INVALID_ARG and B.get_size() == n
        assert (loops == -77).all() and (biases == -7.5).all() and (dists == -3.25).all()
    A.close(); B.close()


# ---- 8. interleaving -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shift_search", [0, 1])
def test_single_and_batch_calls_interleaved(shift_search):
    """one handle alternates single and batch calls (build, detect, wire), its twin makes single calls only: the two sets of work
    buffers do not disturb each other"""
    kw = dict(num_exclude_recent=3, num_candidates=2, robot_num=2, this_id=0, wire_decode=1, shift_search=shift_search, **CONF)
    cfg = oi.config(**CONF)
    A, B = _engine(**kw), _engine(**kw)
    clouds = [_scan(1500 + k, n=2000 + 97 * k) for k in range(24)]
    clouds[20] = _moved(clouds[4], 35.0, 0.1, 0.1, 6)
    wires = np.stack([_wire_of(cfg, _scan(1600 + k)) for k in range(8)])
    for k in range(24):
        A.make_and_save(clouds[k], 0, k)
    for k in range(8):
        A.save_from_wire(wires[k], 1, k)
    for k in range(0, 24, 6):                                                          # B: three singles, then a batch of three
        for j in range(k, k + 3):
            B.make_and_save(clouds[j], 0, j)
        B.make_and_save_many(clouds[k + 3:k + 6], indexs=np.arange(k + 3, k + 6))
        got = B.detect_intra_many(np.arange(k + 6))
        assert_same_answers(got, singles(B.detect_intra, np.arange(k + 6)), k)
        assert_same_answers(B.detect_intra_many(np.arange(k + 6)), got, k)               # the batch again, after the singles used their buffers
    B.save_from_wire(wires[0], 1, 0); B.save_from_wire_many(wires[1:4], [1, 1, 1], [1, 2, 3]); B.save_from_wire(wires[4], 1, 4)
    B.save_from_wire_many(wires[5:], [1, 1, 1], [5, 6, 7])
    assert_same_state(A, B, 2)
    keys = np.arange(32)
    for e in (A, B):
        assert_same_answers(B.detect_inter_many(keys), singles(e.detect_inter, keys))
        assert_same_answers(B.detect_intra_many(np.arange(24)), singles(e.detect_intra, np.arange(24)))
    A.close(); B.close()
