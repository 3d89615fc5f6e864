"""tests/iris_search_cases.py, the CPU checker of the exhaustive ranked search, pinned by answers worked out by hand: templates of
2 rows x 4 columns (rows = 1, nscale = 1), and the search sets of a registry of three robots.  No GPU."""
import numpy as np

from iris_search_cases import World, bits, rank

TINY = dict(rows=1, cols=4, nscale=1)
Z = [[0, 0, 0, 0], [0, 0, 0, 0]]


def _world(**kw):
    return World(TINY, **kw)


def test_the_first_minimum_among_equal_shifts_wins():
    w = _world()
    # the pattern repeats every two columns: shifts 0 and 2 give distance 0, shifts 1 and 3 give 4 / 8
    w.add_feature("q", [[255, 0, 255, 0], Z[1]], Z)
    w.add_feature("c", [[255, 0, 255, 0], Z[1]], Z)
    assert w.score("q", "c") == (np.float32(0.0), 0)
    # shifted by one column the query meets the candidate at shifts 1 and 3: the first is reported
    w.add_feature("c1", [[0, 255, 0, 255], Z[1]], Z)
    assert w.score("q", "c1") == (np.float32(0.0), 1)


def test_a_fully_masked_shift_is_skipped():
    w = _world()
    # query mask on columns 0, 1 (both rows), candidate mask on columns 2, 3.  The query is the shifted operand (dst(:, k) =
    # src(:, k - s)): shift 0 masks every bit (skipped); shift 1 leaves column 0 (2 bits); shift 2 leaves columns 0, 1 (4 bits);
    # shift 3 leaves column 1 (2 bits).  Candidate T has one bit at (row 0, column 0), the query's T is zero:
    # shift 1 -> 1 / 2, shift 2 -> 1 / 4, shift 3 -> 0 / 2
    w.add_feature("q", Z, [[255, 255, 0, 0], [255, 255, 0, 0]])
    w.add_feature("c", [[255, 0, 0, 0], Z[1]], [[0, 0, 255, 255], [0, 0, 255, 255]])
    assert w.score("q", "c") == (np.float32(0.0), 3)
    # with the candidate's bit moved to column 1 the distances are 0 / 2, 1 / 4, 1 / 2: shift 1 wins, shift 0 never counted
    w.add_feature("c2", [[0, 255, 0, 0], Z[1]], [[0, 0, 255, 255], [0, 0, 255, 255]])
    assert w.score("q", "c2") == (np.float32(0.0), 1)
    # and one bit on both columns: 1 / 2, 2 / 4, 1 / 2 -> the first of the equal minima, shift 1, at 0.5
    w.add_feature("c3", [[255, 255, 0, 0], Z[1]], [[0, 0, 255, 255], [0, 0, 255, 255]])
    assert w.score("q", "c3") == (np.float32(0.5), 1)


def test_a_fully_masked_pair_is_nan_and_leaves_the_list():
    w = _world()
    full = [[255] * 4, [255] * 4]
    w.add_feature("q", [[255, 0, 0, 0], Z[1]], Z)
    w.add_feature("blank", Z, full)
    w.add_feature("near", [[255, 0, 0, 0], Z[1]], Z)
    d, b = w.score("q", "blank")
    assert np.isnan(d) and b == -1
    for wid in ("near", "blank", "near", "q"):
        w.push(wid)
    ids, biases, dists, found = w.expected("intra", [3], 4)
    assert found.tolist() == [2] and ids.tolist() == [[0, 2, -1, -1]]
    assert biases.tolist() == [[0.0, 0.0, 0.0, 0.0]] and dists[0, :2].tolist() == [0.0, 0.0] and np.all(np.isinf(dists[0, 2:]))
    # the blank keyframe as the query: every pair is NaN, nothing is listed
    w.push("blank")
    ids, biases, dists, found = w.expected("intra", [4], 2)
    assert found.tolist() == [0] and ids.tolist() == [[-1, -1]] and np.all(np.isinf(dists))


def test_a_tie_between_two_candidates_goes_to_the_lower_position():
    w = _world()
    w.add_feature("q", [[255, 0, 0, 0], Z[1]], Z)
    w.add_feature("a", [[255, 255, 0, 0], Z[1]], Z)          # 1 / 8 at shifts 0 and 1
    w.add_feature("b", [[0, 255, 255, 0], Z[1]], Z)          # the same image one column on: 1 / 8 at shifts 1 and 2
    w.add_feature("far", [[255, 255, 255, 0], [255, 255, 255, 255]], Z)
    assert w.score("q", "a") == (np.float32(0.125), 0) and w.score("q", "b") == (np.float32(0.125), 1)
    for wid in ("far", "b", "a", "b", "q"):
        w.push(wid)
    ids, biases, dists, found = w.expected("intra", [4], 3)
    assert found.tolist() == [3] and ids.tolist() == [[1, 2, 3]] and biases.tolist() == [[1.0, 0.0, 1.0]]
    assert bits(dists).tolist() == [[bits(np.float32(0.125))[0]] * 3]
    assert w.expected("intra", [4], 1)[0].tolist() == [[1]]
    # rank() itself: bits, then position; NaN never enters; -0.0 does not occur (scores are non-negative)
    assert rank(np.array([0.5, np.nan, 0.25, 0.5, 0.25], np.float32), 4) == [2, 4, 0, 3]
    assert rank(np.array([np.nan, np.nan], np.float32), 2) == []


def test_the_search_sets_of_a_registry_of_three_robots():
    w = _world(robot_num=3, this_id=1, num_exclude_recent=1)
    w.add_feature("x", Z, Z)
    for robot in (0, 1, 1, 2, 1, 0, 2, 1, 1):
        w.push("x", robot)
    assert w.keys_of == [[0, 5], [1, 2, 4, 7, 8], [3, 6]]
    # intra: this robot's keyframes [0, cur - num_exclude_recent), LOCAL ids, no minimum size
    assert w.intra_set(4) == [1, 2, 4] and w.intra_set(2) == [1] and w.intra_set(1) == [] and w.intra_set(0) == []
    assert w.query_and_set("intra", 4) == (8, [1, 2, 4], [0, 1, 2])
    # inter: a keyframe of this robot searches every other robot's keys in the registry's concatenation order, unsorted ...
    assert w.inter_set(4) == [0, 5, 3, 6] and w.inter_set(1) == [0, 5, 3, 6]
    assert w.query_and_set("inter", 4) == (4, [0, 5, 3, 6], [0, 5, 3, 6])
    # ... and a received one searches this robot's keys
    assert w.inter_set(0) == [1, 2, 4, 7, 8] and w.inter_set(6) == [1, 2, 4, 7, 8]
    # equal scores everywhere (unmasked zero templates: distance 0): the lists come back in search-set order
    ids, _, dists, found = w.expected("inter", [4, 0], 3)
    assert ids.tolist() == [[0, 5, 3], [1, 2, 4]] and found.tolist() == [3, 3] and not dists.any()
    ids, _, _, found = w.expected("intra", [4, 1, 2], 2)
    assert ids.tolist() == [[0, 1], [-1, -1], [0, -1]] and found.tolist() == [2, 0, 1]
