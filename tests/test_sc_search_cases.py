"""tests/sc_search_cases.py `ranked` -- the checker the GPU tests of the ranked search compare with -- pinned by hand-written rows
and answers (no GPU)."""
import numpy as np

from sc_search_cases import NO_DIST, ranked, assert_lists_equal


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def test_three_equal_distances_across_the_tile_border_keep_their_order():
    d = np.full(70, 0.5); d[[62, 63, 64]] = 0.25; d[5] = 0.375
    s = np.arange(70, dtype=np.int32) % 60
    ids, shifts, dists, found = ranked(d, s, 0, 70, 4)
    assert ids.tolist() == [62, 63, 64, 5] and shifts.tolist() == [2, 3, 4, 5] and dists.tolist() == [0.25, 0.25, 0.25, 0.375] and found == 4
    ids, _, _, found = ranked(d, s, 0, 70, 2)
    assert ids.tolist() == [62, 63] and found == 2
    ids, _, _, _ = ranked(d, s, 63, 70, 3)                               # the range starts inside the tie
    assert ids.tolist() == [63, 64, 65]


def test_an_unscored_and_a_nan_entry_are_never_listed():
    d = np.array([0.3, NO_DIST, 0.1, np.nan, 0.2]); s = np.array([7, 0, 9, 3, 11], dtype=np.int32)
    ids, shifts, dists, found = ranked(d, s, 0, 5, 5)
    assert found == 3 and ids.tolist() == [2, 4, 0, -1, -1] and shifts.tolist() == [9, 11, 7, 0, 0]
    assert np.array_equal(bits(dists), bits([0.1, 0.2, 0.3, NO_DIST, NO_DIST]))
    assert ranked(d, s, 0, 5, 1)[0].tolist() == [2]
    ids, _, _, found = ranked(np.array([np.inf, np.nan, 2e7, NO_DIST]), np.zeros(4, dtype=np.int32), 0, 4, 2)
    assert found == 0 and ids.tolist() == [-1, -1]


def test_order_is_by_value_not_by_bit_pattern():
    d = np.array([0.0, -0.0, -1.5, 0.0, 1e-300]); s = np.array([1, 2, 3, 4, 5], dtype=np.int32)
    ids, shifts, dists, found = ranked(d, s, 0, 5, 5)
    assert found == 5 and ids.tolist() == [2, 0, 1, 3, 4] and shifts.tolist() == [3, 1, 2, 4, 5]
    assert np.array_equal(bits(dists), bits([-1.5, 0.0, -0.0, 0.0, 1e-300]))   # every distance keeps its own bits, the sign of -0.0 too


def test_k_larger_than_the_row_and_the_fillers():
    ids, shifts, dists, found = ranked([0.2, 0.1], [4, 6], 0, 2, 4)
    assert found == 2 and ids.tolist() == [1, 0, -1, -1] and shifts.tolist() == [6, 4, 0, 0]
    assert np.array_equal(bits(dists), bits([0.1, 0.2, NO_DIST, NO_DIST]))
    assert ids.dtype == np.int32 and shifts.dtype == np.int32 and dists.dtype == np.float64


def test_empty_range_and_sub_range():
    d = np.array([0.5, 0.4, 0.3, 0.2, 0.1]); s = np.arange(5, dtype=np.int32)
    for lo, hi in ((0, 0), (3, 3), (5, 5)):
        ids, shifts, dists, found = ranked(d, s, lo, hi, 3)
        assert found == 0 and ids.tolist() == [-1] * 3 and shifts.tolist() == [0] * 3 and dists.tolist() == [NO_DIST] * 3
    ids, shifts, _, found = ranked(d, s, 1, 4, 2)
    assert found == 2 and ids.tolist() == [3, 2] and shifts.tolist() == [3, 2]
    # a row that starts at keyframe 10: ids are keyframes, not positions
    ids, _, _, found = ranked(d, s, 11, 14, 5, base=10)
    assert found == 3 and ids.tolist() == [13, 12, 11, -1, -1]
    assert_lists_equal(ranked(d, s, 1, 4, 2), ranked(d, s, 1, 4, 2))
