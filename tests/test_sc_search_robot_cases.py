"""tests/sc_search_robot_cases.py -- the checker the GPU tests of the per-robot ranked searches compare with -- pinned by hand-written
rows and answers: the rules, the 64-bit bound, a duplicate, an out-of-order pair, an empty set, ties by slot; and the layout's
planted features."""
import numpy as np
import pytest

from sc_search_cases import NO_DIST, assert_lists_equal
from sc_search_robot_cases import (ANY_OTHER_ROBOT, COPIES, COPY_ROBOTS, DUP_AT, NAN_AT, SWAP_AT, TILE2, ZERO_AT, eligible, layout,
                                   ranked_eligible)

INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1

#            slot:  0  1  2  3  4  5  6  7  8  9
ROBOTS = np.int8([0, 1, 0, 2, 1, 0, 0, 1, 2, 0])
INDEXS = np.int32([0, 0, 1, 0, 1, 3, 2, 1, 1, 4])      # robot 0: slots 5 and 6 out of order; robot 1: slots 4 and 7 both index 1


def slots(mask):
    return np.flatnonzero(mask).tolist()


def test_intra_is_the_robots_own_older_keyframes_by_index():
    assert slots(eligible(ROBOTS, INDEXS, 9, "intra", exclude=0)) == [0, 2, 5, 6]          # robot 0, index < 4
    assert slots(eligible(ROBOTS, INDEXS, 9, "intra", exclude=1)) == [0, 2, 6]             # index < 3: slot 6 (index 2) behind slot 5 (index 3)
    assert slots(eligible(ROBOTS, INDEXS, 9, "intra", exclude=2)) == [0, 2]
    assert slots(eligible(ROBOTS, INDEXS, 9, "intra", exclude=4)) == []                    # index < 0: the empty set
    assert slots(eligible(ROBOTS, INDEXS, 6, "intra", exclude=0)) == [0, 2]                # index < 2: slot 5 lies before the query and is out
    assert slots(eligible(ROBOTS, INDEXS, 5, "intra", exclude=0)) == [0, 2, 6]             # index < 3: slot 6 lies BEHIND the query and is in
    assert slots(eligible(ROBOTS, INDEXS, 0, "intra", exclude=0)) == []
    for cur in range(10):                                                                  # exclude >= 0: never the query itself
        assert not eligible(ROBOTS, INDEXS, cur, "intra", exclude=0)[cur]


def test_intra_with_a_duplicate_index():
    assert slots(eligible(ROBOTS, INDEXS, 7, "intra", exclude=0)) == [1]                   # index < 1: the twin at slot 4 is not older
    assert slots(eligible(ROBOTS, INDEXS, 4, "intra", exclude=0)) == [1]
    assert slots(eligible(ROBOTS, INDEXS, 7, "intra", exclude=-1)) == [1, 4, 7]            # index < 2: both of the pair (a negative exclude lists the query)


def test_inter_rules():
    assert slots(eligible(ROBOTS, INDEXS, 9, "inter")) == [1, 3, 4, 7, 8]
    assert slots(eligible(ROBOTS, INDEXS, 9, "inter", robot_pre=ANY_OTHER_ROBOT, exclude=100)) == [1, 3, 4, 7, 8]     # no index rule
    assert slots(eligible(ROBOTS, INDEXS, 9, "inter", robot_pre=1)) == [1, 4, 7]
    assert slots(eligible(ROBOTS, INDEXS, 9, "inter", robot_pre=2)) == [3, 8]
    assert slots(eligible(ROBOTS, INDEXS, 3, "inter", robot_pre=0)) == [0, 2, 5, 6, 9]                                # slots behind the query too
    assert slots(eligible(ROBOTS, INDEXS, 9, "inter", robot_pre=5)) == []                                             # a robot nobody has
    with pytest.raises(AssertionError):
        eligible(ROBOTS, INDEXS, 9, "inter", robot_pre=0)                                                             # the query's own robot
    neg = ROBOTS.copy(); neg[3] = -3                                                                                  # a negative robot id is "another robot"
    assert slots(eligible(neg, INDEXS, 9, "inter")) == [1, 3, 4, 7, 8]
    assert slots(eligible(neg, INDEXS, 3, "inter")) == [0, 1, 2, 4, 5, 6, 7, 8, 9]


def test_the_bound_is_formed_in_64_bits():
    robots = np.int8([0, 0, 0, 0])
    indexs = np.int32([INT_MIN, INT_MIN + 5, INT_MAX - 5, INT_MAX])
    assert slots(eligible(robots, indexs, 1, "intra", exclude=10)) == []                   # INT_MIN + 5 - 10 is below every int32 (wrapped: all)
    assert slots(eligible(robots, indexs, 0, "intra", exclude=1)) == []
    assert slots(eligible(robots, indexs, 1, "intra", exclude=4)) == [0]                   # index < INT_MIN + 1
    assert slots(eligible(robots, indexs, 3, "intra", exclude=0)) == [0, 1, 2]
    assert slots(eligible(robots, indexs, 3, "intra", exclude=-10)) == [0, 1, 2, 3]        # INT_MAX + 10 is above every int32 (wrapped: none)
    assert slots(eligible(robots, indexs, 2, "intra", exclude=INT_MIN)) == [0, 1, 2, 3]
    assert slots(eligible(robots, indexs, 2, "intra", exclude=INT_MAX)) == [0, 1]          # INT_MAX - 5 - INT_MAX = -5


def test_ranked_eligible_is_stable_by_slot_and_skips_the_unlistable():
    d = np.array([0.5, 0.25, 0.25, NO_DIST, np.nan, 0.25, -0.0, 0.0, 0.75, 0.1])
    s = np.arange(10, dtype=np.int32) * 3
    every = np.ones(10, dtype=bool)
    ids, shifts, dists, found = ranked_eligible(d, s, every, 32)
    assert found == 8 and ids[:8].tolist() == [6, 7, 9, 1, 2, 5, 0, 8] and shifts[:8].tolist() == [18, 21, 27, 3, 6, 15, 0, 24]
    assert (ids[8:] == -1).all() and (shifts[8:] == 0).all() and (dists[8:] == NO_DIST).all()
    assert np.signbit(dists[0]) and not np.signbit(dists[1])                               # -0.0 ties with 0.0: the slot decides, the bits stay
    mask = eligible(ROBOTS, INDEXS, 9, "inter", robot_pre=1)                               # slots 1, 4, 7
    assert_lists_equal(ranked_eligible(d, s, mask, 2), (np.int32([7, 1]), np.int32([21, 3]), np.float64([0.0, 0.25]), 2))
    mask = eligible(ROBOTS, INDEXS, 9, "intra")                                            # slots 0, 2, 5, 6: the tie 2 / 5 by slot, slot 1 absent
    assert ranked_eligible(d, s, mask, 3)[0].tolist() == [6, 2, 5]
    mask = eligible(ROBOTS, INDEXS, 9, "inter", robot_pre=2)                               # slots 3 (1e7) and 8
    assert_lists_equal(ranked_eligible(d, s, mask, 2), (np.int32([8, -1]), np.int32([24, 0]), np.float64([0.75, NO_DIST]), 1))
    assert_lists_equal(ranked_eligible(d, s, np.zeros(10, dtype=bool), 1), (np.int32([-1]), np.int32([0]), np.float64([NO_DIST]), 0))


@pytest.mark.parametrize("n", [40, 60, 260, 300])
def test_the_layout_has_what_the_gpu_tests_rely_on(n):
    robots, indexs = layout(n)
    assert robots.dtype == np.int8 and indexs.dtype == np.int32 and set(robots.tolist()) == {0, 1, 2}
    a, b = layout(n)
    assert np.array_equal(a, robots) and np.array_equal(b, indexs)                         # seeded
    for t in range(0, n, 64):                                                              # robots alternate inside every tile but the planted one
        if t != TILE2[0] and n - t >= 16:
            assert len(set(robots[t:t + 64].tolist())) == 3, t
    assert robots[ZERO_AT] == robots[NAN_AT] == 1
    if n > TILE2[1]:
        assert (robots[TILE2[0]:TILE2[1]] == 2).all()
        assert [int(robots[p]) for p in COPIES] == list(COPY_ROBOTS)
    zero, one = np.flatnonzero(robots == 0), np.flatnonzero(robots == 1)
    assert indexs[zero[SWAP_AT]] == SWAP_AT + 1 and indexs[zero[SWAP_AT + 1]] == SWAP_AT   # the pair out of order
    assert indexs[one[DUP_AT]] == indexs[one[DUP_AT - 1]] == DUP_AT - 1                    # the duplicate
    for r, own in ((0, zero), (1, one), (2, np.flatnonzero(robots == 2))):
        plain = np.ones(own.size, dtype=bool)
        if r == 0:
            plain[[SWAP_AT, SWAP_AT + 1]] = False
        if r == 1:
            plain[DUP_AT] = False
        assert np.array_equal(indexs[own][plain], np.arange(own.size)[plain])              # everything else counts up
