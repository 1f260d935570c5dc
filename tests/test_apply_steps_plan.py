"""CPU-only: the grouping of a run of applies for the steps launch (planApplySteps in hyteg_amd/host/lanes.hpp) through its C
entry hyteg_host_apply_steps_plan.

Step k of a cycle over a ring of pairs reads src[(first + k) % n] and writes dst[(first + k) % n]; consecutive steps share a
launch while none of them writes an array another one reads or writes.  With one lane the groups are the maximal ones of up to
G steps.  With several lanes a group takes 1 / lanes of the conflict-free steps ahead of it (and the next lanes - 1 groups as
many), so that every lane still gets a launch (and a short ring keeps alternating between the lanes as it did without groups).
"""
import ctypes as C

import pytest

from hyteg_amd import host


def plan(srcs, dsts, first, steps, G, lanes=1, expect_rc=0):
    n = len(srcs)
    sizes, ngroups = (C.c_int * max(1, steps))(), C.c_int(-1)
    rc = host.lib().hyteg_host_apply_steps_plan(n, (C.c_ulonglong * max(1, n))(*srcs), (C.c_ulonglong * max(1, n))(*dsts), first, steps,
                                                G, lanes, sizes, C.byref(ngroups))
    if expect_rc:
        assert rc != 0
        return None
    assert rc == 0, host.lib().hyteg_host_last_error().decode()
    out = [sizes[k] for k in range(ngroups.value)]
    assert sum(out) == steps and all(1 <= g <= G for g in out)
    return out


def check_independent(srcs, dsts, first, sizes):
    """no step of a group writes what another step of the group reads or writes"""
    n, k = len(srcs), 0
    for g in sizes:
        idx = [(first + k + i) % n for i in range(g)]
        w = [dsts[j] for j in idx]
        assert len(set(w)) == len(w)
        assert not set(w) & {srcs[j] for j in idx}
        k += g


def ring(n):
    return [1000 + 2 * k for k in range(n)], [1001 + 2 * k for k in range(n)]


def test_ring_of_26_pairs_gives_groups_of_8():
    s, d = ring(26)
    assert plan(s, d, 0, 26, 8) == [8, 8, 8, 2]
    # the wrap-around of first + k: a group runs across the end of the ring, and ends only where a pair would repeat
    assert plan(s, d, 20, 26, 8) == [8, 8, 8, 2]
    assert plan(s, d, 0, 52, 8) == [8] * 6 + [4]
    assert plan(s, d, 25, 60, 16) == [16, 16, 16, 12]
    for first, steps, G in ((0, 26, 8), (20, 26, 8), (0, 52, 8), (25, 60, 16), (7, 100, 16)):
        check_independent(s, d, first, plan(s, d, first, steps, G))
    # a group never holds a pair twice: G = 16 on a ring of 10
    s, d = ring(10)
    assert plan(s, d, 3, 35, 16) == [10, 10, 10, 5]


def test_one_pair_repeated_is_single_launches():
    assert plan([5], [6], 0, 9, 8) == [1] * 9
    assert plan([5], [6], 0, 9, 8, lanes=2) == [1] * 9


def test_dependent_chain_is_single_launches():
    # dst[k] == src[k+1]
    s = [10 + k for k in range(12)]
    d = [11 + k for k in range(12)]
    assert plan(s, d, 0, 12, 8) == [1] * 12
    assert plan(s, d, 4, 7, 16) == [1] * 7
    # one dependency in an otherwise independent ring: the reader starts a new group
    s, d = ring(8)
    s[5] = d[4]
    assert plan(s, d, 0, 8, 8) == [5, 3]
    # a step that writes what an earlier step of the group reads
    s, d = ring(6)
    d[3] = s[1]
    assert plan(s, d, 0, 6, 8) == [3, 3]
    # shared sources do not conflict (one source into several destinations)
    assert plan([7, 7, 7, 7], [1, 2, 3, 4], 0, 4, 8) == [4]
    # several sources into one destination do
    assert plan([1, 2, 3], [9, 9, 9], 0, 3, 8) == [1, 1, 1]


def test_ring_of_3_pairs_ends_groups_where_a_pair_would_repeat():
    s, d = ring(3)
    assert plan(s, d, 0, 11, 8) == [3, 3, 3, 2]
    assert plan(s, d, 2, 7, 8) == [3, 3, 1]


def test_group_size_1_is_the_identity():
    s, d = ring(26)
    assert plan(s, d, 3, 40, 1) == [1] * 40
    assert plan(s, d, 3, 40, 1, lanes=2) == [1] * 40


def test_fewer_steps_than_the_group_size():
    s, d = ring(26)
    assert plan(s, d, 0, 5, 8) == [5]
    assert plan(s, d, 24, 3, 16) == [3]
    assert plan(s, d, 0, 1, 8) == [1]
    assert plan(s, d, 0, 0, 8) == []


def test_several_lanes_leave_every_lane_a_launch():
    s, d = ring(26)
    # enough independent steps ahead: full groups, also across the end of the ring (26 = 13 per lane >= 8)
    assert plan(s, d, 0, 48, 8, lanes=2) == [8] * 6
    assert plan(s, d, 0, 64, 16, lanes=2)[:3] == [13, 13, 13]
    # a short ring is not swallowed by one launch: 3 pairs on 2 or 3 lanes stay single launches, 5 pairs on 2 lanes pair up
    s3, d3 = ring(3)
    assert plan(s3, d3, 0, 17, 8, lanes=2) == [1] * 17
    assert plan(s3, d3, 0, 17, 8, lanes=3) == [1] * 17
    s5, d5 = ring(5)
    assert plan(s5, d5, 0, 20, 16, lanes=2) == [2] * 10
    # a split gives the lanes equal shares: 20 steps are two launches of 10; what is left at the end of a run is split again
    assert plan(s, d, 0, 20, 16, lanes=2) == [10, 10]
    assert plan(s, d, 0, 20, 8, lanes=2) == [8, 8, 2, 2]
    assert plan(s, d, 0, 30, 16, lanes=2) == [13, 13, 2, 2]
    for lanes in (2, 3):
        for first, steps, G in ((0, 26, 8), (20, 77, 16), (5, 9, 4)):
            check_independent(s, d, first, plan(s, d, first, steps, G, lanes))


def test_bad_arguments_are_errors():
    s, d = ring(4)
    plan(s, d, 0, 4, 0, expect_rc=1)
    plan(s, d, 0, 4, 8, lanes=0, expect_rc=1)
    plan(s, d, -1, 4, 8, expect_rc=1)
    plan(s, d, 0, -1, 8, expect_rc=1)
