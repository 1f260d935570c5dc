"""CPU-only: the lane planner of the host layer (hyteg_amd/host/lanes.hpp) through its C entry hyteg_host_lane_plan.

A step reads and writes whole arrays named by ids.  The planner answers with the lane (an in-order stream) the step is issued
on and the lanes that lane waits for first; a wait on lane j covers everything issued on j so far.  Checked here: every
read-after-write, write-after-write and write-after-read pair is ordered by happens-before (same-lane order plus the waits,
transitively), and the patterns the host layer relies on place themselves as intended.
"""
import ctypes as C

import numpy as np
import pytest

from hyteg_amd import host


def plan(steps, lanes=2):
    """steps: list of (reads, writes) id lists -> (lane of every step, list of waited-for lanes of every step)"""
    rp, wp, rid, wid = [0], [0], [], []
    for r, w in steps:
        rid += list(r)
        wid += list(w)
        rp.append(len(rid))
        wp.append(len(wid))
    n = len(steps)
    lane, waits = (C.c_int * max(1, n))(), (C.c_uint * max(1, n))()
    rc = host.lib().hyteg_host_lane_plan(lanes, n, (C.c_int * len(rp))(*rp), (C.c_ulonglong * max(1, len(rid)))(*rid),
                                         (C.c_int * len(wp))(*wp), (C.c_ulonglong * max(1, len(wid)))(*wid), lane, waits)
    assert rc == 0, host.lib().hyteg_host_last_error().decode()
    return [lane[k] for k in range(n)], [[j for j in range(32) if waits[k] >> j & 1] for k in range(n)]


def check_ordered(steps, lane, waits, lanes):
    """happens-before as vector clocks: clock[j] = number of steps of lane j that the current step is ordered behind"""
    issued = [0] * lanes
    lane_clock = [[0] * lanes for _ in range(lanes)]  # what the NEXT step of a lane is ordered behind
    pos = []
    last_write, reads_since = {}, {}
    for k, (r, w) in enumerate(steps):
        a = lane[k]
        assert 0 <= a < lanes
        assert a not in waits[k]
        for j in waits[k]:
            assert 0 <= j < lanes
            # an event recorded on j now: behind all of j's steps and whatever they are behind
            lane_clock[a] = [max(x, y) for x, y in zip(lane_clock[a], lane_clock[j])]
            lane_clock[a][j] = max(lane_clock[a][j], issued[j])
        clock = list(lane_clock[a])
        clock[a] = issued[a]  # same-lane order
        conflicts = [last_write[x] for x in list(r) + list(w) if x in last_write]
        for x in w:
            conflicts += reads_since.get(x, [])
        for c in conflicts:
            assert clock[lane[c]] >= pos[c], f"step {k} on lane {a} is not ordered behind step {c} on lane {lane[c]}"
        issued[a] += 1
        lane_clock[a] = clock
        lane_clock[a][a] = issued[a]
        pos.append(issued[a])
        for x in r:
            reads_since.setdefault(x, []).append(k)
        for x in w:
            last_write[x] = k
            reads_since[x] = []


@pytest.mark.parametrize("lanes", [1, 2, 3, 4])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_sequences_order_every_conflict(lanes, seed):
    rng = np.random.default_rng(1000 * lanes + seed)
    for narrays in (2, 3, 5, 9, 17):
        ids = [0x7F0000000000 + 4096 * int(i) for i in rng.choice(1 << 20, size=narrays, replace=False)]
        steps = []
        for _ in range(4000):
            nr, nw = int(rng.integers(0, 4)), int(rng.integers(0, 3))
            # drawn with replacement from one pool: a step may read what it writes, and name an array twice
            steps.append(([ids[int(i)] for i in rng.integers(0, narrays, nr)], [ids[int(i)] for i in rng.integers(0, narrays, nw)]))
        lane, waits = plan(steps, lanes)
        check_ordered(steps, lane, waits, lanes)


def ring(npairs, k):
    src = [0x10000 + 0x100 * j for j in range(npairs)]
    dst = [0x20000 + 0x100 * j for j in range(npairs)]
    return [([src[j % npairs]], [dst[j % npairs]]) for j in range(k)]


def test_benchmark_ring_uses_both_lanes_without_waits():
    steps = ring(26, 2000)
    lane, waits = plan(steps, 2)
    check_ordered(steps, lane, waits, 2)
    assert sum(len(w) for w in waits) == 0
    assert abs(lane.count(0) - lane.count(1)) <= 2
    # neighbours in time are on different lanes: they can overlap
    assert sum(lane[k] != lane[k + 1] for k in range(len(lane) - 1)) >= len(lane) - 2


@pytest.mark.parametrize("npairs", [5, 9])
def test_odd_rings_follow_their_history(npairs):
    steps = ring(npairs, 40 * npairs)
    lane, waits = plan(steps, 2)
    check_ordered(steps, lane, waits, 2)
    assert sum(len(w) for w in waits[npairs:]) == 0
    assert sum(len(w) for w in waits) == 0  # the first pass is independent as well
    for k in range(npairs, len(steps)):
        assert lane[k] == lane[k - npairs]
    assert min(lane.count(0), lane.count(1)) >= len(lane) // 2 - len(lane) // npairs


def test_ping_pong_chain_stays_on_one_lane():
    a, b = 0xA000, 0xB000
    steps = [([a], [b]) if k % 2 == 0 else ([b], [a]) for k in range(500)]
    for lanes in (2, 3):
        lane, waits = plan(steps, lanes)
        check_ordered(steps, lane, waits, lanes)
        assert len(set(lane)) == 1
        assert sum(len(w) for w in waits) == 0


def test_one_lane_is_the_input_order():
    rng = np.random.default_rng(7)
    steps = [([int(x) for x in rng.integers(1, 6, 2)], [int(rng.integers(1, 6))]) for _ in range(300)]
    lane, waits = plan(steps, 1)
    assert lane == [0] * len(steps)
    assert all(w == [] for w in waits)


def test_fan_out_and_fan_in():
    src, dsts = 1, [10, 11, 12, 13]
    steps = [([src], [d]) for d in dsts]  # one source into several destinations: independent
    lane, waits = plan(steps, 2)
    assert sum(len(w) for w in waits) == 0 and lane == [0, 1, 0, 1]
    steps = [([s], [99]) for s in (1, 2, 3, 4)]  # several sources into one destination: the writes keep their order
    lane, waits = plan(steps, 2)
    check_ordered(steps, lane, waits, 2)
    assert len(set(lane)) == 1 and sum(len(w) for w in waits) == 0


def test_bad_lane_count_is_an_error():
    out, w = (C.c_int * 1)(), (C.c_uint * 1)()
    z = (C.c_int * 1)(0)
    ids = (C.c_ulonglong * 1)()
    assert host.lib().hyteg_host_lane_plan(0, 0, z, ids, z, ids, out, w) != 0
    assert host.lib().hyteg_host_lane_plan(9, 0, z, ids, z, ids, out, w) != 0
