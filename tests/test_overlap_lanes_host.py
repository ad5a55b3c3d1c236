"""The rule that picks a launch's lane (tinybvh_amd/csrc/overlap_lanes.h; no GPU needed), driven through tbvh_debug_lane_script: a launch whose byte
ranges no launch in flight touches takes the lane the previous launch did not take; one that intersects launches on one lane goes behind them on that
lane; one that intersects launches on both lanes, or whose lane already holds 8 records, joins the lanes and takes lane 0.  Finished launches leave the
lists.  Ranges are half open: [lo, hi)."""
import ctypes as C

import numpy as np

import tinybvh_amd as tb
from tinybvh_amd import _capi

L0, L1, JOIN0 = 0, 1, 2     # out: lane, + 2 when the lanes were joined first


def run(ops):
    a = np.array([list(op) + [0] * (5 - len(op)) for op in ops], np.uint64)
    out = np.zeros(len(ops), np.int32)
    tb.check(_capi.lib.tbvh_debug_lane_script(C.c_void_p(a.ctypes.data), len(ops), C.c_void_p(out.ctypes.data)), "tbvh_debug_lane_script")
    return [int(x) for x in out]


def launch(lo, hi, olo=0, ohi=0):
    return (0, lo, hi, olo, ohi)


def test_disjoint_launches_alternate_and_the_first_takes_lane_0():
    out = run([launch(0, 64), launch(64, 128), launch(128, 192), launch(192, 256)])
    assert out == [L0, L1, L0, L1]


def test_touching_ranges_do_not_conflict_one_shared_byte_does():
    # [0, 64) and [64, 128) touch: independent.  [0, 65) shares byte 64 with [64, 128): behind it, on ITS lane.
    assert run([launch(0, 64), launch(64, 128)]) == [L0, L1]
    assert run([launch(64, 128), launch(0, 65)]) == [L0, L0]
    assert run([launch(1000, 2000), launch(64, 128), launch(0, 65)]) == [L0, L1, L1]
    # the same on the low side: [63, 64) is byte 63 alone
    assert run([launch(0, 64), launch(63, 64)]) == [L0, L0]
    assert run([launch(0, 63), launch(63, 64)]) == [L0, L1]


def test_nested_and_identical_ranges_follow_the_earlier_launch():
    assert run([launch(0, 1024), launch(256, 512)]) == [L0, L0]
    assert run([launch(256, 512), launch(0, 1024)]) == [L0, L0]
    assert run([launch(0, 1024), launch(0, 1024), launch(0, 1024)]) == [L0, L0, L0]
    # ... whichever lane that one took
    assert run([launch(5000, 6000), launch(0, 1024), launch(256, 512), launch(5000, 5001)]) == [L0, L1, L1, L0]


def test_flag_ranges_count_like_ray_ranges():
    # closest-hit and any-hit on the SAME rays conflict through the rays; two any-hit launches on different rays conflict through one occ buffer
    assert run([launch(0, 640), launch(0, 640, 9000, 9010)]) == [L0, L0]
    assert run([launch(0, 640, 9000, 9010), launch(1000, 1640, 9009, 9019)]) == [L0, L0]
    assert run([launch(0, 640, 9000, 9010), launch(1000, 1640, 9010, 9020)]) == [L0, L1]
    # a launch's flags inside another launch's rays
    assert run([launch(0, 640), launch(1000, 1640, 100, 110)]) == [L0, L0]
    # an empty flag range (a closest-hit launch) touches nothing, wherever it points
    assert run([launch(0, 640, 0, 0), launch(1000, 1640, 300, 300)]) == [L0, L1]


def test_a_conflict_with_both_lanes_joins_and_takes_lane_0():
    out = run([launch(0, 64), launch(64, 128), launch(32, 96), launch(200, 264), (3,)])
    assert out[:4] == [L0, L1, JOIN0, L1]
    assert out[4] == 1 + 256 * 1            # the join emptied both lists: the joining launch on lane 0, the next one on lane 1


def shifted(k):
    """launch k of a row of launches that all share bytes, none covering another: [k, 64 + k)"""
    return launch(k, 64 + k)


def test_a_full_list_joins():
    ops = [shifted(k) for k in range(8)]    # 8 launches sharing bytes: all on lane 0, one behind the other
    ops.append((3,))
    ops.append(shifted(8))                  # the ninth finds the list full
    ops.append((3,))
    ops.append(launch(1000, 1064))          # and independent work goes on alternating
    out = run(ops)
    assert out[:8] == [L0] * 8 and out[8] == 8
    assert out[9] == JOIN0 and out[10] == 1
    assert out[11] == L1
    # a full lane 1 likewise: the launch that would go behind its 8 records joins instead
    ops = [launch(1000, 1064)] + [shifted(k) for k in range(8)] + [(3,), shifted(8), (3,)]
    out = run(ops)
    assert out[:9] == [L0] + [L1] * 8 and out[9] == 1 + 256 * 8
    assert out[10] == JOIN0 and out[11] == 1


def test_a_launch_stands_for_the_records_it_covers():
    # a loop over two buffers: however many launches are in flight, one record per buffer, never a join
    ops = []
    for _ in range(20):
        ops += [launch(0, 64), launch(64, 128, 500, 501)]
    out = run(ops + [(3,)])
    assert out[:40] == [L0, L1] * 20 and out[40] == 1 + 256 * 1
    # a launch over the whole buffer replaces the records of its parts; a part does not replace the whole
    out = run([launch(256, 512), launch(0, 256), (3,), launch(0, 1024), (3,), launch(0, 16), (3,)])
    assert out == [L0, L1, 1 + 256, JOIN0, 1, L0, 2]
    # ... and flags count: the same rays with other flags are not covered
    out = run([launch(0, 64, 500, 510), launch(0, 64, 600, 610), (3,), launch(0, 64, 500, 610), (3,)])
    assert out == [L0, L0, 2, L0, 1]


def test_finished_launches_are_pruned():
    # A on lane 0, B on lane 1; a launch on A's buffer follows A — unless A has finished: then nothing holds it and it takes the other lane
    assert run([launch(0, 64), launch(64, 128), launch(0, 64)]) == [L0, L1, L0]
    out = run([launch(0, 64), launch(64, 128), (1, 0), (3,), launch(0, 64)])
    assert out[3] == 0 + 256 * 1 and out[4] == L0         # (lane 0: the lane the previous launch, B, did not take)
    out = run([launch(0, 64), launch(64, 128), (1, 1), (3,), launch(64, 128)])
    assert out[3] == 1 and out[4] == L0                   # B finished: its buffer is free, lane 0 is the other lane
    # pruning keeps the order of what stays: 8 on lane 0, the 2nd and 5th finish, two more fit without a join
    ops = [shifted(k) for k in range(8)] + [(1, 1), (1, 4), shifted(8), shifted(9), (3,), shifted(10)]
    out = run(ops)
    assert out[10] == L0 and out[11] == L0 and out[12] == 8 and out[13] == JOIN0


def test_without_a_second_lane_everything_stays_on_lane_0():
    out = run([(2, 0), launch(0, 64), launch(64, 128), launch(128, 192), (3,)])
    assert out[1:4] == [L0, L0, L0] and out[4] == 3
    # the second lane goes away while it holds a launch: what conflicts with that launch joins, what does not simply takes lane 0
    out = run([launch(0, 64), launch(64, 128), (2, 0), launch(64, 128), launch(300, 364)])
    assert out[3] == JOIN0 and out[4] == L0
    out = run([launch(0, 64), launch(64, 128), (2, 0), launch(300, 364)])
    assert out[3] == L0


def test_bad_scripts_are_refused():
    import pytest
    with pytest.raises(tb.TbvhError):
        run([(9,)])
    with pytest.raises(tb.TbvhError):
        run([(1, 5)])
