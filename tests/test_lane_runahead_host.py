"""When a launch may START beside the other lane's launches, and when a probed launch may leave out its coherent flavor (tinybvh_amd/csrc/overlap_lanes.h:
LaneBook::gate; probe_memory.h; no GPU needed), driven through tbvh_debug_runahead_script.

The start rule.  Depth 1: a launch waits for the start of the other lane's latest launch while that lane holds anything in flight.  Depth 2: for the start of
the other lane's launch BEFORE its latest one, and only while that launch is in flight; with fewer than two launches of the other lane in flight it waits for
nothing.  A join empties the history.  The expected answers come from a model of these sentences kept here, over the lanes the script itself reports (the
lane choice has its own tests: test_overlap_lanes_host.py).

The verdict memory.  A launch goes solo only when the last two FINISHED launches of exactly its footprint (ray range, closest or any hit, scene) both voted
incoherent; the table holds eight footprints and gives up the one that has gone longest without a verdict."""
import ctypes as C

import numpy as np
import pytest

import tinybvh_amd as tb
from tinybvh_amd import _capi

A, B, CBUF = (0, 1000), (1000, 2000), (2000, 3000)
INCOHERENT, COHERENT = 1, 2


def run(ops, depth):
    a = np.array([list(op) + [0] * (6 - len(op)) for op in ops], np.uint64)
    out = np.zeros((len(ops), 2), np.int64)
    tb.check(_capi.lib.tbvh_debug_runahead_script(C.c_void_p(a.ctypes.data), len(ops), depth, C.c_void_p(out.ctypes.data)), "tbvh_debug_runahead_script")
    return [(int(x), int(y)) for x, y in out]


def launch(buf, occ=(0, 0)):
    return (0, buf[0], buf[1], occ[0], occ[1])


def finish(row):
    return (1, row)


JOIN = (4,)


def expected_gates(ops, out, depth):
    """the rule's sentences, over the lanes the script reported: {row: row waited for or -1}"""
    recent = {0: [], 1: []}     # rows launched on each lane since the last join
    done = set()
    want = {}
    for i, (op, (code, _)) in enumerate(zip(ops, out)):
        if op[0] == 1:
            done.add(op[1])
        elif op[0] == 4:
            recent = {0: [], 1: []}
        elif op[0] == 0:
            lane = code & 1
            if code & 2:
                recent = {0: [], 1: []}
            other = recent[lane ^ 1]
            if depth == 1:
                want[i] = other[-1] if any(r not in done for r in other) else -1
            else:
                want[i] = other[-2] if len(other) >= 2 and other[-2] not in done else -1
            recent[lane].append(i)
    return want


def check(ops, depth):
    out = run(ops, depth)
    want = expected_gates(ops, out, depth)
    got = {i: out[i][1] for i in want}
    assert got == want, (depth, got, want)
    done_before = set()
    for i, op in enumerate(ops):                 # a finished launch is never named, nor a later one, nor one of the launch's own lane
        if op[0] == 1:
            done_before.add(op[1])
        if op[0] == 0 and out[i][1] >= 0:
            g = out[i][1]
            assert g < i and ops[g][0] == 0 and (out[g][0] & 1) != (out[i][0] & 1)
            if depth == 2:
                assert g not in done_before
    return out


def test_the_bench_pattern_two_buffers_alternated_20_pairs():
    ops = [launch(A), launch(B)] * 20
    for depth in (1, 2):
        out = check(ops, depth)
        assert [c for c, _ in out] == [0, 1] * 20                                   # camera buffer on lane 0, bounce buffer on lane 1, no join
    d1 = [g for _, g in run(ops, 1)]
    d2 = [g for _, g in run(ops, 2)]
    assert d1 == [-1] + list(range(0, 39))                                          # depth 1: launch i waits for the other lane's latest, launch i - 1
    assert d2 == [-1, -1, -1] + list(range(0, 37))                                  # depth 2: for the one before that, launch i - 3: C(k+2) for D(k)


def test_no_wait_when_the_other_lane_has_fewer_than_two_launches_in_flight():
    # the same pattern, the device keeping up: before launch i everything up to launch i - 3 has finished (i - 1 and i - 2 are in flight)
    ops, rows = [], []
    for i in range(40):
        if len(rows) >= 3:
            ops.append(finish(rows[-3]))
        rows.append(len(ops))
        ops.append(launch(A if i % 2 == 0 else B))
    out = check(ops, 2)
    assert all(out[r][1] == -1 for r in rows)
    out = check(ops, 1)                                                             # depth 1 still orders the starts: the other lane's latest is in flight
    assert [out[r][1] for r in rows[1:]] == rows[:-1]
    # one launch later: launch i - 3 is still in flight and is the one named
    ops, rows = [], []
    for i in range(40):
        if len(rows) >= 4:
            ops.append(finish(rows[-4]))
        rows.append(len(ops))
        ops.append(launch(A if i % 2 == 0 else B))
    out = check(ops, 2)
    assert [out[r][1] for r in rows[3:]] == rows[:-3]


def test_a_finished_launch_is_never_named():
    # everything finished before each launch: no launch waits at either depth
    ops, rows = [], []
    for i in range(12):
        ops += [finish(r) for r in rows[-1:]]
        rows.append(len(ops))
        ops.append(launch(A if i % 2 == 0 else B))
    for depth in (1, 2):
        out = check(ops, depth)
        assert all(out[r][1] == -1 for r in rows)


@pytest.mark.parametrize("depth", [1, 2])
def test_after_a_join_nothing_is_waited_for(depth):
    ops = [launch(A), launch(B)] * 3 + [JOIN, launch(A), launch(B), launch(A), launch(B)]
    out = check(ops, depth)
    assert out[7][1] == -1                                                          # the first launch after the join
    if depth == 2:
        assert out[8][1] == -1 and out[9][1] == -1                                  # one launch on the other lane since the join: nothing to name yet
        assert out[10][1] == 7
    else:
        assert out[8][1] == 7
    # a launch that conflicts with launches on both lanes joins them itself and names nothing either
    ops = [launch(A), launch(B)] * 3 + [launch((500, 1500)), launch(CBUF)]
    out = check(ops, depth)
    assert out[6] == (2, -1)
    assert out[7][1] == (6 if depth == 1 else -1)


@pytest.mark.parametrize("depth", [1, 2])
def test_three_buffers_in_rotation(depth):
    ops = [launch(A), launch(B), launch(CBUF)] * 8
    out = check(ops, depth)
    lanes = [c for c, _ in out]
    assert lanes[:3] == [0, 1, 0] and lanes[3:] == [0, 1, 0] * 7                    # A and C follow their own earlier launches on lane 0, B on lane 1
    if depth == 2:
        assert out[4][1] == 2 and out[5][1] == 1 and out[7][1] == 5               # B2: lane 0 took A1 C1 A2, the one before its latest is C1; C2: lane 1 took B1 B2; B3: C2
    # ... and with the device keeping up nothing of it is left
    ops, rows = [], []
    for i in range(24):
        ops += [finish(r) for r in rows[-3:-2]]
        rows.append(len(ops))
        ops.append(launch((A, B, CBUF)[i % 3]))
    check(ops, depth)


def test_depth_is_checked():
    a = np.zeros((1, 6), np.uint64)
    out = np.zeros((1, 2), np.int64)
    for depth in (0, 3):
        assert _capi.lib.tbvh_debug_runahead_script(C.c_void_p(a.ctypes.data), 1, depth, C.c_void_p(out.ctypes.data)) != 0


# ---- the verdict memory ------------------------------------------------------------------------------------------------------------------------------------

def probed(buf, scene=7, any_hit=0, lane=0):
    return (5, buf[0], buf[1], scene, any_hit, lane)


def said(row, verdict):
    return (6, row, verdict)


def solo_of(ops):
    out = run(ops, 2)
    return [out[i][0] for i, op in enumerate(ops) if op[0] == 5]


def voted(ops, buf, verdict, **kw):
    """a probed launch on buf that finishes with that verdict; returns its row"""
    row = len(ops)
    ops += [probed(buf, **kw), said(row, verdict), finish(row)]
    return row


def test_two_incoherent_votes_are_needed_before_a_launch_goes_solo():
    ops = []
    voted(ops, B, INCOHERENT)
    voted(ops, B, INCOHERENT)
    voted(ops, B, INCOHERENT)
    ops.append(probed(B))
    assert solo_of(ops) == [0, 0, 1, 1]                                             # nothing known; one vote; two votes; still two


def test_one_coherent_vote_goes_back_to_two_flavors():
    ops = []
    voted(ops, B, INCOHERENT); voted(ops, B, INCOHERENT)
    voted(ops, B, COHERENT)                                                         # launched solo, and its own sample says coherent
    voted(ops, B, INCOHERENT)                                                       # two flavors: last two are (coherent, incoherent)
    voted(ops, B, INCOHERENT)                                                       # two flavors: (incoherent, coherent)
    ops.append(probed(B))                                                           # (incoherent, incoherent)
    assert solo_of(ops) == [0, 0, 1, 0, 0, 1]
    ops = []
    voted(ops, A, COHERENT); voted(ops, A, COHERENT); ops.append(probed(A))         # a coherent buffer never goes solo
    assert solo_of(ops) == [0, 0, 0]
    ops = []
    voted(ops, B, INCOHERENT); voted(ops, B, 0); voted(ops, B, 0); ops.append(probed(B))   # a launch whose probe published nothing is no evidence
    assert solo_of(ops) == [0, 0, 0, 0]


def test_evidence_from_an_unfinished_launch_is_not_used():
    ops = [probed(B), said(0, INCOHERENT), probed(B), said(2, INCOHERENT)]          # two launches in flight, their verdicts already in their slots
    ops += [probed(B)]                                                              # 4: nothing has finished
    ops += [finish(0), probed(B)]                                                   # 6: one finished
    ops += [finish(2), probed(B)]                                                   # 8: both
    assert solo_of(ops) == [0, 0, 0, 0, 1]
    # the two lanes finish independently: a launch on lane 1 is harvested while an older one on lane 0 is still in flight
    ops = [probed(A, lane=0), said(0, COHERENT), probed(B, lane=1), said(2, INCOHERENT), finish(2), probed(B, lane=1), said(5, INCOHERENT), finish(5), probed(B, lane=1)]
    assert solo_of(ops) == [0, 0, 0, 1]


def test_footprints_that_only_overlap_do_not_match():
    ops = []
    voted(ops, B, INCOHERENT); voted(ops, B, INCOHERENT)
    ops += [probed((B[0], B[1] - 64)), probed((B[0] + 64, B[1])), probed((B[0], B[1] + 64)), probed((B[0] - 64, B[1] + 64)),
            probed(B, scene=8), probed(B, any_hit=1), probed(B)]
    assert solo_of(ops) == [0, 0, 0, 0, 0, 0, 0, 0, 1]


def test_the_table_evicts_its_oldest_entry():
    bufs = [(i * 1000, i * 1000 + 1000) for i in range(9)]
    ops = []
    for b in bufs[:8]:
        voted(ops, b, INCOHERENT); voted(ops, b, INCOHERENT)
    assert solo_of(ops + [probed(b) for b in bufs[:8]]) == [0, 0] * 8 + [1] * 8    # eight footprints fit
    voted(ops, bufs[0], INCOHERENT)                                                 # footprint 0 is now the most recent one, footprint 1 the oldest
    voted(ops, bufs[8], INCOHERENT); voted(ops, bufs[8], INCOHERENT)                # a ninth
    got = solo_of(ops + [probed(b) for b in bufs])
    assert got[-9:] == [1, 0, 1, 1, 1, 1, 1, 1, 1]
