"""Two-deep run-ahead between a context's launch lanes, and incoherent batches launched as one kernel (tinybvh_amd/csrc/overlap_lanes.h: LaneBook::gate,
probe_memory.h, capi_query.hip: launchQuery).  As in test_overlap_gpu.py a caller must see no difference but in time: every case runs the same calls with
overlap off and with overlap on at depth 2 and compares what it reads back byte for byte; the serial run is checked against the oracle.

The solo flavor needs a probed two-flavor launch: a scene just over 48 MiB (the smallest street stand-in of that class) and 2 M rays.  There the same calls run
with the verdict memory off and on, again byte for byte, and the debug counter says which launches left the coherent flavor out."""
import os
import time

import numpy as np
import pytest

import tinybvh_amd as tb
from tinybvh_amd import rays as R
from tinybvh_amd import scenes
from oracle_lib import compare_hits

pytestmark = pytest.mark.gpu

MODES = ["uploaded", "hybrid90"]
DEFAULT_ON = os.environ.get("TBVH_OVERLAP", "1") != "0"
DEFAULT_DEPTH = int(os.environ.get("TBVH_OVERLAP_DEPTH", "1"))
DEFAULT_MEMORY = os.environ.get("TBVH_PROBE_MEMORY", "1") != "0"


class World:
    pass


@pytest.fixture(scope="module")
def world(ctx, oracle_ties):
    w = World()
    w.verts = scenes.atrium(20_000, seed=7)
    w.host_scene = {}
    for mode in MODES:
        sc = tb.BVH8_CWBVH(ctx).Build(w.verts)
        if mode == "hybrid90":
            sc.set_hybrid(1024)
            sc.set_variant(90)
        w.host_scene[mode] = sc
    h = w.host_scene["uploaded"].host
    w.cam = R.primary(R.camera(*scenes.SPONZA_CAMERAS[0], 256, 256, 1, 1))                    # 65536 camera rays
    w.want_cam = oracle_ties.bvh2_intersect(h.bvh2_nodes(), h.bvh2_prim_idx(), w.verts, w.cam)
    w.bounce = R.bounce(w.want_cam, w.verts, seed=9)                                          # 65536 diffuse rays
    w.want_bounce = oracle_ties.bvh2_intersect(h.bvh2_nodes(), h.bvh2_prim_idx(), w.verts, w.bounce)
    w.n = w.cam.shape[0]
    w.big = np.concatenate([w.cam, w.bounce, w.cam, w.bounce])                                # 262144 rays for the timing case
    w.d = [ctx.malloc(w.n * 64) for _ in range(4)]
    w.d_big = [ctx.malloc(w.big.shape[0] * 64) for _ in range(2)]
    w.d_occ = ctx.malloc(w.n)
    w.d_verts = ctx.malloc(w.verts.nbytes)
    ctx.to_device(w.d_verts, w.verts)
    yield w
    for p in w.d + w.d_big + [w.d_occ, w.d_verts]:
        ctx.free(p)
    for sc in w.host_scene.values():
        sc.free()
    ctx.set_overlap(DEFAULT_ON)
    ctx.set_overlap_depth(DEFAULT_DEPTH)


def read(ctx, dptr, n):
    out = np.zeros(n, dtype=tb.RAY_DTYPE)
    ctx.from_device(out, dptr)
    return out


def read_occ(ctx, dptr, n):
    out = np.zeros(n, np.uint8)
    ctx.from_device(out, dptr)
    return out


def serial_and_depth2(ctx, fn):
    """fn() run with overlap off, then on at depth 2: (what each returned, lane-1 launches of the second run)"""
    try:
        ctx.set_overlap(False)
        s0 = ctx.overlap_stats()
        serial = fn()
        assert ctx.overlap_stats()[0] == s0[0]                 # off: nothing takes the second lane
        ctx.set_overlap(True)
        ctx.set_overlap_depth(2)
        s1 = ctx.overlap_stats()
        over = fn()
        return serial, over, ctx.overlap_stats()[0] - s1[0]
    finally:
        ctx.set_overlap(DEFAULT_ON)
        ctx.set_overlap_depth(DEFAULT_DEPTH)


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) for x, y in zip(a, b))


def exact(got, want):
    c = compare_hits(got, want)
    assert c["hits"] > 1000 and c["hitmiss"] == 0 and c["prim_real"] == 0 and c["t_bad"] == 0 and c["uv_bad"] == 0, c
    assert c["tie"] == 0 and c["onsurf"] <= max(4, c["n"] // 5000), c
    assert c["bit_identical"] == c["same_prim"], c


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nbuf", [2, 3])
def test_buffers_alternated_10_times(ctx, world, mode, nbuf):
    w, sc, n = world, world.host_scene[mode], world.n
    src = [w.cam, w.bounce, w.cam][:nbuf]
    want = [w.want_cam, w.want_bounce, w.want_cam][:nbuf]

    def fn():
        for d, a in zip(w.d, src):
            ctx.to_device(d, a)
        for _ in range(10):
            for d in w.d[:nbuf]:
                sc.intersect_device_fresh(d, n, 1e30)
        return tuple(read(ctx, d, n) for d in w.d[:nbuf])      # (no synchronize: from_device right after the last launches)

    serial, over, lane1 = serial_and_depth2(ctx, fn)
    for got, ser in zip(over, serial):
        assert not ((got["t"] >= 1e30) & (ser["t"] < 1e30)).any()            # no record left armed where the serial run has a hit
    assert same(serial, over)
    assert lane1 >= 10                                           # two buffers: every second launch; three: the buffer that lives on the second lane
    for got, wnt in zip(serial, want):
        exact(got, wnt)


@pytest.mark.parametrize("mode", MODES)
def test_a_generator_reads_a_buffer_whose_launch_is_two_ahead(ctx, world, mode):
    w, sc, n = world, world.host_scene[mode], world.n
    d_a, d_b, d_c = w.d[:3]

    def fn():
        ctx.to_device(d_a, w.cam); ctx.to_device(d_b, w.bounce)
        sc.intersect_device_fresh(d_b, n, 1e30)                  # lane 0
        sc.intersect_device_fresh(d_a, n, 34.0)                  # lane 1: near hits only ...
        sc.intersect_device_fresh(d_b, n, 1e30)                  # lane 0
        sc.intersect_device_fresh(d_a, n, 1e30)                  # lane 1, behind the near launch: may start two launches ahead of lane 0's first
        ctx.generate_bounce(w.d_verts, d_a, d_c, n, 77)          # reads the hits of that last launch, every one of them
        sc.intersect_device_fresh(d_c, n, 1e30)
        return read(ctx, d_c, n), read(ctx, d_a, n)

    serial, over, lane1 = serial_and_depth2(ctx, fn)
    assert same(serial, over) and lane1 >= 2
    assert int((serial[0]["t"] < 1e30).sum()) > 1000
    exact(serial[1], w.want_cam)


@pytest.mark.parametrize("mode", MODES)
def test_any_hit_launches_sharing_a_flag_buffer(ctx, world, mode):
    w, sc, n = world, world.host_scene[mode], world.n
    d_a, d_b, d_c = w.d[:3]

    def fn():
        ctx.to_device(d_a, w.cam); ctx.to_device(d_b, w.bounce); ctx.to_device(d_c, w.cam)
        ctx.to_device(w.d_occ, np.full(n, 7, np.uint8))
        sc.intersect_device_fresh(d_c, n, 1e30)                  # a closest-hit launch beside them
        sc.occluded_device(d_a, n, w.d_occ)                      # three any-hit launches on different rays, ONE flag buffer: they keep their order,
        sc.occluded_device(d_b, n, w.d_occ)
        sc.intersect_device_fresh(d_c, n, 1e30)
        sc.occluded_device(d_a, n, w.d_occ)
        sc.occluded_device(d_b, n, w.d_occ)                      # ... the last one's flags stay
        return read_occ(ctx, w.d_occ, n), read(ctx, d_c, n)

    serial, over, _ = serial_and_depth2(ctx, fn)
    assert same(serial, over)
    assert np.array_equal(serial[0].astype(bool), w.want_bounce["t"] < 1e30)
    assert not np.array_equal(serial[0].astype(bool), w.want_cam["t"] < 1e30)
    exact(serial[1], w.want_cam)


@pytest.mark.parametrize("mode", MODES)
def test_reported_times_are_positive_and_sum_to_at_most_the_wall_time(ctx, world, mode):
    """tbvh_time_history at depth 2: each launch reports the time it added, so ten alternated launches still sum to at most the loop's wall time.  The margin
    is what the same comparison needs with overlap off on this box (event time stamps against the host clock)."""
    w, sc = world, world.host_scene[mode]
    nb = w.big.shape[0]
    for d in w.d_big:
        ctx.to_device(d, w.big)

    def fn():
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(5):
            sc.intersect_device_fresh(w.d_big[0], nb, 1e30)
            sc.intersect_device_fresh(w.d_big[1], nb, 1e30)
        ctx.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        return (np.array(ctx.time_history(10), np.float64), np.float64(wall))

    fn()                                                         # (first launches of this size: not timed)
    serial, over, lane1 = serial_and_depth2(ctx, fn)
    margin = max(0.0, float(serial[0].sum() - serial[1]))
    print(f"[{mode}] serial: sum {serial[0].sum():.4f} ms of wall {serial[1]:.4f} ms {np.round(serial[0], 4)}; depth 2: sum {over[0].sum():.4f} ms of wall {over[1]:.4f} ms {np.round(over[0], 4)}; margin {margin:.4f} ms")
    assert lane1 >= 5
    assert len(serial[0]) == 10 and (serial[0] > 0).all()
    assert len(over[0]) == 10 and (over[0] > 0).all(), over[0]
    assert over[0].sum() <= over[1] + margin, (over, margin)


# ---- the solo flavor ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def street(ctx):
    w = World()
    w.verts = scenes.street(595_000, seed=2)
    w.sc = tb.BVH8_CWBVH(ctx).Build(w.verts)
    blob_bytes = w.sc.host.blob(0, np.uint32, 4).nbytes + w.sc.host.blob(1, np.uint32, 4).nbytes
    assert (48 << 20) < blob_bytes <= (49 << 20), blob_bytes      # just inside the class whose batches of 2 M rays and more are two-flavor launches
    hint = w.sc.schedule_hint()
    hint["closest_hit"] = [1, 1, 1]                                # (the schedule of coherent batches pinned: a tuner still measuring keeps every launch two-flavor)
    w.sc.set_schedule_hint(hint)
    w.n = 1 << 21
    cam = R.camera(*scenes.STREET_CAMERAS[0], 2048, 1024, 1, 1)
    w.d_cam, w.d_bounce, w.d_work = ctx.malloc(w.n * 64), ctx.malloc(w.n * 64), ctx.malloc(w.n * 64)
    w.d_verts = ctx.malloc(w.verts.nbytes)
    ctx.to_device(w.d_verts, w.verts)
    ctx.set_probe_memory(False)
    ctx.generate_primary(cam, w.d_cam, 0, w.n)
    w.cam = read(ctx, w.d_cam, w.n)                                # camera rays, armed
    ctx.to_device(w.d_work, w.cam)
    w.sc.intersect_device(w.d_work, w.n)
    assert ctx.last_probe()[2] == 2
    ctx.generate_bounce(w.d_verts, w.d_work, w.d_bounce, w.n, 4711)
    w.bounce = read(ctx, w.d_bounce, w.n)                          # their diffuse bounces, armed
    ctx.set_probe_memory(DEFAULT_MEMORY)
    yield w
    for p in (w.d_cam, w.d_bounce, w.d_work, w.d_verts):
        ctx.free(p)
    w.sc.free()
    ctx.set_probe_memory(DEFAULT_MEMORY)


def memory_off_and_on(ctx, fn):
    """fn() with the verdict memory off, then on (forgetting what was learnt before): (what each returned, solo launches of each run)"""
    try:
        out, solos = [], []
        for on in (False, True):
            ctx.set_probe_memory(on)
            s0 = ctx.probe_memory_stats()[0]
            out.append(fn())
            solos.append(ctx.probe_memory_stats()[0] - s0)
        return out[0], out[1], solos
    finally:
        ctx.set_probe_memory(DEFAULT_MEMORY)


def test_an_incoherent_buffer_goes_solo_after_two_finished_launches(ctx, street):
    w, n = street, street.n

    def fn():
        ctx.to_device(w.d_work, w.bounce)
        out, solo, verdicts = [], [], []
        for _ in range(4):
            s0 = ctx.probe_memory_stats()[0]
            w.sc.intersect_device_fresh(w.d_work, n, 1e30)
            solo.append(ctx.probe_memory_stats()[0] - s0)
            verdicts.append(ctx.last_probe()[2])                 # (synchronizes: the launch has finished before the next one is chosen)
            out.append(read(ctx, w.d_work, n))
        return out, solo, verdicts

    (off, solo_off, v_off), (on, solo_on, v_on), _ = memory_off_and_on(ctx, fn)
    assert solo_off == [0, 0, 0, 0] and solo_on == [0, 0, 1, 1]   # two finished incoherent launches first
    assert v_off == [1, 1, 1, 1] and v_on == [1, 1, 1, 1]         # a solo launch still publishes its sample (tbvh_debug_last_probe)
    assert int((off[0]["t"] < 1e30).sum()) > n // 4
    assert same(off, on) and same(off[1:], off[:-1])


def test_launches_in_flight_are_no_evidence(ctx, street):
    w, n = street, street.n

    def fn():
        ctx.to_device(w.d_work, w.bounce)
        ctx.synchronize()
        s0 = ctx.probe_memory_stats()[0]
        for _ in range(3):                                       # enqueued back to back: the third is chosen while the first is still running
            w.sc.intersect_device_fresh(w.d_work, n, 1e30)
        early = ctx.probe_memory_stats()[0] - s0
        ctx.synchronize()
        w.sc.intersect_device_fresh(w.d_work, n, 1e30)
        return read(ctx, w.d_work, n), early, ctx.probe_memory_stats()[0] - s0

    (off, _, _), (on, early, late), _ = memory_off_and_on(ctx, fn)
    assert early == 0 and late == 1
    assert same([off], [on])


def test_a_buffer_that_turns_coherent_is_traced_solo_once_then_two_flavors_again(ctx, street):
    w, n = street, street.n

    def fn():
        ctx.to_device(w.d_work, w.bounce)
        for _ in range(2):
            w.sc.intersect_device_fresh(w.d_work, n, 1e30)
            ctx.synchronize()
        out, solo, verdicts = [], [], []
        ctx.to_device(w.d_work, w.cam)                           # the same buffer, now camera rays
        for _ in range(3):
            s0 = ctx.probe_memory_stats()[0]
            w.sc.intersect_device_fresh(w.d_work, n, 1e30)
            solo.append(ctx.probe_memory_stats()[0] - s0)
            verdicts.append(ctx.last_probe()[2])
            out.append(read(ctx, w.d_work, n))
        return out, solo, verdicts

    (off, solo_off, v_off), (on, solo_on, v_on), _ = memory_off_and_on(ctx, fn)
    assert solo_off == [0, 0, 0] and solo_on == [1, 0, 0]         # predicted incoherent once; its own sample says coherent; two flavors from then on
    assert v_off == [2, 2, 2] and v_on == [2, 2, 2]
    assert int((off[0]["t"] < 1e30).sum()) > n // 4
    assert same(off, on)                                         # the coherent batch traced by the incoherent flavor alone: the same records


def test_a_buffer_that_turns_incoherent(ctx, street):
    w, n = street, street.n

    def fn():
        ctx.to_device(w.d_work, w.cam)
        for _ in range(2):
            w.sc.intersect_device_fresh(w.d_work, n, 1e30)
            ctx.synchronize()
        out, solo = [], []
        ctx.to_device(w.d_work, w.bounce)                        # the same buffer, now bounce rays
        for _ in range(4):
            s0 = ctx.probe_memory_stats()[0]
            w.sc.intersect_device_fresh(w.d_work, n, 1e30)
            solo.append(ctx.probe_memory_stats()[0] - s0)
            ctx.synchronize()
            out.append(read(ctx, w.d_work, n))
        return out, solo

    (off, solo_off), (on, solo_on), _ = memory_off_and_on(ctx, fn)
    assert solo_off == [0, 0, 0, 0] and solo_on == [0, 0, 1, 1]   # (coherent, coherent) -> (incoherent, coherent) -> (incoherent, incoherent)
    assert same(off, on)


def test_a_non_fresh_launch_after_a_fresh_one_keeps_the_reach_it_found(ctx, street):
    w, n = street, street.n
    t_near = 20.0

    def fn():
        ctx.to_device(w.d_work, w.bounce)
        out, solo = [], 0
        for _ in range(3):
            s0 = ctx.probe_memory_stats()[0]
            w.sc.intersect_device_fresh(w.d_work, n, t_near)     # near hits only; misses keep t = t_near ...
            w.sc.intersect_device(w.d_work, n)                   # ... which this launch must find there and leave
            solo += ctx.probe_memory_stats()[0] - s0
            ctx.synchronize()
            out.append(read(ctx, w.d_work, n))
        ctx.to_device(w.d_work, w.bounce)
        w.sc.intersect_device_fresh(w.d_work, n, 1e30)
        out.append(read(ctx, w.d_work, n))
        return out, solo

    (off, solo_off), (on, solo_on), _ = memory_off_and_on(ctx, fn)
    assert solo_off == 0 and solo_on >= 3
    assert same(off, on) and same(off[1:3], off[0:2])
    near, far = off[0], off[3]
    hits_near, hits_far = int((near["t"] < t_near).sum()), int((far["t"] < 1e30).sum())
    assert hits_far > hits_near > 1000                            # the reach does cut hits off: a launch that forgot it would show
    assert float(near["t"].max()) <= t_near


def test_an_undecided_tuner_keeps_every_launch_two_flavor(ctx, street):
    """The scene's coherent-schedule tuner must see the coherent launches it saw before: while it has not settled a class of batch, no launch of that class goes solo,
    whatever the memory holds.  A scene of its own, without the pinned hint of the fixture."""
    w, n = street, street.n
    sc = tb.BVH8_CWBVH(ctx).Build(w.verts)
    try:
        ctx.set_probe_memory(True)
        s0 = ctx.probe_memory_stats()
        ctx.to_device(w.d_work, w.bounce)
        for _ in range(5):                                       # incoherent launches are no samples: the tuner stays undecided, the memory fills
            sc.intersect_device_fresh(w.d_work, n, 1e30)
            assert ctx.last_probe()[2] == 1
        assert sc.coherent_schedule(False)[0] == 0
        s1 = ctx.probe_memory_stats()
        assert s1[0] == s0[0] and s1[1] - s0[1] >= 4            # no solo launch, though two incoherent verdicts and more are known
        ctx.to_device(w.d_cam, w.cam)
        for _ in range(14):                                      # coherent launches until it has decided (three schedules, three samples each)
            if sc.coherent_schedule(False)[0]:
                break
            sc.intersect_device_fresh(w.d_cam, n, 1e30)
            ctx.synchronize()
            assert ctx.probe_memory_stats()[0] == s0[0]
        assert sc.coherent_schedule(False)[0] != 0
        sc.intersect_device_fresh(w.d_work, n, 1e30)             # decided: the bounce buffer's launches go solo from here
        assert ctx.probe_memory_stats()[0] == s0[0] + 1
    finally:
        sc.free()
        ctx.set_probe_memory(DEFAULT_MEMORY)
