"""Independent device-resident queries overlap within one context (tbvh_context_set_overlap; tinybvh_amd/csrc/overlap_lanes.h, capi_query.hip: launchQuery): a
launch whose ray records and flags no launch in flight touches goes to the context's second lane and starts while the earlier launch's last waves still run.
A caller must see no difference but in time, so every case here runs the same sequence of calls twice — overlap off, overlap on — and compares what it reads
back byte for byte; the serial run itself is checked against the oracle once.  The scene is traced as uploaded and through the incoherent flavor on its
hybrid copies (set_hybrid + variant 90).  Batches of 64 k - 256 k rays: the hazards are in the host logic (lane choice, joins, per-lane counter areas), not in
the size."""
import os
import time

import numpy as np
import pytest

import tinybvh_amd as tb
from tinybvh_amd import rays as R
from tinybvh_amd import scenes
from oracle_lib import compare_hits

MODES = ["uploaded", "hybrid90"]
DEFAULT_ON = os.environ.get("TBVH_OVERLAP", "1") != "0"
T_NEAR = 34.0         # a reach that cuts off about half of the camera batch's hits (they lie 27 - 52 units from the eye)


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
    w.d_a, w.d_b = ctx.malloc(w.n * 64), ctx.malloc(w.n * 64)
    w.d_c = ctx.malloc(w.n * 64)
    w.d_big = [ctx.malloc(w.big.shape[0] * 64) for _ in range(2)]
    w.d_occ = [ctx.malloc(w.n) for _ in range(2)]
    w.d_verts = ctx.malloc(w.verts.nbytes)
    ctx.to_device(w.d_verts, w.verts)
    yield w
    for p in [w.d_a, w.d_b, w.d_c, w.d_verts] + w.d_big + w.d_occ:
        ctx.free(p)
    for sc in w.host_scene.values():
        sc.free()
    ctx.set_overlap(DEFAULT_ON)


def read(ctx, dptr, n):
    out = np.zeros(n, dtype=tb.RAY_DTYPE)
    ctx.from_device(out, dptr)
    return out


def read_occ(ctx, dptr, n):
    out = np.zeros(n, np.uint8)
    ctx.from_device(out, dptr)
    return out


def serial_and_overlapped(ctx, fn):
    """fn() run with overlap off, then on: (what each returned, lane-1 launches of the second run)"""
    try:
        ctx.set_overlap(False)
        s0 = ctx.overlap_stats()
        serial = fn()
        assert ctx.overlap_stats()[0] == s0[0]                 # off: nothing takes the second lane
        ctx.set_overlap(True)
        s1 = ctx.overlap_stats()
        over = fn()
        return serial, over, ctx.overlap_stats()[0] - s1[0]
    finally:
        ctx.set_overlap(DEFAULT_ON)


def same(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) for x, y in zip(a, b)) and len(a) == len(b)


def exact(got, want):
    c = compare_hits(got, want)
    assert c["hits"] > 1000 and c["hitmiss"] == 0 and c["prim_real"] == 0 and c["t_bad"] == 0 and c["uv_bad"] == 0, c
    assert c["tie"] == 0 and c["onsurf"] <= max(4, c["n"] // 5000), c
    assert c["bit_identical"] == c["same_prim"], c


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_disjoint_buffers_alternated(ctx, world, mode):
    w, sc = world, world.host_scene[mode]

    def fn():
        ctx.to_device(w.d_a, w.cam); ctx.to_device(w.d_b, w.bounce)
        for _ in range(3):
            sc.intersect_device_fresh(w.d_a, w.n, 1e30)
            sc.intersect_device_fresh(w.d_b, w.n, 1e30)
        return read(ctx, w.d_a, w.n), read(ctx, w.d_b, w.n)      # (no synchronize: from_device right after an overlapped pair)

    serial, over, lane1 = serial_and_overlapped(ctx, fn)
    assert same(serial, over)
    assert lane1 >= 3                                            # every second launch of the overlapped run took the second lane
    exact(serial[0], w.want_cam)
    exact(serial[1], w.want_bounce)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_same_buffer_and_ranges_sharing_one_ray_keep_their_order(ctx, world, mode):
    w, sc, n = world, world.host_scene[mode], world.n
    m = n // 2 + 37                                              # the shared ray: neither a multiple of the wave nor of the chunk

    def fn():
        out = []
        ctx.to_device(w.d_a, w.cam)
        sc.intersect_device_fresh(w.d_a, n, T_NEAR)              # near hits only; misses keep t = T_NEAR ...
        sc.intersect_device(w.d_a, n)                            # ... which this launch must find there (not the 1e30 of the upload)
        out.append(read(ctx, w.d_a, n))
        sc.intersect_device_fresh(w.d_a, n, 1e30)                # every hit ...
        sc.intersect_device_fresh(w.d_a, n, T_NEAR)              # ... cut back to the near ones: the other order leaves every hit
        out.append(read(ctx, w.d_a, n))
        for first_near in (False, True):                         # [0, m] and [m, n) share ray m: the later launch decides its record
            ctx.to_device(w.d_a, w.cam)
            if first_near:
                sc.intersect_device_fresh(w.d_a + m * 64, n - m, T_NEAR)
                sc.intersect_device_fresh(w.d_a, m + 1, 1e30)
            else:
                sc.intersect_device_fresh(w.d_a, m + 1, 1e30)
                sc.intersect_device_fresh(w.d_a + m * 64, n - m, T_NEAR)
            out.append(read(ctx, w.d_a, n))
        return out

    serial, over, _ = serial_and_overlapped(ctx, fn)
    assert same(serial, over)
    near, far = serial[1], w.want_cam
    assert int((far["t"] < 1e30).sum()) > int((near["t"] < T_NEAR).sum()) > 1000      # the reach does cut hits off: a reordering would show
    assert np.array_equal(serial[0].view(np.uint8), near.view(np.uint8))
    assert serial[2]["t"][m] == near["t"][m] and serial[3]["t"][m] == far["t"][m]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_any_hit_beside_closest_hit_and_a_shared_flag_buffer(ctx, world, mode):
    w, sc, n = world, world.host_scene[mode], world.n

    def fn():
        ctx.to_device(w.d_a, w.cam); ctx.to_device(w.d_b, w.bounce)
        ctx.to_device(w.d_occ[0], np.full(n, 7, np.uint8)); ctx.to_device(w.d_occ[1], np.full(n, 7, np.uint8))
        # closest-hit and any-hit on the SAME rays, flags in separate buffers: the any-hit launches read the reach the closest-hit launch before them left
        sc.occluded_device(w.d_a, n, w.d_occ[0])
        sc.intersect_device_fresh(w.d_a, n, T_NEAR)
        sc.occluded_device(w.d_a, n, w.d_occ[1])
        first = read_occ(ctx, w.d_occ[0], n), read_occ(ctx, w.d_occ[1], n), read(ctx, w.d_a, n)
        # two any-hit launches on different rays sharing ONE flag buffer: the later one's flags stay
        ctx.to_device(w.d_a, w.cam)
        sc.occluded_device(w.d_a, n, w.d_occ[0])
        sc.occluded_device(w.d_b, n, w.d_occ[0])
        return first + (read_occ(ctx, w.d_occ[0], n),)

    serial, over, _ = serial_and_overlapped(ctx, fn)
    assert same(serial, over)
    occ_far, occ_near, _, occ_b = serial
    assert np.array_equal(occ_far.astype(bool), w.want_cam["t"] < 1e30)
    assert int(occ_near.sum()) < int(occ_far.sum()) // 2          # (nothing lies in front of a closest hit: run before that launch, the second query would flag as the first)
    assert np.array_equal(occ_b.astype(bool), w.want_bounce["t"] < 1e30) and not np.array_equal(occ_b, occ_far)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_a_generator_reads_a_buffer_whose_launch_is_in_flight_on_the_second_lane(ctx, world, mode):
    w, sc, n = world, world.host_scene[mode], world.n

    def fn():
        ctx.to_device(w.d_a, w.cam); ctx.to_device(w.d_b, w.bounce)
        sc.intersect_device_fresh(w.d_b, n, 1e30)                # lane 0
        sc.intersect_device_fresh(w.d_a, n, 1e30)                # lane 1 in the overlapped run
        ctx.generate_bounce(w.d_verts, w.d_a, w.d_c, n, 77)      # reads the hits of the launch on lane 1
        sc.intersect_device_fresh(w.d_c, n, 1e30)                # and a launch on what the generator wrote (whichever lane: after the generator)
        return (read(ctx, w.d_c, n),)

    serial, over, lane1 = serial_and_overlapped(ctx, fn)
    assert same(serial, over) and lane1 >= 1
    assert int((serial[0]["t"] < 1e30).sum()) > 1000


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_a_refit_between_two_launches(ctx, world, mode):
    w, n = world, world.n
    sc = tb.BVH8_CWBVH(ctx).Build(w.verts)                       # (its own scene: the refit moves it)
    if mode == "hybrid90":
        sc.set_hybrid(1024); sc.set_variant(90)
    moved = w.verts.copy(); moved[:, 1] += np.float32(0.3) * np.sin(w.verts[:, 0]).astype(np.float32)

    def fn():
        sc.Refit(w.verts)
        ctx.to_device(w.d_a, w.cam); ctx.to_device(w.d_b, w.bounce); ctx.to_device(w.d_c, w.cam)
        sc.intersect_device_fresh(w.d_b, n, 1e30)
        sc.intersect_device_fresh(w.d_a, n, 1e30)                # in flight on the second lane when the refit is called
        sc.Refit(moved)
        sc.intersect_device_fresh(w.d_c, n, 1e30)
        sc.intersect_device_fresh(w.d_b, n, 1e30)
        return read(ctx, w.d_a, n), read(ctx, w.d_b, n), read(ctx, w.d_c, n)

    try:
        serial, over, lane1 = serial_and_overlapped(ctx, fn)
    finally:
        sc.free()
    assert same(serial, over) and lane1 >= 1
    assert np.array_equal(serial[0].view(np.uint8), read_back_reference(ctx, w, mode).view(np.uint8))   # before the refit: the unmoved scene's records
    assert not np.array_equal(serial[2]["t"], serial[0]["t"])                                         # after it: the moved one's


def read_back_reference(ctx, w, mode):
    """the camera batch on the module's unmoved scene, serial"""
    ctx.set_overlap(False)
    try:
        ctx.to_device(w.d_c, w.cam)
        w.host_scene[mode].intersect_device_fresh(w.d_c, w.n, 1e30)
        return read(ctx, w.d_c, w.n)
    finally:
        ctx.set_overlap(DEFAULT_ON)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_reported_times_are_positive_and_sum_to_at_most_the_wall_time(ctx, world, mode):
    """tbvh_time_history of overlapped launches: each reports the time it added (the end of the launch before it to its own end), so six alternated launches
    still sum to at most the loop's wall time.  The margin is what the same comparison needs with overlap off on this box (event time stamps against the host clock)."""
    w, sc = world, world.host_scene[mode]
    nb = w.big.shape[0]
    for d in w.d_big:
        ctx.to_device(d, w.big)

    def fn():
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            sc.intersect_device_fresh(w.d_big[0], nb, 1e30)
            sc.intersect_device_fresh(w.d_big[1], nb, 1e30)
        ctx.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        return (np.array(ctx.time_history(6), np.float64), np.float64(wall))

    fn()                                                         # (first launches of this size: not timed)
    serial, over, lane1 = serial_and_overlapped(ctx, fn)
    margin = max(0.0, float(serial[0].sum() - serial[1]))
    print(f"[{mode}] serial: sum {serial[0].sum():.4f} ms of wall {serial[1]:.4f} ms {np.round(serial[0], 4)}; overlapped: sum {over[0].sum():.4f} ms of wall {over[1]:.4f} ms {np.round(over[0], 4)}; margin {margin:.4f} ms")
    assert lane1 >= 3
    assert len(serial[0]) == 6 and (serial[0] > 0).all()
    assert len(over[0]) == 6 and (over[0] > 0).all(), over[0]
    assert over[0].sum() <= over[1] + margin, (over, margin)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_each_lane_has_its_own_counter_areas(ctx, world, mode):
    """The ray pool's two counter areas alternate per launch, each launch zeroing the other one for the next: shared between two overlapping launches that scheme
    hands rays out twice or never.  20 alternated launches of two 64 k batches: every record written, every record the serial run's."""
    w, sc, n = world, world.host_scene[mode], world.n

    def fn():
        ctx.to_device(w.d_a, w.cam); ctx.to_device(w.d_b, w.bounce)
        for _ in range(10):
            sc.intersect_device_fresh(w.d_a, n, 1e30)
            sc.intersect_device_fresh(w.d_b, n, 1e30)
        return read(ctx, w.d_a, n), read(ctx, w.d_b, n)

    serial, over, lane1 = serial_and_overlapped(ctx, fn)
    assert lane1 >= 10
    for got, ser in zip(over, serial):
        assert not ((got["t"] >= 1e30) & (ser["t"] < 1e30)).any()            # no record left armed where the serial run has a hit
    assert same(serial, over)
