"""The seam between the launch plan (tinybvh_amd/csrc/launch_plan.h, asked through tbvh_debug_launch_plan) and the launch itself (capi_query.hip:
launchQuery): on a scene of the small class (20 000 triangles) a batch is probed for the packet kernel from 3 * 2^18 rays on, so batches of 3 * 2^18 - 64
and of 3 * 2^18 camera rays, and the larger one again under debug flag 64 (no probe), are the smallest shape at which the two can disagree.  For each the
plan is made from the scene's facts, the query runs once, tbvh_debug_last_probe must report a probe exactly where the plan says one runs — and what the three
runs write for the rays they share is the same, byte for byte: the probe chooses kernels, never results.

The context is this test's own, made with TBVH_COHERENT_TUNER unset: the scene's tuners start undecided and the facts say what they have settled on by each
launch.  256 CUs, 24 workgroups per CU and 128 rays per workgroup are stated as tbvh_init sets them on an MI355X; of the answers checked here only the grids depend on them."""
import os

import numpy as np
import pytest

import tinybvh_amd as tb
from tinybvh_amd import rays as R
from tinybvh_amd import scenes
from test_launch_plan_host import facts, plan

pytestmark = pytest.mark.gpu

N_PROBED = 3 * 2 ** 18           # 1024 x 768 camera rays
N_BELOW = N_PROBED - 64


@pytest.fixture(scope="module")
def own_ctx():
    saved = os.environ.pop("TBVH_COHERENT_TUNER", None)
    try:
        c = tb.Context(0)
    finally:
        if saved is not None:
            os.environ["TBVH_COHERENT_TUNER"] = saved
    yield c
    c.close()


def scene_facts(sc, n, anyhit, flags):
    hint = sc.schedule_hint()
    decided = (hint["any_hit"] if anyhit else hint["closest_hit"]) + [hint["small_batches"][1 if anyhit else 0]]
    blob = (sc.host.blob(0, np.uint32, 4).shape[0] + sc.host.blob(1, np.uint32, 4).shape[0]) * 16
    return facts(blobBytes=blob, n=n, any=int(anyhit), expFlags=flags, decided0=decided[0], decided1=decided[1], decided2=decided[2], decided3=decided[3],
                 hasPadded=0, hasHybrid=0, hasTrisPadded=0)       # (a small scene never gets the copies for incoherent batches)


def test_a_probe_runs_exactly_where_the_plan_says_and_changes_no_result(own_ctx):
    ctx = own_ctx
    verts = scenes.soup(20_000)
    sc = tb.BVH8_CWBVH(ctx).Build(verts)
    rays = R.primary(R.camera((5.0, 5.0, -12.0), (0.0, 0.0, 1.0), 1024, 768, 1, 1))
    assert rays.shape[0] == N_PROBED
    d_rays, d_occ = ctx.malloc(N_PROBED * 64), ctx.malloc(N_PROBED)
    hits, occs, said = [], [], []
    try:
        for n, flags in ((N_BELOW, 0), (N_PROBED, 0), (N_PROBED, 64)):
            ctx.set_debug_flags(flags)
            for anyhit in (False, True):
                p = plan(scene_facts(sc, n, anyhit, flags))
                assert p["small"] and not p["probed"]
                ctx.to_device(d_rays, rays[:n])
                if anyhit:
                    sc.occluded_device(d_rays, n, d_occ)
                else:
                    sc.intersect_device(d_rays, n)
                verdict = ctx.last_probe()[2]
                print(f"n {n} flags {flags} any {int(anyhit)}: plan probedSmall {p['probedSmall']} shape {p['shape']} grid {p['blocks']}, probe verdict {verdict}")
                assert (verdict != 0) == bool(p["probed"] or p["probedSmall"]), (n, flags, anyhit, p, verdict)
                said.append(bool(p["probedSmall"]))
                out = np.zeros(n, np.uint8 if anyhit else tb.RAY_DTYPE)
                ctx.from_device(out, d_occ if anyhit else d_rays)
                (occs if anyhit else hits).append(out[:N_BELOW])
    finally:
        ctx.set_debug_flags(0)
        ctx.free(d_rays)
        ctx.free(d_occ)
        sc.free()
    assert said == [False, False, True, True, False, False]      # the case is what it is meant to be: undecided tuners, the threshold between the batches
    assert 0 < int((hits[0]["t"] < 1e29).sum()) < N_BELOW          # some camera rays hit, some miss
    for other in hits[1:]:
        assert hits[0].tobytes() == other.tobytes()
    for other in occs[1:]:
        assert occs[0].tobytes() == other.tobytes()
    assert 0 < int(occs[0].sum()) < N_BELOW
