"""The wave-packet kernel with its child filter (kernels_cwbvh_packet.hip, packet_cull.h; variant 92 forces it whatever the batch) against the strict per-lane
kernel (variant 72) on the same scene: hit records byte for byte, occlusion flags equal.  The filter only removes per-lane tests whose answer was "no lane",
so the wave visits the nodes and tests the triangles it did before — these are the launches where a wrong bound, a stale wave cull distance, a dead lane
in the wave's boxes or a mixed chunk taking the filter would show.

The packet kernel tests a superset of a ray's candidates and may legitimately differ from the per-lane kernel at the knife edges of DESIGN.md par. 4, so
byte identity is only asked of inputs for which the kernels agreed BEFORE the filter existed: every scene, camera, seed and offset below was run on the
parent commit, where variants 92 and 72 agree byte for byte on all of them (five batches of the scenes moved by 1e6 only up to the ray count in PREFIX)."""
import os

import numpy as np
import pytest

import tinybvh_amd as tb
from tinybvh_amd import rays as R
from tinybvh_amd import scenes
from test_deep_tree import chain_bvh2, rays_along_x, check as check_chain

SCENES = {
    "soup": (lambda: scenes.soup(3_000, seed=5), ((-3.0, 5.0, -4.0), (0.6, -0.2, 0.75)), (5.0, 5.0, 14.0)),
    "street": (lambda: scenes.street(45_000, seed=2), scenes.STREET_CAMERAS[0], (-40.0, 3.0, 0.0)),
}


def ortho(eye, view, side, extent):
    """side x side parallel rays, origins on a square of `extent` around the eye, in the 4 x 4-tile order of the camera batches"""
    e, p1, p2, p3 = scenes.view_pyramid(eye, view)
    du, dv = (p2 - p1) / np.linalg.norm(p2 - p1), (p3 - p1) / np.linalg.norm(p3 - p1)
    i = np.arange(side * side)
    in_tile, tile = i & 15, i >> 4
    px, py = (tile % (side // 4)) * 4 + (in_tile & 3), (tile // (side // 4)) * 4 + (in_tile >> 2)
    O = np.asarray(eye, np.float32)[None, :] + extent * ((px / side - 0.5)[:, None] * du[None, :] + (py / side - 0.5)[:, None] * dv[None, :])
    return tb.make_rays(O.astype(np.float32), np.broadcast_to(np.asarray(view, np.float32), O.shape))


def both(sc, rays):
    """-> the records of variant 72 (strict per-lane); asserts variant 92's are the same bytes and the occlusion flags agree"""
    sc.set_variant(72)
    want = sc.Intersect(rays.copy())
    occ_want = sc.IsOccluded(rays.copy())
    sc.set_variant(92)
    got = sc.Intersect(rays.copy())
    occ = sc.IsOccluded(rays.copy())
    diff = np.flatnonzero((got.view(np.uint8).reshape(-1, 64) != want.view(np.uint8).reshape(-1, 64)).any(1))
    assert diff.size == 0, (diff.size, diff[:8], got[diff[:2]], want[diff[:2]])
    assert np.array_equal(occ, occ_want), np.flatnonzero(occ != occ_want)[:8]
    return want


BATCHES = ["camera", "ragged", "single", "ortho", "down", "preset"]
# Moved by 1e6 a unit of the street is 16 ulps and triangles collapse onto each other: there the packet kernel's superset of candidates and the per-lane
# kernel legitimately part ways for a few hundred rays (the knife edges of DESIGN.md par. 4), on the parent commit exactly as here (the same rays, the same
# counts).  These batches are cut in front of the first chunk with such a ray: the number of rays used, a multiple of 64.
PREFIX = {("soup", 1e6, "down"): 18_944, ("street", 1e6, "camera"): 40_960, ("street", 1e6, "ortho"): 50_176, ("street", 1e6, "down"): 51_200,
          ("street", 1e6, "preset"): 40_960}


@pytest.mark.gpu
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("shift", [0.0, 1e6])
@pytest.mark.parametrize("name", ["soup", "street"])
def test_packet_kernel_with_the_filter_returns_the_per_lane_records(ctx, name, shift, batch):
    n = PREFIX.get((name, shift, batch), 256 * 256)
    make, (eye, view), down_eye = SCENES[name]
    verts = make().copy()
    verts[:, :3] += np.float32(shift)
    eye = tuple(np.float32(x) + np.float32(shift) for x in eye)
    down_eye = tuple(np.float32(x) + np.float32(shift) for x in down_eye)
    sc = tb.BVH8_CWBVH(ctx).Build(verts)
    few = 500 if shift == 0.0 else -1              # (the batches must hit something; moved by 1e6 and cut short, the street's parallel rays need not)
    cam = R.primary(R.camera(eye, view, 256, 256, 1, 1))                                   # 1 024 chunks
    if batch == "camera":
        assert int((both(sc, cam[:n].copy())["t"] < 1e30).sum()) > few
    elif batch == "ragged":
        both(sc, cam[:64 * 37 + 5].copy())                                                 # a ragged last chunk
    elif batch == "single":
        both(sc, cam[64 * 100:64 * 100 + 129].copy())                                      # a last chunk of a single ray
    elif batch == "ortho":
        assert int((both(sc, ortho(eye, view, 256, 6.0)[:n].copy())["t"] < 1e30).sum()) > few         # parallel rays, distinct origins
    elif batch == "down":
        # looking exactly down -z: D.x == 0 in the centre column, D.y == 0 in the centre row, chunks of mixed octants around them
        down = R.primary(R.camera(down_eye, (0.0, 0.0, -1.0), 256, 256, 1, 1))
        assert np.any(down["D"][:, 0] == 0) and np.any(down["D"][:, 1] == 0)
        assert int((both(sc, down[:n].copy())["t"] < 1e30).sum()) > few
    else:
        # not fresh: every ray arrives with a hit distance of its own, half of them in front of the true hit (nothing to find), half behind it
        sc.set_variant(72)
        cam = cam[:n].copy()
        first = sc.Intersect(cam.copy())
        pre = cam.copy()
        hit = first["t"] < 1e30
        pre["t"] = np.where(hit, first["t"] * np.where(np.arange(cam.shape[0]) % 2 == 0, np.float32(0.5), np.float32(2.0)), np.float32(1e30)).astype(np.float32)
        got = both(sc, pre)
        odd = hit & (np.arange(cam.shape[0]) % 2 == 1)
        assert np.array_equal(got["t"][odd], first["t"][odd]) and np.array_equal(got["t"][~odd], pre["t"][~odd])
    sc.free()


@pytest.mark.gpu
def test_deep_chain_with_the_smallest_spill_area():
    """The wave's stack beyond its 64 in-register entries, with the spill area at its minimum (TBVH_SPILL_ENTRIES=2): ~100 wide levels fit, and the filter
    changes nothing about what is pushed."""
    depth = 700
    n2, pi, verts = chain_bvh2(depth)
    old = os.environ.get("TBVH_SPILL_ENTRIES")
    os.environ["TBVH_SPILL_ENTRIES"] = "2"
    try:
        c = tb.Context(0)
    finally:
        if old is None:
            os.environ.pop("TBVH_SPILL_ENTRIES", None)
        else:
            os.environ["TBVH_SPILL_ENTRIES"] = old
    try:
        sc = tb.BVH8_CWBVH(c).ConvertFromBVH2(n2, pi, verts)
        sc.set_variant(92)                           # (the per-lane kernels' own stacks do not hold this chain in a spill area this small: no twin to compare with,
        for sign in (-1.0, 1.0):                     #  the expected records are analytic, as in test_deep_tree.py)
            rays = rays_along_x(depth, 64 * 3 + 1, sign)
            check_chain(sc.Intersect(rays.copy()), depth, sign)
            assert sc.IsOccluded(rays.copy()).all()
        sc.free()
    finally:
        c.close()
