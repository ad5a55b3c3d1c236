"""fp64 custom geometry (sphere BLASes of BVH_Double) on the GPU against the restatement (tests/oracle_custom_double.c) under the library's
rule: every record comes back byte-identical (t bit-identical, prim and inst exact, u and v as they went in, misses untouched) and every
occlusion byte equal.  The fixtures are those test_custom_double_host.py shows tree-independent on the CPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tinybvh_amd as tb
from custom_double_lib import (FAR, GOLDEN, N_RAYS, bounce_rays, camera_rays, chain_spheres, chain_tree, decorate, karras_spheres, ocd, same_records,  # noqa: F401 (ocd: fixture)
                               sphere_boxes, sphere_set, tlas_rays, tlas_scene, translated)
from double_lib import rotated_soup
from native_build import ROOT
from tinybvh_amd import lib, rays as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = tb.Context(0)
    yield c
    c.close()


def check_scene(ocd, sc, nodes, idx, sph, rays, what):
    """closest and any hit of scene sc (whose tree is nodes / idx) against the oracle; returns the traced records"""
    want = ocd.intersect(nodes, idx, sph, rays, rule=1)
    same_records(sc.Intersect(rays.copy()), want, what + " Intersect")
    occ, occ_want = sc.IsOccluded(rays), ocd.occluded(nodes, idx, sph, rays, rule=1)
    assert np.array_equal(occ, occ_want), f"{what} IsOccluded: {int((occ != occ_want).sum())} differ"
    return want


# ---- BLAS -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bunny", "soup"])
def test_blas_three_trees(ctx, ocd, name):
    """the uploaded host-builder tree, the device-built tree and the reference's own tree give the oracle's records, which are the same for all three"""
    sph = sphere_set(name)
    up = tb.SphereBVH_Double(ctx).Build(sph)
    dev = tb.SphereBVH_Double(ctx).BuildOnDevice(sph)
    assert lib.tbvh_scene_layout(up._h) == tb.LAYOUT_BVH_DOUBLE == lib.tbvh_scene_layout(dev._h) and up.device_bytes > 0
    dn, di, gathered = dev.Download()
    kn, ki = karras_spheres(sph)
    assert dn.tobytes() == kn.tobytes() and np.array_equal(di, ki) and np.array_equal(gathered, sph[ki.astype(np.int64)])
    cam = decorate(camera_rays(sph), 3)
    hn, hi = up.host.nodes(), up.host.prim_idx()
    traced = check_scene(ocd, up, hn, hi, sph, cam, name + " camera, uploaded")
    same_records(check_scene(ocd, dev, dn, di, sph, cam, name + " camera, device-built"), traced, "the two trees")
    bounce = decorate(bounce_rays(sph, ocd.intersect(hn, hi, sph, camera_rays(sph), rule=1)), 4)
    traced = check_scene(ocd, up, hn, hi, sph, bounce, name + " bounce, uploaded")
    same_records(check_scene(ocd, dev, dn, di, sph, bounce, name + " bounce, device-built"), traced, "the two trees")
    hit = traced["t"] != bounce["t"]
    assert hit.any() and np.array_equal(traced["inst"][hit], bounce["instIdx"][hit]) and np.array_equal(traced["u"], bounce["u"])
    # the real reference's tree (tests/golden/custom_double): uploaded as it is, the same records again
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    ref = tb.SphereBVH_Double(ctx).Upload(g["nodes"], g["prim_idx"], sph)
    same_records(check_scene(ocd, ref, g["nodes"], g["prim_idx"], sph, bounce, name + " bounce, the reference's tree"), traced, "the reference's tree")
    same_records(check_scene(ocd, ref, g["nodes"], g["prim_idx"], sph, cam, name + " camera, the reference's tree"),
                 ocd.intersect(hn, hi, sph, cam, rule=1), "the reference's tree")


# ---- edges ------------------------------------------------------------------------------------------------------------------------------
def test_one_sphere_is_a_leaf_root(ctx, ocd):
    sph = sphere_set("one")
    for sc in (tb.SphereBVH_Double(ctx).Build(sph), tb.SphereBVH_Double(ctx).BuildOnDevice(sph)):
        nodes, idx, _ = sc.Download()
        assert len(nodes) == 1 and nodes[0]["triCount"] == 1
        traced = check_scene(ocd, sc, nodes, idx, sph, camera_rays(sph, 256), "one sphere")
        assert 0 < (traced["t"] < 1e299).sum() < 256


def test_duplicates_tie_to_the_smaller_prim(ctx, ocd):
    sph = sphere_set("dups")
    for sc in (tb.SphereBVH_Double(ctx).Build(sph), tb.SphereBVH_Double(ctx).BuildOnDevice(sph)):
        nodes, idx, _ = sc.Download()
        traced = check_scene(ocd, sc, nodes, idx, sph, camera_rays(sph, 512), "duplicates")
        hit = traced["t"] < 1e299
        assert hit.sum() > 50 and (traced["prim"][hit] == 0).all()


def test_origins_inside_tangents_and_short_tmax(ctx, ocd):
    sph = sphere_set("soup")
    sc = tb.SphereBVH_Double(ctx).Build(sph)
    nodes, idx = sc.host.nodes(), sc.host.prim_idx()
    rng = np.random.default_rng(12)
    n = 1024
    k = rng.integers(0, len(sph), n)
    # origins inside a sphere: t <= 0, no hit from it (another sphere further on may be hit)
    inside = tb.make_rays_ex(sph[k, :3] + rng.normal(0, 0.1, (n, 3)) * sph[k, 3:4], rng.normal(size=(n, 3)))
    traced = check_scene(ocd, sc, nodes, idx, sph, inside, "origins inside")
    assert not (traced["prim"][traced["t"] < 1e299] == k[traced["t"] < 1e299]).any()
    # tangent rays: aimed at a point at distance exactly r (as exactly as doubles allow) from the centre, d <= 0 on some, d a rounding error on others
    D = rng.normal(size=(n, 3)); D /= np.linalg.norm(D, axis=1, keepdims=True)
    side = np.cross(D, rng.normal(size=(n, 3))); side /= np.linalg.norm(side, axis=1, keepdims=True)
    tangent = tb.make_rays_ex(sph[k, :3] + side * sph[k, 3:4] - 30.0 * D, D)
    check_scene(ocd, sc, nodes, idx, sph, tangent, "tangent rays")
    # a short incoming hit.t in front of and behind the sphere's near side
    cam = camera_rays(sph, n)
    first = ocd.intersect(nodes, idx, sph, cam, rule=1)
    hit = first["t"] < 1e299
    for scale, what in ((0.999, "tmax in front"), (1.001, "tmax behind")):
        short = cam.copy(); short["t"] = np.where(hit, first["t"] * scale, 5.0); short["u"] = 0.25; short["prim"] = 12345
        traced = check_scene(ocd, sc, nodes, idx, sph, short, what)
        if scale < 1:
            assert traced[hit].tobytes() == short[hit].tobytes()   # a miss leaves every byte as it was
        else:
            assert np.array_equal(traced["prim"][hit], first["prim"][hit])


def test_axis_parallel_rays_on_slab_planes(ctx, ocd):
    sph = sphere_set("soup")
    sc = tb.SphereBVH_Double(ctx).Build(sph)
    nodes, idx = sc.host.nodes(), sc.host.prim_idx()
    rng = np.random.default_rng(9)
    n = 2048
    axes = np.eye(3)[rng.integers(0, 3, n)] * rng.choice([-1.0, 1.0], (n, 1))
    pick = rng.integers(1, len(nodes), n)
    corner = np.where(rng.random((n, 3)) < 0.5, nodes["aabbMin"][pick], nodes["aabbMax"][pick])
    rays = tb.make_rays_ex(np.where(rng.random((n, 3)) < 0.5, corner, rng.uniform(-10, 10, (n, 3))), axes)
    assert np.isinf(rays["rD"]).any()
    traced = check_scene(ocd, sc, nodes, idx, sph, rays, "axis-parallel")
    assert (traced["t"] < 1e299).sum() > n // 20


@pytest.mark.parametrize("length", [0.5, 3.0])
def test_unnormalised_direction_records_ray_parameters(ctx, ocd, length):
    sph = sphere_set("soup")
    sc = tb.SphereBVH_Double(ctx).Build(sph)
    nodes, idx = sc.host.nodes(), sc.host.prim_idx()
    unit = camera_rays(sph, 1024)
    rays = unit.copy(); rays["D"] = unit["D"] * length; rays["rD"] = 1.0 / rays["D"]
    traced = check_scene(ocd, sc, nodes, idx, sph, rays, f"|D| = {length}")
    ref = ocd.intersect(nodes, idx, sph, unit, rule=1)
    hit = ref["t"] < 1e299
    both = hit & (traced["t"] < 1e299) & (traced["prim"] == ref["prim"])   # (a grazing ray may round to the other side of d <= 0)
    assert hit.sum() > 100 and both.sum() >= hit.sum() - 2
    assert np.allclose(traced["t"][both] * length, ref["t"][both], rtol=1e-9, atol=0)   # the recorded distance is a ray parameter, not a length


def test_deep_chain_uses_the_spill_area(ctx, ocd):
    nodes, idx, sph = chain_spheres(220)
    sc = tb.SphereBVH_Double(ctx).Upload(nodes, idx, sph)
    rng = np.random.default_rng(4)
    n = 1024
    O = np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n), np.full(n, 3.0 * 220 + 40.0)], 1)
    rays = tb.make_rays_ex(O, np.tile([0.0, 0.0, -1.0], (n, 1)) + np.concatenate([rng.normal(0, 1e-5, (n, 2)), np.zeros((n, 1))], 1))
    traced = check_scene(ocd, sc, nodes, idx, sph, rays, "chain")
    assert (traced["prim"] == 220).all()


def test_tlas_stack_overflow_is_an_error_not_a_wild_access(ocd):
    """test_double_gpu's overflow scene with sphere BLASes: a TLAS chain 40 levels deep over instances of a sphere chain 30 levels deep, a stack
    of 18 entries (TBVH_SPILL_ENTRIES=2).  Rays travelling in -z enter the instances with the stack full: TBVH_E_FORMAT; the other direction is
    answered right; the context traces correctly afterwards."""
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
        bn, bi, sph = chain_spheres(30)
        blas = tb.SphereBVH_Double(c).Upload(bn, bi, sph)
        n_inst = 41
        T = np.tile(np.eye(4), (n_inst, 1, 1))
        T[:, 2, 3] = 100.0 * np.arange(n_inst)
        inst = tb.make_instances_ex(T, 0)
        tb.host_build_tlas_double(inst, blas.bounds[None, :])   # (fills invTransform and the instance boxes)
        tn, ti = chain_tree(inst["aabbMin"], inst["aabbMax"]), np.arange(n_inst, dtype=np.uint64)
        tl = tb.TLAS_Double(c).Upload(tn, ti, inst, [blas])
        rng = np.random.default_rng(8)
        n = 256
        xy = np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n)], 1)
        bl = [("sph", bn, bi, sph)]
        errors = 0
        for z0, dz in ((100.0 * n_inst + 50.0, -1.0), (-50.0, 1.0)):
            rays = tb.make_rays_ex(np.concatenate([xy, np.full((n, 1), z0)], 1), np.tile([1e-5, 2e-5, dz], (n, 1)))
            for query in ("Intersect", "IsOccluded"):
                try:
                    if query == "Intersect":
                        same_records(tl.Intersect(rays.copy()), ocd.tlas_intersect(tn, ti, inst, bl, rays, rule=1), f"dz {dz} Intersect")
                    else:
                        assert np.array_equal(tl.IsOccluded(rays), ocd.tlas_occluded(tn, ti, inst, bl, rays, rule=1))
                    assert dz > 0, "the -z direction must overflow an 18-entry stack"
                except tb.TbvhError as e:
                    assert dz < 0 and e.code == -5 and "stack overflow" in str(e), e
                    errors += 1
        assert errors == 2
        s2 = sphere_set("soup")
        sc = tb.SphereBVH_Double(c).Build(s2)
        check_scene(ocd, sc, sc.host.nodes(), sc.host.prim_idx(), s2, camera_rays(s2, 1024), "after overflow")
    finally:
        c.close()


# ---- far from the origin ----------------------------------------------------------------------------------------------------------------
def test_far_from_the_origin(ctx, ocd):
    sph = sphere_set("small")
    far = sph.copy(); far[:, :3] += FAR
    rays = camera_rays(sph)
    moved = translated(rays, FAR)
    sc = tb.SphereBVH_Double(ctx).Build(far)
    traced = check_scene(ocd, sc, sc.host.nodes(), sc.host.prim_idx(), far, moved, "1e7 from the origin")
    dev = tb.SphereBVH_Double(ctx).BuildOnDevice(far)
    dn, di, _ = dev.Download()
    same_records(check_scene(ocd, dev, dn, di, far, moved, "1e7 from the origin, device-built"), traced, "the two trees")
    h0 = tb.host_build_custom_spheres_double(sph)
    near = ocd.intersect(h0.nodes(), h0.prim_idx(), sph, rays, rule=1)
    hit = near["t"] < 1e299
    same = ((traced["t"] < 1e299) == hit) & (~hit | (traced["prim"] == near["prim"]))
    assert hit.sum() > N_RAYS // 10 and (~same).sum() <= 2   # (test_custom_double_host.py: the oracle says so)
    # the fp32 sphere BLAS of the rounded set, beside it: recorded, not asserted
    s32 = tb.SphereBVH(ctx).Build(far.astype(np.float32))
    r32 = tb.make_rays(moved["O"].astype(np.float32), moved["D"].astype(np.float32))
    h32 = s32.Intersect(r32)
    hit32 = h32["t"] < np.float32(1e29)
    wrong = (hit32 != hit) | (hit & hit32 & (h32["prim"].astype(np.uint64) != near["prim"]))
    print(f"fp32 SphereBVH at 1e7: {int(wrong.sum())} of {N_RAYS} rays wrong ({int(hit.sum())} hit in fp64, {int(hit32.sum())} in fp32)")


# ---- TLAS_Double ------------------------------------------------------------------------------------------------------------------------
def _two_level(ctx):
    sph, verts, inst = tlas_scene()
    bs, bt = tb.SphereBVH_Double(ctx).Build(sph), tb.BVH_Double(ctx).Build(verts)
    tl = tb.TLAS_Double(ctx).Build(inst, [bs, bt])
    blas = [("sph", bs.host.nodes(), bs.host.prim_idx(), sph), ("tri", bt.host.nodes(), bt.host.prim_idx(), verts)]
    return sph, verts, inst, bs, bt, tl, blas


def check_tlas(ocd, tl, tn, ti, inst, blas, rays, what):
    want = ocd.tlas_intersect(tn, ti, inst, blas, rays, rule=1)
    same_records(tl.Intersect(rays.copy()), want, what + " Intersect")
    occ, occ_want = tl.IsOccluded(rays), ocd.tlas_occluded(tn, ti, inst, blas, rays, rule=1)
    assert np.array_equal(occ, occ_want), f"{what} IsOccluded: {int((occ != occ_want).sum())} differ"
    return want


def test_tlas_over_spheres_and_triangles(ctx, ocd):
    sph, verts, inst, bs, bt, tl, blas = _two_level(ctx)
    tn, ti = tl.host.nodes(), tl.host.prim_idx()
    rays = decorate(tlas_rays(inst), 6)
    traced = check_tlas(ocd, tl, tn, ti, inst, blas, rays, "six instances")
    hit = traced["t"] != rays["t"]
    assert hit.sum() > N_RAYS // 10 and np.unique(traced["inst"][hit]).size == 5 and not (traced["inst"][hit] == 5).any()   # (mask = 0: never entered)
    even = np.arange(N_RAYS) % 2 == 0   # ray mask 0x1: instances 0, 2, 4; 0x2: 1, 3, 4
    assert np.isin(traced["inst"][hit & even], [0, 2, 4]).all() and np.isin(traced["inst"][hit & ~even], [1, 3, 4]).all()
    on_sphere = hit & np.isin(traced["inst"], [0, 1, 3])
    assert on_sphere.sum() > 100 and np.array_equal(traced["u"][on_sphere], rays["u"][on_sphere])
    # the stale-u, v class: origins inside a triangle instance's box, a triangle hit first and a nearer sphere after it: the record's own u, v go back
    r0 = ocd.tlas_intersect(tn, ti, inst, blas, rays, rule=0)
    stale = int(((r0["u"] != traced["u"]) & on_sphere).sum())
    print("records where the reference's rule would leave a triangle's u, v under a sphere hit:", stale)
    assert stale > 0   # (the class is in the batch: instance 4's triangles lie inside instance 0)
    # every ray through every instance
    all_rays = rays.copy(); all_rays["mask"] = 0x3
    check_tlas(ocd, tl, tn, ti, inst, blas, all_rays, "mask 0x3")


def test_tlas_of_one_kind(ctx, ocd):
    sph, verts, inst, bs, bt, tl, blas = _two_level(ctx)
    for kind, scene, desc in (("spheres", bs, blas[0]), ("triangles", bt, blas[1])):
        one = inst.copy(); one["blasIdx"] = 0
        t1 = tb.TLAS_Double(ctx).Build(one, [scene])
        rays = decorate(tlas_rays(one, 2048), 8)
        traced = check_tlas(ocd, t1, t1.host.nodes(), t1.host.prim_idx(), one, [desc], rays, "TLAS of " + kind)
        assert (traced["t"] != rays["t"]).sum() > (200 if kind == "spheres" else 20)   # (the triangle soup is sparse)


# ---- moving spheres ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on_device", [False, True])
def test_rebuild_on_device_three_frames(ctx, ocd, on_device):
    rng = np.random.default_rng(21)
    sph = sphere_set("soup")[:1000].copy()
    sc = tb.SphereBVH_Double(ctx).BuildOnDevice(sph)
    verts = rotated_soup(300, seed=13) * 0.2
    bt = tb.BVH_Double(ctx).Build(verts)
    T = np.tile(np.eye(4), (2, 1, 1)); T[1, :3, 3] = [30.0, 0.0, 0.0]
    inst = tb.make_instances_ex(T, [0, 1])
    tl = tb.TLAS_Double(ctx).Build(inst, [sc, bt])
    d = ctx.malloc(sph.nbytes * 2) if on_device else 0
    try:
        bytes0 = None
        for frame in range(3):
            sph[:, :3] += rng.normal(0, 0.4, (sph.shape[0], 3)); sph[:, 3] *= rng.uniform(0.9, 1.1, sph.shape[0])
            if on_device:
                ctx.to_device(d, sph)
                sc.RebuildOnDevice((d, sph.shape[0]))
            else:
                sc.RebuildOnDevice(sph)
            nodes, idx, gathered = sc.Download()
            kn, ki = karras_spheres(sph)
            assert nodes.tobytes() == kn.tobytes() and np.array_equal(idx, ki) and np.array_equal(gathered, sph[ki.astype(np.int64)]), frame
            check_scene(ocd, sc, nodes, idx, sph, decorate(camera_rays(sph, 2048, seed=frame), frame), f"frame {frame}")
            tl.RebuildOnDevice(None)   # the new root box; no upload
            tn, ti, ti_inst = tl.Download()
            lo, hi = sphere_boxes(sph)
            assert np.array_equal(ti_inst["aabbMin"][0], lo.min(0)) and np.array_equal(ti_inst["aabbMax"][0], hi.max(0))
            rays = decorate(tlas_rays(ti_inst, 2048, seed=frame), frame)
            rays["mask"] = 0xFFFF
            check_tlas(ocd, tl, tn, ti, ti_inst, [("sph", nodes, idx, sph), ("tri", bt.host.nodes(), bt.host.prim_idx(), verts)], rays, f"TLAS, frame {frame}")
            if bytes0 is None:
                bytes0 = (sc.device_bytes, tl.device_bytes)   # (the first rebuild stages host spheres; nothing is allocated after it)
            assert (sc.device_bytes, tl.device_bytes) == bytes0, frame
        # a frame that grows n past the capacity: the scene moves, the TLAS over it is re-pointed
        grown = np.concatenate([sph, sphere_set("soup")[1000:1500]])
        if on_device:
            ctx.to_device(d, grown)
            sc.RebuildOnDevice((d, grown.shape[0]))
        else:
            sc.RebuildOnDevice(grown)
        nodes, idx, _ = sc.Download()
        kn, ki = karras_spheres(grown)
        assert nodes.tobytes() == kn.tobytes() and np.array_equal(idx, ki) and sc.device_bytes > bytes0[0]
        tl.RebuildOnDevice(None)
        tn, ti, ti_inst = tl.Download()
        rays = decorate(tlas_rays(ti_inst, 2048, seed=9), 9); rays["mask"] = 0xFFFF
        check_tlas(ocd, tl, tn, ti, ti_inst, [("sph", nodes, idx, grown), ("tri", bt.host.nodes(), bt.host.prim_idx(), verts)], rays, "TLAS after growth")
    finally:
        if d:
            ctx.free(d)


def test_first_rebuild_of_an_uploaded_scene_moves_it(ctx, ocd):
    sph = sphere_set("soup")[:300].copy()
    sc = tb.SphereBVH_Double(ctx).Build(sph)
    inst = tb.make_instances_ex(np.eye(4)[None], 0)
    tl = tb.TLAS_Double(ctx).Build(inst, [sc])
    sph[:, :3] *= 1.5
    sc.RebuildOnDevice(sph)
    tl.RebuildOnDevice(None)
    nodes, idx, _ = sc.Download()
    tn, ti, ti_inst = tl.Download()
    rays = camera_rays(sph, 1024)
    traced = check_tlas(ocd, tl, tn, ti, ti_inst, [("sph", nodes, idx, sph)], rays, "TLAS over a moved scene")
    assert (traced["t"] < 1e299).sum() > 100


# ---- batches and refusals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 65])
def test_batch_sizes(ctx, ocd, n):
    sph = sphere_set("soup")
    sc = tb.SphereBVH_Double(ctx).Build(sph)
    rays = camera_rays(sph, max(n, 1))[:n]
    got, occ = sc.Intersect(rays.copy()), sc.IsOccluded(rays)
    if n:
        same_records(got, ocd.intersect(sc.host.nodes(), sc.host.prim_idx(), sph, rays, rule=1), f"batch {n}")
        assert np.array_equal(occ, ocd.occluded(sc.host.nodes(), sc.host.prim_idx(), sph, rays, rule=1))


def test_device_resident_queries(ctx, ocd):
    sph = sphere_set("soup")
    sc = tb.SphereBVH_Double(ctx).Build(sph)
    rays = decorate(camera_rays(sph), 2)
    d = ctx.malloc(rays.nbytes); docc = ctx.malloc(rays.shape[0])
    try:
        ctx.to_device(d, rays)
        sc.occluded_device(d, rays.shape[0], docc)
        sc.intersect_device(d, rays.shape[0])
        out = np.zeros_like(rays); occ = np.zeros(rays.shape[0], np.uint8)
        ctx.from_device(out, d); ctx.from_device(occ, docc)
    finally:
        ctx.free(d); ctx.free(docc)
    same_records(out, ocd.intersect(sc.host.nodes(), sc.host.prim_idx(), sph, rays, rule=1), "device Intersect")
    assert np.array_equal(occ, ocd.occluded(sc.host.nodes(), sc.host.prim_idx(), sph, rays, rule=1))


def test_refusals(ctx, ocd):
    sph = sphere_set("soup")[:200]
    sc = tb.SphereBVH_Double(ctx).Build(sph)
    verts = np.zeros((600, 3))
    assert lib.tbvh_refit_double(sc._h, verts.ctypes.data, 200, 0) == -1 and b"sphere BLAS has no refit" in lib.tbvh_last_error()
    r32 = R.random_rays(64, (-5, -5, -5), (5, 5, 5))
    buf = np.zeros(1 << 12, np.uint8)
    s16 = np.zeros((200, 4), np.float32)
    nb_ = C.c_uint64(0)
    fp32_calls = {
        "tbvh_intersect": lambda h: lib.tbvh_intersect(h, r32.ctypes.data, 64, 64),
        "tbvh_occluded": lambda h: lib.tbvh_occluded(h, r32.ctypes.data, 64, 64, buf.ctypes.data),
        "tbvh_refit_custom_spheres": lambda h: lib.tbvh_refit_custom_spheres(h, s16.ctypes.data, 200, 0),
        "tbvh_rebuild_custom_spheres_device": lambda h: lib.tbvh_rebuild_custom_spheres_device(h, s16.ctypes.data, 200, 0),
        "tbvh_custom_spheres_download": lambda h: lib.tbvh_custom_spheres_download(h, None, 0, None, 0, None, 0, C.byref(nb_), C.byref(nb_)),
        "tbvh_scene_download": lambda h: lib.tbvh_scene_download(h, 0, None, 0, C.byref(nb_)),
        "tbvh_upload_tlas (double sphere BLAS)": lambda h: lib.tbvh_upload_tlas(ctx._h, buf.ctypes.data, 1, buf.ctypes.data, 1, buf.ctypes.data, 1, (C.c_void_p * 1)(h), 1,
                                                                                C.byref(C.c_void_p())),
    }
    for name, call in fp32_calls.items():
        assert call(sc._h) == -1, name
    # an fp32 sphere BLAS is no BLAS of a double TLAS, and takes none of the double sphere calls
    s32 = tb.SphereBVH(ctx).Build(sph.astype(np.float32))
    inst = tb.make_instances_ex(np.eye(4)[None], 0)
    th = tb.host_build_tlas_double(inst, sc.bounds[None, :])
    tn, ti = th.nodes(), th.prim_idx()
    h = C.c_void_p()
    assert lib.tbvh_upload_tlas_double(ctx._h, tn.ctypes.data, len(tn), ti.ctypes.data, ti.size, inst.ctypes.data, 1, (C.c_void_p * 1)(s32._h), 1, C.byref(h)) == -1
    assert lib.tbvh_rebuild_custom_spheres_double_device(s32._h, sph.ctypes.data, 200, 0) == -1
    assert lib.tbvh_custom_spheres_double_download(s32._h, None, 0, None, 0, None, 0, None, None) == -1
    # a triangle BVH_Double is no sphere scene either
    bt = tb.BVH_Double(ctx).Build(rotated_soup(100, seed=1))
    assert lib.tbvh_rebuild_custom_spheres_double_device(bt._h, sph.ctypes.data, 200, 0) == -1 and b"not a sphere BLAS" in lib.tbvh_last_error()
    # the scene still answers
    check_scene(ocd, sc, sc.host.nodes(), sc.host.prim_idx(), sph, camera_rays(sph, 256), "after the refusals")


# ---- the example ------------------------------------------------------------------------------------------------------------------------
def test_example_matches_the_host():
    exe = os.path.join(ROOT, "examples", "_build", "sphere_bvh_double")
    if not os.path.isfile(exe):
        pytest.skip("examples/_build/sphere_bvh_double is built only where the reference header is present")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 differing pixels" in out.stdout, out.stdout
