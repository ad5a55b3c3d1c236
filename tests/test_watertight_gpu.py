"""A scene in watertight mode on the device (tbvh_set_triangle_test; DESIGN.md par. 4.6): for every ray the closest triangle the UNCONTRACTED reference test
accepts among ALL the scene's triangles — prim exact, t / u / v bit-identical to the brute force recorded under tests/golden/watertight from the real reference
(tests/watertight_ref_shim.cpp built with -DWATERTIGHT_TRITEST -ffp-contract=off), zero differences, so no ray aimed at a vertex or an edge of a closed mesh
misses.  The default test is untouched by the call, and loses what the fixture says Moeller-Trumbore loses.  Batches are cut to a size that is no multiple
of 64 (the aimed sets, 108 N^2 rays, happen to be one).

Two levels: a TLAS over watertight BLASes (all of them, or tbvh_upload_tlas refuses) equals the instance-wise brute force, instance included; both kinds of
query run the watertight form of k_tlas8 (k_tlas4 has none: a deviation from the issue, DESIGN.md par. 4.6)."""
import ctypes as C

import numpy as np
import pytest

import tinybvh_amd as tb
from tinybvh_amd import _capi

import watertight_lib as W

pytestmark = pytest.mark.gpu
lib = _capi.lib
F = np.float32
CUT = 7   # rays left off the end of every batch: 19641 and 5817 rays, neither a multiple of 64


def make_scene(ctx, kind, verts):
    if kind == "bvh_gpu":
        return tb.BVH_GPU(ctx).Build(verts)
    if kind == "bvh4_gpu":
        return tb.BVH4_GPU(ctx).Build(verts)
    if kind == "cwbvh_build":      # whole triangles: the tree of BVH::Build
        return tb.BVH8_CWBVH(ctx).Build(verts, split_budget=0)
    if kind == "cwbvh_buildhq":    # spatial splits (30 % extra references): the tree of BVH::BuildHQ; a triangle may sit in several leaves
        return tb.BVH8_CWBVH(ctx).Build(verts)
    if kind == "device_lbvh":
        return tb.BVH8_CWBVH(ctx).BuildOnDevice(verts)
    if kind == "device_sah":
        return tb.BVH8_CWBVH(ctx).BuildOnDevice(verts, builder="sah")
    raise ValueError(kind)


KINDS = ("bvh_gpu", "bvh4_gpu", "cwbvh_build", "cwbvh_buildhq", "device_lbvh", "device_sah")


def trace(ctx, sc, rays):
    """(hit fields (n, 4) uint32, occlusion flags) through tbvh_intersect_device / tbvh_occluded_device"""
    n = rays.shape[0]
    d = ctx.malloc(rays.nbytes); o = ctx.malloc(n)
    try:
        ctx.to_device(d, rays)
        sc.occluded_device(d, n, o)
        occ = np.zeros(n, np.uint8); ctx.from_device(occ, o)
        sc.intersect_device(d, n)
        out = rays.copy(); ctx.from_device(out, d)
    finally:
        ctx.free(d); ctx.free(o)
    return W.hit_fields(out), occ


def unpack(bits, n):
    return np.unpackbits(bits)[:n]


def differences(got, want):
    return int((got != want).any(1).sum())


@pytest.mark.parametrize("N", [4, 12])
@pytest.mark.parametrize("kind", KINDS)
def test_closed_meshes_are_closed(ctx, kind, N):
    verts, rays, g = W.fixture_inputs(N)
    rays = rays[:-CUT]
    n, n_aimed = rays.shape[0], int(g["n_aimed"])
    sc = make_scene(ctx, kind, verts)
    try:
        assert sc.triangle_test == "moller-trumbore"
        sc.SetTriangleTest("watertight", verts)
        assert sc.triangle_test == "watertight"
        got, occ = trace(ctx, sc, rays)
    finally:
        sc.free()
    missed = int((got[:n_aimed, 0].view(F) >= W.BVH_FAR).sum())
    print(f"star{N} {kind}: aimed rays missed: library {missed}, the reference's own BVH::Intersect under its watertight test {int(g['counts'][2])}, "
          f"under Moeller-Trumbore {int(g['counts'][0])}; records differing from the brute force: {differences(got, g['wt'][:n])} of {n}")
    assert missed == 0
    assert differences(got, g["wt"][:n]) == 0
    assert np.array_equal(occ, unpack(g["wt_occ"], n))


@pytest.mark.parametrize("N", [4, 12])
@pytest.mark.parametrize("kind", ("bvh_gpu", "bvh4_gpu", "cwbvh_build"))
def test_the_default_is_untouched_and_the_set_has_teeth(ctx, kind, N):
    verts, rays, g = W.fixture_inputs(N)
    rays = rays[:-CUT]
    n_aimed = int(g["n_aimed"])
    never = make_scene(ctx, kind, verts)
    sc = make_scene(ctx, kind, verts)
    try:
        want, want_occ = trace(ctx, never, rays)
        bytes0 = sc.device_bytes
        before, before_occ = trace(ctx, sc, rays)
        bytes1 = sc.device_bytes   # (a first query may have made a derived copy)
        sc.SetTriangleTest("watertight", verts)
        assert sc.device_bytes >= bytes1 + verts.nbytes   # the vertex copy is counted
        wt, _ = trace(ctx, sc, rays)
        sc.SetTriangleTest("moller-trumbore")
        assert sc.triangle_test == "moller-trumbore" and sc.device_bytes in (bytes0, bytes1)
        after, after_occ = trace(ctx, sc, rays)
    finally:
        never.free(); sc.free()
    missed = int((want[:n_aimed, 0].view(F) >= W.BVH_FAR).sum())
    print(f"star{N} {kind}: aimed rays missed at test 0: {missed} (Moeller-Trumbore brute force: {int(g['counts'][1])})")
    assert missed >= int(g["counts"][1])   # no traversal finds a hit no triangle's test accepts
    assert np.array_equal(before, want) and np.array_equal(before_occ, want_occ)
    assert np.array_equal(after, want) and np.array_equal(after_occ, want_occ)   # back to 0: bit for bit
    assert differences(wt, want) > 0


@pytest.mark.parametrize("kind", ("bvh_gpu", "bvh4_gpu", "cwbvh_build", "device_lbvh"))
def test_a_refitted_watertight_scene_tests_the_new_vertices(ctx, kind):
    verts, _, _ = W.fixture_inputs(12)
    moved, rays, g = W.fixture_inputs(12, moved=True)
    rays = rays[:-CUT]
    n = rays.shape[0]
    sc = make_scene(ctx, kind, verts)
    try:
        sc.SetTriangleTest("watertight", verts)
        sc.Refit(moved)
        got, occ = trace(ctx, sc, rays)
    finally:
        sc.free()
    assert differences(got, g["wt"][:n]) == 0 and np.array_equal(occ, unpack(g["wt_occ"], n))


def test_an_updated_bvh_gpu_blob_brings_its_vertices(ctx):
    verts, _, _ = W.fixture_inputs(12)
    moved, rays, g = W.fixture_inputs(12, moved=True)
    rays = rays[:-CUT]
    n = rays.shape[0]
    sc = make_scene(ctx, "bvh_gpu", verts)
    try:
        sc.SetTriangleTest("watertight", verts)
        trace(ctx, sc, rays[:2048])
        h = tb.HostBVH(moved, tb.LAYOUT_BVH_GPU)
        sc.Update(h.blob(0, np.uint32, 16), h.blob(1, np.uint32, 1), moved)
        assert sc.triangle_test == "watertight"
        got, occ = trace(ctx, sc, rays)
    finally:
        sc.free()
    assert differences(got, g["wt"][:n]) == 0 and np.array_equal(occ, unpack(g["wt_occ"], n))


def test_a_morph_pose_refit(ctx):
    """tbvh_pose_refit with a morph pose: base = star12, one target = the moved mesh, weight 1 -> exactly the moved vertices (base + 1 * (target - base) is not
    the target in floating point, so the brute force is not the golden's: the posed vertices are read back and the records must be closed and equal to a
    watertight scene built over those vertices directly)."""
    verts, _, _ = W.fixture_inputs(12)
    moved, rays, g = W.fixture_inputs(12, moved=True)
    n_aimed = int(g["n_aimed"])
    pose = None
    sc = make_scene(ctx, "cwbvh_build", verts)
    direct = None
    try:
        sc.SetTriangleTest("watertight", verts)
        pose = tb.Pose(ctx).Morph(np.stack([verts[:, :3], moved[:, :3] - verts[:, :3]])).SetPose(np.array([1.0], F))   # (a target is an offset from the base)
        pose.Refit(sc)
        posed = pose.Download()
        v4 = np.zeros((posed.shape[0], 4), F); v4[:, :3] = posed[:, :3]
        direct = make_scene(ctx, "cwbvh_build", v4).SetTriangleTest("watertight", v4)
        got, occ = trace(ctx, sc, rays[:n_aimed])
        want, want_occ = trace(ctx, direct, rays[:n_aimed])
    finally:
        sc.free()
        if direct is not None:
            direct.free()
        if pose is not None:
            pose.free()
    assert int((got[:, 0].view(F) >= W.BVH_FAR).sum()) == 0   # the posed mesh is closed (its shared vertices are posed from the same inputs)
    # ... and an expectation from outside the device code: the host test (held to the reference bit for bit by the CPU tests) over every triangle of the posed mesh
    assert np.array_equal(got[:, 0], host_brute(tb.TRITEST_WATERTIGHT, rays[:n_aimed], v4).view(np.uint32))
    assert np.array_equal(got, want) and np.array_equal(occ, want_occ)


@pytest.mark.parametrize("kind", ("bvh_gpu", "cwbvh_buildhq"))
def test_opacity_micromaps_in_watertight_mode(ctx, kind):
    verts, rays, g = W.fixture_inputs(4)
    rays = rays[:-CUT]
    n = rays.shape[0]
    sc = make_scene(ctx, kind, verts)
    try:
        sc.SetOpacityMicroMaps(W.checker_map(verts.shape[0] // 3, 4), 4)
        sc.SetTriangleTest("watertight", verts)
        got, occ = trace(ctx, sc, rays)
    finally:
        sc.free()
    assert differences(got, g["omm"][:n]) == 0
    assert differences(got, g["wt"][:n]) > 0   # the map removes hits
    # (under a map the any-hit test is IntersectTri's — the reference's TriOccludes has no u, v to look up there, and the line put in for the shim would
    # take other corners' weights —, so a ray is occluded exactly when the closest-hit brute force finds it a hit)
    assert np.array_equal(occ, (g["omm"][:n, 0].view(F) < W.BVH_FAR).astype(np.uint8))


def test_one_consumer_the_sharded_call(ctx):
    verts, rays, g = W.fixture_inputs(12)
    rays = rays[:-CUT]
    sc = make_scene(ctx, "cwbvh_build", verts)
    try:
        sc.SetTriangleTest("watertight", verts)
        out = tb.intersect_sharded([sc], rays.copy())
    finally:
        sc.free()
    assert differences(W.hit_fields(out), g["wt"][:rays.shape[0]]) == 0


def test_refusals_leave_the_scene_usable(ctx):
    verts, rays, g = W.fixture_inputs(4)
    rays = rays[:-CUT]
    E = -1
    sc = make_scene(ctx, "cwbvh_build", verts)
    other = make_scene(ctx, "bvh_gpu", verts)
    pinned = make_scene(ctx, "bvh_gpu", verts)
    tlas = None
    try:
        assert lib.tbvh_set_triangle_test(sc._h, 2, verts.ctypes.data_as(C.c_void_p), verts.shape[0] // 3, 0) == E       # no such test
        assert lib.tbvh_set_triangle_test(sc._h, 1, None, 0, 0) == E                                                      # the scene holds no vertices
        assert b"vertices" in lib.tbvh_last_error()
        assert lib.tbvh_set_triangle_test(sc._h, 0, None, 0, 0) == 0                                                      # 0 on a scene at 0: nothing to do
        pinned.set_variant(1)
        assert lib.tbvh_set_triangle_test(pinned._h, 1, verts.ctypes.data_as(C.c_void_p), verts.shape[0] // 3, 0) == E    # pinned to its uploaded nodes
        sc.SetTriangleTest("watertight", verts)
        sc.SetTriangleTest("watertight")                                                                                   # NULL on a scene that holds its vertices
        assert lib.tbvh_set_variant(sc._h, 72) == E                                                                        # pinning a watertight scene
        inst = tb.make_instances(np.eye(4, dtype=F)[None], [0])
        two = tb.make_instances(np.stack([np.eye(4, dtype=F)] * 2), [0, 1])
        with pytest.raises(tb.TbvhError, match="all watertight or all not"):                                              # a mix of modes, either way round
            tb.TLAS(ctx).Build(two.copy(), [sc, other])
        with pytest.raises(tb.TbvhError, match="all watertight or all not"):
            tb.TLAS(ctx).Build(two.copy(), [other, sc])
        spheres = tb.SphereBVH(ctx).Build(np.array([[0, 0, 0, 1], [3, 0, 0, 0.5]], F))
        try:
            with pytest.raises(tb.TbvhError, match="watertight"):                                                         # watertight triangles next to another kind
                tb.TLAS(ctx).Upload(*_tlas_blob(two.copy(), [sc, sc]), [sc, spheres])
        finally:
            spheres.free()
        tlas = tb.TLAS(ctx).Build(inst, [other])
        assert lib.tbvh_set_triangle_test(other._h, 1, verts.ctypes.data_as(C.c_void_p), verts.shape[0] // 3, 0) == E  # a live TLAS is built over it
        assert b"TLAS" in lib.tbvh_last_error()
        assert lib.tbvh_set_triangle_test(tlas._h, 1, verts.ctypes.data_as(C.c_void_p), verts.shape[0] // 3, 0) == E   # a TLAS has no test of its own
        got, _ = trace(ctx, sc, rays)
        assert differences(got, g["wt"][:rays.shape[0]]) == 0
        trace(ctx, other, rays); trace(ctx, pinned, rays)
    finally:
        if tlas is not None:
            tlas.free()
        sc.free(); other.free(); pinned.free()


def test_a_record_naming_no_vertex_is_reported_not_dereferenced(ctx):
    verts, rays, _ = W.fixture_inputs(4)
    sc = make_scene(ctx, "cwbvh_build", verts)
    try:
        sc.SetTriangleTest("watertight", verts[:3 * 100])   # vertices for the first 100 triangles of 192
        with pytest.raises(tb.TbvhError, match="watertight"):
            sc.Intersect(rays.copy())
        sc.SetTriangleTest("watertight", verts)
        sc.Intersect(rays.copy())
    finally:
        sc.free()


def test_other_kinds_of_scene_are_refused_and_stay_usable(ctx):
    """BVH_DOUBLE, voxel and sphere scenes have no triangle test to choose: TBVH_E_INVALID, a text that names the kind, and the scene answers queries as before"""
    verts, rays, _ = W.fixture_inputs(4)
    vp, n_tris = verts.ctypes.data_as(C.c_void_p), verts.shape[0] // 3
    dense = np.zeros((8, 8, 8), np.uint32); dense[2:6, 2:6, 2:6] = 5
    spheres = np.array([[0, 0, 0, 1], [3, 0, 0, 0.5], [0, 3, 0, 0.5], [0, 0, 3, 0.25]], F)
    scenes = [(tb.BVH_Double(ctx).Build(verts[:, :3].astype(np.float64)), b"BVH_DOUBLE"), (tb.VoxelSet(ctx).Build(dense), b"voxel"), (tb.SphereBVH(ctx).Build(spheres), b"sphere")]
    try:
        for sc, word in scenes:
            for test in (tb.TRITEST_WATERTIGHT, tb.TRITEST_MOLLER_TRUMBORE):
                assert lib.tbvh_set_triangle_test(sc._h, test, vp, n_tris, 0) == -1, word
                assert word in lib.tbvh_last_error(), (word, lib.tbvh_last_error())
        small = tb.make_rays(np.array([[0.1, 0.1, -20.0], [3.0, 0.05, -20.0]], F), np.array([[0, 0, 1], [0, 0, 1]], F))
        assert int((scenes[1][0].Intersect(small.copy())["t"] < 1e30).sum()) >= 0 and int((scenes[2][0].Intersect(small.copy())["t"] < 1e30).sum()) == 2
        ex = tb.make_rays_ex(np.tile(W.eyes()[0].astype(np.float64), (4, 1)), rays["D"][:4].astype(np.float64))
        assert int((scenes[0][0].Intersect(ex)["t"] < 1e300).sum()) == 4   # from inside the closed mesh, unaimed: every ray hits
    finally:
        for sc, _ in scenes:
            sc.free()


def host_brute(test, rays, verts):
    """closest-hit t of every ray over every triangle, through the library's HOST triangle tests (tbvh_debug_tri_test_batch): 1e30 = no triangle accepts"""
    tri = np.ascontiguousarray(verts[:, :3].reshape(-1, 9))
    best = np.full(rays.shape[0], W.BVH_FAR, F)
    for at in range(0, rays.shape[0], 128):
        r = rays[at:at + 128]
        rr, tt = np.repeat(r, tri.shape[0]), np.tile(tri, (r.shape[0], 1))
        acc, tuv = np.zeros(rr.shape[0], np.uint8), np.zeros((rr.shape[0], 3), F)
        tb.check(lib.tbvh_debug_tri_test_batch(test, 0, rr.ctypes.data_as(C.c_void_p), tt.ctypes.data_as(C.c_void_p), rr.shape[0], acc.ctypes.data_as(C.c_void_p),
                                               tuv.ctypes.data_as(C.c_void_p), None), "tbvh_debug_tri_test_batch")
        t = np.where(acc == 1, tuv[:, 0], W.BVH_FAR).reshape(r.shape[0], -1)
        best[at:at + 128] = t.min(1)
    return best


def aimed_camera(verts):
    """An 80 x 60 view pyramid from the first eye whose corner p1 IS a mesh vertex or edge point — pixel ( 0, 0 ) looks exactly at it (viewer.h: P = p1 - eye
    there) — and is one that Moeller-Trumbore loses: the first aimed target, in the fixture's order, whose pixel-0 ray no triangle accepts at test 0 on the host."""
    eye = W.eyes()[0]
    aimed = W.aimed_rays(12)[:18 * 144 * 6 // 18]   # the first eye's rays come first; a sixth of them is plenty
    up = np.array([0.0, 1.0, 0.0], F)
    for k in range(aimed.shape[0]):
        f = aimed["D"][k]
        hit = host_brute(tb.TRITEST_WATERTIGHT, aimed[k:k + 1], verts)[0]
        T = (eye + f * hit).astype(F)
        r = np.cross(f, up); r = (r / np.linalg.norm(r)).astype(F)
        d = np.cross(f, r).astype(F)
        cam = tb.viewer_camera(eye, T, T + r * F(0.8) * hit, T + d * F(0.6) * hit, 80, 60)
        ray0 = tb.host_viewer_generate(cam, 0, 1)
        if host_brute(tb.TRITEST_MOLLER_TRUMBORE, ray0, verts)[0] >= W.BVH_FAR and host_brute(tb.TRITEST_WATERTIGHT, ray0, verts)[0] < W.BVH_FAR:
            return cam
    raise AssertionError("no aimed pixel that Moeller-Trumbore loses among the candidates")


def star_fat_tris(verts):
    v = verts[:, :3].reshape(-1, 3, 3)
    n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]); n = (n / np.linalg.norm(n, axis=1)[:, None]).astype(F)
    fat = np.zeros(v.shape[0], tb.FATTRI_DTYPE)
    for k in range(3):
        fat[f"vertex{k}"] = v[:, k]; fat[f"vN{k}"] = n
    fat["Nx"], fat["Ny"], fat["Nz"] = n[:, 0], n[:, 1], n[:, 2]
    return fat


def test_one_consumer_a_viewer_frame_from_inside_the_closed_mesh(ctx):
    """Viewer.Render of an 80 x 60 frame from inside star12, an opaque untextured material: every pixel looks at the mesh.  On the host twin first: at test 0 the
    aimed pixel's ray is accepted by no triangle, the watertight test loses no pixel.  Then on the device: in watertight mode no pixel's final record is a miss
    (no pixel shows the sky), at test 0 at least the aimed one is."""
    verts, _, _ = W.fixture_inputs(12)
    cam = aimed_camera(verts)
    twin = tb.host_viewer_generate(cam)
    assert twin.shape[0] == 80 * 60
    mt, wt = host_brute(tb.TRITEST_MOLLER_TRUMBORE, twin, verts), host_brute(tb.TRITEST_WATERTIGHT, twin, verts)
    assert mt[0] >= W.BVH_FAR and int((wt >= W.BVH_FAR).sum()) == 0
    mats = np.zeros(1, tb.MATERIAL_DTYPE); mats["color"] = 0.5; mats["color_texture"] = tb.NO_TEXTURE; mats["normal_texture"] = tb.NO_TEXTURE
    sky_pixels = np.zeros((4, 8, 3), F); sky_pixels[..., 2] = 9.0
    sc = make_scene(ctx, "cwbvh_build", verts)
    sh = tb.Shading(ctx, mats).SetFatTris(0, star_fat_tris(verts))
    sky = tb.SkyDome(ctx, sky_pixels)
    v = tb.Viewer(ctx, 80, 60)
    try:
        v.Render(sc, sh, sky, cam)
        sky0 = v.Rays()["t"] >= W.BVH_FAR
        sc.SetTriangleTest("watertight", verts)
        v.Render(sc, sh, sky, cam)
        sky1 = v.Rays()["t"] >= W.BVH_FAR
    finally:
        v.free(); sky.free(); sh.free(); sc.free()
    print(f"viewer frame from inside star12: pixels showing the sky at test 0: {int(sky0.sum())} (host twin, brute force: {int((mt >= W.BVH_FAR).sum())}), watertight: {int(sky1.sum())}")
    assert sky0[0] and int(sky0.sum()) >= int((mt >= W.BVH_FAR).sum())
    assert int(sky1.sum()) == 0


def _tlas_blob(inst, blas):
    """(nodes, indices, instances) of a host-built TLAS over `blas` (their .host vertices give the bounds), for Upload with another BLAS list"""
    bounds = np.array([np.concatenate([b.host.verts[:, :3].min(0), b.host.verts[:, :3].max(0)]) for b in blas], F)
    h = C.c_void_p()
    tb.check(lib.tbvh_host_build_tlas(inst.ctypes.data_as(C.c_void_p), inst.shape[0], bounds.ctypes.data_as(C.c_void_p), len(blas), C.byref(h)), "tbvh_host_build_tlas")
    host = tb.HostBVH.__new__(tb.HostBVH)
    host._h = h; host.layout = tb.LAYOUT_BVH_GPU; host.verts = None; host.n_tris = inst.shape[0]
    return host.blob(0, np.uint32, 16).copy(), host.blob(1, np.uint32, 1).copy(), inst   # (the handle goes with `host`)


@pytest.mark.parametrize("kinds", [("cwbvh_build", "cwbvh_buildhq"), ("bvh_gpu", "bvh4_gpu"), ("bvh4_gpu", "device_sah")])
def test_two_levels_equal_the_instance_wise_brute_force(ctx, kinds):
    """star4 and star12 under three instances — the identity, a rotation with a non-uniform scale, a mirrored one —, closest hit and occlusion: inst, prim exact,
    t / u / v bit-identical to the reference's test through the reference's instance transform on every ray, and no aimed ray misses"""
    inst, verts, rays, g = W.tlas_fixture_inputs()
    rays = rays[:-CUT]
    n, n_aimed = rays.shape[0], int(g["n_aimed"])
    blas = [make_scene(ctx, k, v) for k, v in zip(kinds, verts)]
    tlas = None
    try:
        for b, v in zip(blas, verts):
            b.SetTriangleTest("watertight", v)
            if not hasattr(b, "host"):   # (a device-built BLAS: TLAS.Build takes its bounds from .host)
                b._bounds = np.concatenate([v[:, :3].min(0), v[:, :3].max(0)]).astype(F)
        tlas = tb.TLAS(ctx).Build(inst.copy(), blas)
        assert tlas.triangle_test == "watertight"
        d = ctx.malloc(rays.nbytes); o = ctx.malloc(n)
        ctx.to_device(d, rays)
        tlas.occluded_device(d, n, o)
        occ = np.zeros(n, np.uint8); ctx.from_device(occ, o)
        tlas.intersect_device(d, n)
        out = rays.copy(); ctx.from_device(out, d)
        ctx.free(d); ctx.free(o)
    finally:
        if tlas is not None:
            tlas.free()
        for b in blas:
            b.free()
    got = W.hit_fields_inst(out)
    missed = int((got[:n_aimed, 0].view(F) >= W.BVH_FAR).sum())
    print(f"TLAS {kinds}: aimed rays missed {missed} (Moeller-Trumbore brute force: {int(g['mt_misses'])}); records differing from the instance-wise brute force: "
          f"{differences(got, g['wt'][:n])} of {n}")
    assert missed == 0
    assert differences(got, g["wt"][:n]) == 0
    assert np.array_equal(occ, unpack(g["wt_occ"], n))
