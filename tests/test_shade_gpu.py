"""tbvh_shade_hits / _device on the GPU (DESIGN.md par. 16): all 48 bytes of every record equal the plain-C restatement (tests/oracle_shade.c, pinned to the
real reference by tests/test_shade_host.py) on the really traced and the synthetic record set, at both strides, for a TLAS and for a single BLAS; a miss
gets the "no surface" record; bad device-resident indices are reported and never used; replacing and freeing leaves no allocation behind."""
import ctypes as C

import numpy as np
import pytest

import tinybvh_amd as tb
import shade_lib as L
import shade_fixtures as F
from shade_fixtures import shade_oracle, shade_sets  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(np.asarray(a), np.float32).view(np.uint32)


def allocations():
    live = (C.c_uint64 * 2)()
    tb.check(tb.lib.tbvh_debug_device_allocations(live), "tbvh_debug_device_allocations")
    return int(live[0]), int(live[1])


@pytest.fixture(scope="module")
def world(ctx):
    """the fixture scene on the device: two BLASes, the TLAS over the five instances, the shading table with both slots set"""
    sc = F.scene()
    blas = [tb.BVH8_CWBVH(ctx).Build(v) for v in sc.verts]
    inst = sc.instances.copy()
    tlas = tb.TLAS(ctx).Build(inst, blas)
    sh = tb.Shading(ctx, sc.materials, sc.textures)
    for k, f in enumerate(sc.fat):
        sh.SetFatTris(k, f)
    yield sc, blas, tlas, inst, sh
    sh.free(); tlas.free()
    for b in blas:
        b.free()


def device_shade(ctx, sh, scene, rays):
    """tbvh_shade_hits_device on a device copy of `rays` ((n,) records or (n, stride) bytes), guard words behind the output"""
    rays = np.ascontiguousarray(rays)
    n, stride = rays.shape[0], rays.strides[0]
    d_r, d_o = ctx.malloc(rays.nbytes), ctx.malloc(n * 48 + 64)
    out = np.full(n * 12 + 16, 0xDEADBEEF, np.uint32)
    ctx.to_device(d_r, rays); ctx.to_device(d_o, out)
    sh.ShadeHitsDevice(scene, d_r, n, d_o, stride)
    ctx.from_device(out, d_o)
    ctx.free(d_r); ctx.free(d_o)
    assert (out[n * 12:] == 0xDEADBEEF).all(), "wrote past the last record"
    return out[:n * 12].reshape(n, 12)


@pytest.mark.parametrize("name", ["traced", "synthetic"])
def test_records_equal_the_restatement(ctx, world, shade_sets, name):
    sc, blas, tlas, inst, sh = world
    r, host_inst, want, _ = shade_sets[name]
    assert inst.tobytes() == host_inst.tobytes()                        # the TLAS build filled the same instance records
    for rays in (r, F.ShadeScene.stride128(r)):
        got = device_shade(ctx, sh, tlas, rays)
        assert np.array_equal(got, bits(want)), f"{int((got != bits(want)).any(1).sum())} records differ"
        assert np.array_equal(bits(sh.ShadeHits(tlas, rays)), bits(want))
    assert ctx.time_last_ms() > 0


def test_traced_on_the_device(ctx, world, shade_oracle):
    """the camera rays through tbvh_intersect_device, shaded where they lie: equal to the restatement fed the same records; misses are "no surface" """
    sc, blas, tlas, inst, sh = world
    rays = sc.camera_rays()
    n = rays.shape[0]
    d_r, d_o = ctx.malloc(rays.nbytes), ctx.malloc(n * 48)
    ctx.to_device(d_r, rays)
    tlas.intersect_device(d_r, n)
    sh.ShadeHitsDevice(tlas, d_r, n, d_o)
    got = np.zeros((n, 12), np.uint32); traced = np.zeros_like(rays)
    ctx.from_device(got, d_o); ctx.from_device(traced, d_r)
    ctx.free(d_r); ctx.free(d_o)
    want, flags = shade_oracle.shade(sc.materials, sc.textures, sc.fat, traced, inst)
    hit = traced["t"] < 1e30
    assert hit.sum() > 300 and (~hit).sum() > 300 and set(np.unique(traced["inst"][hit])) == {0, 1, 2, 3, 4}
    assert np.array_equal(got, bits(want))
    assert (got[~hit][:, 3] == np.float32(-1).view(np.uint32)).all() and not np.delete(got[~hit], 3, 1).any()
    a = got.view(np.float32).view(tb.ShadedHits)
    assert np.array_equal(a.surface, hit) and set(np.unique(a.alpha[hit])) <= {0.0, 1.0}


def test_single_blas_scene(ctx, world, shade_oracle):
    sc, blas, tlas, inst, sh = world
    r = sc.synthetic_records()
    r = r[np.isin(r["inst"], (0, 3))].copy()
    r["inst"][::2] = 0xFFFFFFFF                                         # a BLAS's records carry ray.instIdx there: not looked at
    want, _ = shade_oracle.shade(sc.materials, sc.textures, sc.fat[:1], r, None)
    assert np.array_equal(device_shade(ctx, sh, blas[0], r), bits(want))
    assert np.array_equal(bits(sh.ShadeHits(blas[0], r)), bits(want))


def test_refusals(ctx, world):
    sc, blas, tlas, inst, sh = world
    r = sc.synthetic_records()[:64]
    dbl = tb.BVH_Double(ctx).Build(sc.verts[1][:, :3])
    dense = np.zeros((8, 8, 8), np.uint8); dense[2:5, 2:5, 2:5] = 1
    vox = tb.VoxelSet(ctx).Build(dense)
    sph = tb.SphereBVH(ctx).Build(np.array([[0, 0, 0, 1], [3, 0, 0, 1]], np.float32))
    for s in (dbl, vox, sph):
        with pytest.raises(tb.TbvhError) as e:
            sh.ShadeHits(s, r)
        assert e.value.code == -1, type(s).__name__
    for s in (dbl, vox, sph):
        s.free()
    d = ctx.malloc(64 * 128)
    for stride, off in ((72, 0), (48, 0), (64, 4)):
        with pytest.raises(tb.TbvhError) as e:
            sh.ShadeHitsDevice(tlas, d + off, 64, d, stride)
        assert e.value.code == -1
    ctx.free(d)
    bad = sc.fat[0].copy(); bad["material"][77] = 4
    with pytest.raises(tb.TbvhError) as e:                              # host-resident: refused before anything is allocated, the slot keeps its records
        sh.SetFatTris(0, bad)
    assert e.value.code == -5 and "triangle 77" in str(e.value)
    m = sc.materials.copy(); m["color_texture"][1] = 9
    with pytest.raises(tb.TbvhError) as e:
        tb.Shading(ctx, m, sc.textures)
    assert e.value.code == -5 and "material 1" in str(e.value)
    assert np.array_equal(sh.Download(0), sc.fat[0])


def test_sphere_blas_under_a_tlas_has_no_surface(ctx, world, shade_oracle):
    sc, blas, tlas, inst, sh = world
    sph = tb.SphereBVH(ctx).Build(np.array([[0, 0, 0, 1], [3, 0, 0, 1]], np.float32))
    T = np.tile(np.eye(4, dtype=np.float32), (2, 1, 1)); T[1, :3, 3] = [0, 0, 8]
    inst2 = tb.make_instances(T, [0, 1])
    t2 = tb.TLAS(ctx).Build(inst2, [blas[1], sph])
    r = sc.synthetic_records()[:256].copy()
    r["inst"] = np.arange(256) % 2; r["prim"] = np.arange(256) % 2
    want, flags = shade_oracle.shade(sc.materials, sc.textures, [sc.fat[1], None], r, inst2, slot_no_surface=[0, 1])
    assert ((flags & L.BAD_INDEX) == 0).all() and (want[1::2, 3] == -1).all() and (want[0::2, 3] >= 0).all()
    sh2 = tb.Shading(ctx, sc.materials, sc.textures).SetFatTris(0, sc.fat[1])
    assert np.array_equal(bits(sh2.ShadeHits(t2, r)), bits(want))       # and no status: ShadeHits would have raised
    sh2.free(); t2.free(); sph.free()


def test_bad_device_indices_are_reported_and_never_used(ctx, world, shade_oracle):
    """Device-resident records with one bad material, hit records with one bad inst and one bad prim: every index is compared with its table's size
    before it becomes an address (shade.h: shade_hit), so the bad ones come back as "no surface" resp. an untextured albedo of 0, the status word is
    raised and the next synchronising call returns TBVH_E_FORMAT."""
    sc, blas, tlas, inst, sh = world
    f = sc.fat[0].copy()
    r = sc.synthetic_records()[:512].copy()
    k_mat, k_inst, k_prim = 40, 41, 42
    r["inst"][k_mat] = 0; r["prim"][k_mat] = 300
    f["material"][300] = 0x80000001
    r["inst"][k_inst] = 5
    r["inst"][k_prim] = 4; r["prim"][k_prim] = 2                        # the quad has two triangles
    d_f = ctx.malloc(f.nbytes); ctx.to_device(d_f, f)
    sh2 = tb.Shading(ctx, sc.materials, sc.textures).SetFatTris(0, d_fat_tris=d_f, n_tris=f.size).SetFatTris(1, sc.fat[1])
    ctx.free(d_f)
    want, flags = shade_oracle.shade(sc.materials, sc.textures, [f, sc.fat[1]], r, inst)
    assert np.array_equal(np.flatnonzero(flags & L.BAD_INDEX), [k_mat, k_inst, k_prim])
    assert (want[[k_inst, k_prim], 3] == -1).all() and not want[k_mat, :3].any() and want[k_mat, 3] == 1 and bits(want[k_mat])[7] == 0x80000001
    got = device_shade(ctx, sh2, tlas, r)                               # (asynchronous: the status word stays raised ...)
    assert np.array_equal(got, bits(want))
    with pytest.raises(tb.TbvhError) as e:                              # (... until a call that reads it)
        sh2.Download(1)
    assert e.value.code == -5 and "shade" in str(e.value)
    assert np.array_equal(sh2.Download(0), f)                           # reported once, clear again
    with pytest.raises(tb.TbvhError) as e:
        sh2.ShadeHits(tlas, r)
    assert e.value.code == -5
    sh2.free()


def test_replacing_and_freeing_gives_everything_back(ctx, world):
    sc, blas, tlas, inst, sh = world
    ctx.synchronize()
    before, bytes_before = allocations(), tlas.device_bytes
    for order in (0, 1):
        a = tb.Shading(ctx, sc.materials, sc.textures).SetFatTris(1, sc.fat[1]).SetFatTris(0, sc.fat[0])
        b = tb.Shading(ctx, sc.materials[:1], None).SetFatTris(0, np.zeros(3, tb.FATTRI_DTYPE))   # (material 0 of one)
        held = allocations()
        a.SetFatTris(0, sc.fat[0][:100]); a.SetFatTris(0, sc.fat[0])    # replaced twice: the same number of allocations, the same bytes
        assert allocations() == held
        p, n = a.FatTris(0)
        assert p and n == sc.fat[0].size and np.array_equal(a.Download(0), sc.fat[0])
        for x in ((a, b) if order else (b, a)):
            x.free()
        assert allocations() == before and tlas.device_bytes == bytes_before


# ---- the FatTri half of SetPose: records attached to a pose follow it ---------------------------------------------------------------------------
def posed_world(ctx, sc, indexed):
    """slot 0's BLAS built so that it can be refitted from the pose (through its own index buffer for the indexed form), a TLAS of one identity instance over
    it, a shading table of its own holding slot 0's records"""
    cases = F.pose_cases()
    if indexed:
        c = cases["skin_indexed"]
        blas = tb.BVH_GPU(ctx).Build(c["rest"], indices=c["indices"])
    else:
        blas = tb.BVH_GPU(ctx).Build(sc.verts[0])
    lo, hi = sc.verts[0][:, :3].min(0), sc.verts[0][:, :3].max(0)
    blas._bounds = np.concatenate([lo - (hi - lo), hi + (hi - lo)]).astype(np.float32)      # (holds every frame)
    inst = tb.make_instances(np.eye(4, dtype=np.float32)[None], [0])
    tlas = tb.TLAS(ctx).Build(inst, [blas])
    sh = tb.Shading(ctx, sc.materials, sc.textures).SetFatTris(0, sc.fat[0])
    return cases, blas, tlas, inst, sh


def check_shading_follows(ctx, sc, tlas, inst, sh, posed, shade_oracle):
    """camera rays through the refitted scene, shaded with the table's records = the restatement fed the posed records"""
    eye = sc.verts[0][:, :3].mean(0) + np.array([0.1, 0.2, 3.0], np.float32) * sc.extent
    target = (posed["vertex0"] + posed["vertex1"] + posed["vertex2"])[::3] / np.float32(3)   # towards every third posed triangle's centroid
    r = tb.make_rays(np.tile(eye, (target.shape[0], 1)), target - eye)
    traced = tlas.Intersect(r)
    assert (traced["t"] < 1e30).sum() > 500
    want, _ = shade_oracle.shade(sc.materials, sc.textures, [posed], traced, inst)
    assert np.array_equal(bits(sh.ShadeHits(tlas, traced)), bits(want))


@pytest.mark.parametrize("kind", ["skin", "morph"])
def test_attached_records_follow_the_pose(ctx, world, shade_oracle, kind):
    sc = world[0]
    cases, blas, tlas, inst, sh = posed_world(ctx, sc, False)
    c, g = cases[kind], L.golden("pose_" + kind)
    if kind == "skin":
        pose = tb.Pose(ctx).Skin(c["rest"], c["joints"], c["weights"], c["mats"].shape[1])
        params = c["mats"]
    else:
        pose = tb.Pose(ctx).Morph(c["positions"])
        params = c["weights"]
    plain = tb.Pose(ctx).Skin(c["rest"], c["joints"], c["weights"], c["mats"].shape[1]) if kind == "skin" else tb.Pose(ctx).Morph(c["positions"])
    pose.AttachFatTris(sh, 0, c["normals"])
    for frame in (1, 0):
        pose.SetPose(params[frame]).Refit(blas)
        assert ctx.time_last_ms() >= 0
        got = sh.Download(0)
        assert got.tobytes() == F.host_posed(c, kind, frame).tobytes()                      # (pinned to the real SetPose by tests/test_shade_host.py)
        assert np.array_equal(pose.Download().view(np.uint32), plain.SetPose(params[frame]).Download().view(np.uint32))   # the vertices: as without records
    assert np.array_equal(L.words(got)[:, L.WRITTEN_WORDS], g["written"])                   # frame 0: the golden, bytewise
    assert L.only_these_changed(sc.fat[0], got, L.skin_fields() if kind == "skin" else L.morph_fields())
    tlas.RebuildOnDevice()
    check_shading_follows(ctx, sc, tlas, inst, sh, got, shade_oracle)
    # the table goes first: the pose is detached and poses vertices only
    sh.free()
    pose.SetPose(params[1])
    assert np.array_equal(pose.Download().view(np.uint32), plain.SetPose(params[1]).Download().view(np.uint32))
    pose.free(); plain.free(); tlas.free(); blas.free()


def test_indexed_and_flat_poses_give_identical_records(ctx, world, shade_oracle):
    sc = world[0]
    cases, blas, tlas, inst, sh = posed_world(ctx, sc, True)
    c, flat = cases["skin_indexed"], cases["skin"]
    pose = tb.Pose(ctx).Skin(c["rest"], c["joints"], c["weights"], c["mats"].shape[1]).AttachFatTris(sh, 0, c["normals"], indices=c["indices"])
    sh_flat = tb.Shading(ctx, sc.materials, sc.textures).SetFatTris(0, sc.fat[0])
    pose_flat = tb.Pose(ctx).Skin(flat["rest"], flat["joints"], flat["weights"], flat["mats"].shape[1]).AttachFatTris(sh_flat, 0, flat["normals"])
    for frame in (1, 0):
        pose.SetPose(c["mats"][frame]).Refit(blas)
        pose_flat.SetPose(flat["mats"][frame])
        got = sh.Download(0)
        assert got.tobytes() == sh_flat.Download(0).tobytes() == F.host_posed(c, "skin_indexed", frame).tobytes()
    assert np.array_equal(L.words(got)[:, L.WRITTEN_WORDS], L.golden("pose_skin")["written"])
    tlas.RebuildOnDevice()
    check_shading_follows(ctx, sc, tlas, inst, sh, got, shade_oracle)
    # refusals: a slot with another record count, indices that are no vertices (host: before anything is allocated), another context's table
    with pytest.raises(tb.TbvhError) as e:
        pose_flat.AttachFatTris(world[4], 1, flat["normals"])
    assert e.value.code == -1
    bad = c["indices"].copy(); bad[9, 2] = c["rest"].shape[0]
    with pytest.raises(tb.TbvhError) as e:
        pose.AttachFatTris(sh, 0, c["normals"], indices=bad)
    assert e.value.code == -5 and "triangle 9" in str(e.value)
    sh.SetFatTris(0, sc.fat[0][:100])                                                       # the slot changes under the pose: refused at the next SetPose
    with pytest.raises(tb.TbvhError) as e:
        pose.SetPose(c["mats"][0])
    assert e.value.code == -1
    before = allocations()
    pose.free(); pose_flat.free()
    assert allocations()[0] < before[0]
    sh.free(); sh_flat.free(); tlas.free(); blas.free()
