"""tbvh_viewer_* / tbvh_sky_* on the GPU (DESIGN.md par. 22).  Every stage kernel equals its host twin (viewer.h compiled for the host, pinned to the real
reference by tests/test_viewer_host.py) in all bits on the same inputs: generate at all sizes and with first > 0, the sky at all skies, shadow rays, light in
both modes at strides 64 and 128, pack.  tbvh_viewer_render equals the same frame composed by this test from the public stage calls with a readback per
round — pixels, colours and final ray records bit-identical, the per-round ray counts equal — for both modes, a TLAS, a single BLAS and scenes with opacity micromaps; the 800 x 600 frame of both modes and scene kinds against the CPU frame over
oracle/_ref's traversal, which equals the golden buf; rendering twice
gives the same bytes; the 8-round cap, the refusals, bad device-resident indices (status word, no fault) and the allocations given back after destroy.
(Where a colour is a NaN — a NaN normal in the synthetic records — both sides must have a NaN; its payload is not compared.)"""
import ctypes as C

import numpy as np
import pytest

import tinybvh_amd as tb
import shade_fixtures as SF
import viewer_fixtures as F
import viewer_lib as L

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(np.asarray(a), np.float32).view(np.uint32)


def same_floats(a, b):
    """bit-identical, or a NaN on both sides"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def allocations():
    live = (C.c_uint64 * 2)()
    tb.check(tb.lib.tbvh_debug_device_allocations(live), "tbvh_debug_device_allocations")
    return int(live[0]), int(live[1])


class Dev:
    """device buffers of one test, freed together"""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def put(self, a, extra=0):
        a = np.ascontiguousarray(a)
        d = self.ctx.malloc(max(a.nbytes + extra, 16))
        self.ptrs.append(d)
        if a.nbytes:
            self.ctx.to_device(d, a)
        return d

    def room(self, nbytes):
        d = self.ctx.malloc(max(nbytes, 16))
        self.ptrs.append(d)
        return d

    def get(self, d, shape, dtype):
        out = np.zeros(shape, dtype)
        if out.nbytes:
            self.ctx.from_device(out, d)
        return out

    def free(self):
        for d in self.ptrs:
            self.ctx.free(d)
        self.ptrs = []


@pytest.fixture(scope="module")
def world(ctx):
    """the fixture scene on the device: three BLASes, the TLAS over the six instances, the shading table with the three slots set, the frames' sky; and the
    third BLAS once more as a scene of its own with a table whose slot 0 holds its records"""
    sc = F.scene()
    blas = [tb.BVH8_CWBVH(ctx).Build(v) for v in sc.verts]
    inst = sc.instances.copy()
    tlas = tb.TLAS(ctx).Build(inst, blas)
    sh = tb.Shading(ctx, sc.materials, sc.textures)
    for k, f in enumerate(sc.fat):
        sh.SetFatTris(k, f)
    sh_single = tb.Shading(ctx, sc.materials, sc.textures).SetFatTris(0, sc.fat[2])
    pixels = F.sky(F.FRAME_SKY)
    sky = tb.SkyDome(ctx, pixels)
    # the third BLAS once more with opacity micromaps baked from its materials' colour textures (alpha 0 of the "foliage masked" texels: that quad is gone for
    # the traversal), under a TLAS of its own with the other two
    f = sc.fat[2]
    uv = np.stack([np.stack([f[f"u{k}"], f[f"v{k}"]], 1) for k in range(3)], 1).reshape(-1, 2).astype(np.float32)
    blas_omm = tb.BVH8_CWBVH(ctx).Build(sc.verts[2])
    blas_omm.BakeOpacityMicroMaps(uv, sc.textures, 8, tri_texture=sc.materials["color_texture"][f["material"]].astype(np.uint32))
    tlas_omm = tb.TLAS(ctx).Build(sc.instances.copy(), [blas[0], blas[1], blas_omm])
    yield {"sc": sc, "blas": blas, "tlas": tlas, "inst": inst, "sh": sh, "sh_single": sh_single, "sky": sky, "pixels": pixels, "tlas_omm": tlas_omm, "blas_omm": blas_omm}
    sky.free(); sh.free(); sh_single.free(); tlas_omm.free(); blas_omm.free(); tlas.free()
    for b in blas:
        b.free()


def pick(world, which):
    if which == "blas_omm":
        return world["blas_omm"], world["sh_single"]
    return (world["tlas_omm" if which == "omm" else "tlas"], world["sh"]) if which in ("tlas", "omm") else (world["blas"][2], world["sh_single"])


# ---- the stages = their host twins -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", F.FRAME_SIZES)
def test_generate_equals_the_host_twin(ctx, size):
    cam = F.scene().camera(*size)
    n = size[0] * size[1]
    dev = Dev(ctx)
    guard = np.full(n * 16 + 16, 0xDEADBEEF, np.uint32)
    d = dev.put(guard)
    tb.viewer_generate(ctx, cam, d)
    got = dev.get(d, n * 16 + 16, np.uint32)
    want = tb.host_viewer_generate(cam)
    assert np.array_equal(got[:n * 16], want.view(np.uint32).reshape(-1)) and (got[n * 16:] == 0xDEADBEEF).all()
    first = n // 3
    ctx.to_device(d, guard)
    tb.viewer_generate(ctx, cam, d, first, n - first)
    got = dev.get(d, n * 16 + 16, np.uint32)
    k = (n - first) * 16
    assert np.array_equal(got[:k], want[first:].view(np.uint32).reshape(-1)) and (got[k:] == 0xDEADBEEF).all()
    dev.free()


@pytest.mark.parametrize("shape", F.SKY_SHAPES)
def test_sky_equals_the_host_twin(ctx, shape):
    pixels = F.sky(shape)
    dirs, _ = F.sky_directions()
    n = dirs.shape[0]
    d4 = np.zeros((n, 4), np.float32); d4[:, :3] = dirs
    dev = Dev(ctx)
    sky = tb.SkyDome(ctx, pixels)
    d_in, d_out = dev.put(d4), dev.put(np.full(n * 4 + 4, 0xDEADBEEF, np.uint32))
    sky.SampleDevice(d_in, n, d_out)
    got = dev.get(d_out, n * 4 + 4, np.uint32)
    want = tb.host_sky_sample(pixels, dirs)
    assert np.array_equal(got[:n * 4], bits(want).reshape(-1)) and (got[n * 4:] == 0xDEADBEEF).all()
    assert (got[:n * 4].reshape(n, 4)[:, 3] < shape[0] * shape[1]).all()
    sky.free(); dev.free()


def traced_records(ctx, world, size=(70, 53)):
    """a small frame's records and shading records as the device leaves them after round 0"""
    sc, tlas, sh = world["sc"], world["tlas"], world["sh"]
    cam = sc.camera(*size)
    n = size[0] * size[1]
    dev = Dev(ctx)
    d_r, d_o = dev.room(n * 64), dev.room(n * 48)
    tb.viewer_generate(ctx, cam, d_r)
    tlas.intersect_device(d_r, n)
    sh.ShadeHitsDevice(tlas, d_r, n, d_o)
    r, o = dev.get(d_r, n, tb.RAY_DTYPE), dev.get(d_o, (n, 12), np.float32)
    dev.free()
    return r, o


def lighting_inputs(ctx, world):
    r0, o0, occ0 = F.synthetic_lighting_records()
    r1, o1 = traced_records(ctx, world)
    occ1 = (np.arange(r1.shape[0]) % 3 == 0).astype(np.uint8)
    return np.concatenate([r0, r1]), np.concatenate([o0, o1]), np.concatenate([occ0, occ1])


def test_shadow_rays_and_pack_equal_the_host_twins(ctx, world):
    r, o, occ = lighting_inputs(ctx, world)
    n = r.shape[0]
    dev = Dev(ctx)
    for rays in (r, SF.ShadeScene.stride128(r)):
        for light in (None, np.array([0.3, -0.2, 0.9], np.float32)):
            d_r, d_s = dev.put(rays), dev.put(np.full(n * 16 + 16, 0xDEADBEEF, np.uint32))
            tb.viewer_shadow_rays(ctx, d_r, n, d_s, light, stride=rays.strides[0])
            got = dev.get(d_s, n * 16 + 16, np.uint32)
            want = tb.host_viewer_shadow_rays(rays if rays.dtype == tb.RAY_DTYPE else r, light)
            assert np.array_equal(got[:n * 16], want.view(np.uint32).reshape(-1)) and (got[n * 16:] == 0xDEADBEEF).all()
    rgb = np.zeros((4099, 4), np.float32)
    rgb[:, :3] = np.random.default_rng(1).uniform(-0.5, 1.5, (4099, 3))
    rgb[0, :3] = [np.nan, np.inf, -np.inf]; rgb[1, :3] = [1.0, 0.99999994, 0.0]; rgb[2, :3] = [-1e30, 2.0, 1 / 255]
    d_c, d_p = dev.put(rgb), dev.put(np.full(4099 + 4, 0xDEADBEEF, np.uint32))
    tb.viewer_pack(ctx, d_c, 4099, d_p)
    got = dev.get(d_p, 4099 + 4, np.uint32)
    assert np.array_equal(got[:4099], tb.host_viewer_pack(rgb)) and (got[4099:] == 0xDEADBEEF).all()
    dev.free()


@pytest.mark.parametrize("mode", [tb.VIEWER_GLTF, tb.VIEWER_FOLIAGE])
def test_light_equals_the_host_twin(ctx, world, mode):
    r, o, occ = lighting_inputs(ctx, world)
    n = r.shape[0]
    dev = Dev(ctx)
    d_o, d_occ = dev.put(o), dev.put(occ)
    for rays in (r, SF.ShadeScene.stride128(r)):
        d_r = dev.put(rays)
        for sky, pixels in ((world["sky"], world["pixels"]), (None, None)):
            for light in (None, np.array([0.3, -0.2, 0.9], np.float32)):
                d_c = dev.put(np.full(n * 4 + 4, 0xDEADBEEF, np.uint32))
                tb.viewer_light(ctx, mode, sky, d_r, d_o, n, d_c, d_occ=d_occ, light_dir=light, stride=rays.strides[0], shading=world["sh"])
                got = dev.get(d_c, n * 4 + 4, np.uint32)
                want = tb.host_viewer_light(mode, pixels, rays, o, occ, light)
                assert same_floats(got[:n * 4].view(np.float32).reshape(n, 4), want), f"{int((got[:n * 4].reshape(n, 4) != bits(want)).any(1).sum())} records differ"
                assert (got[n * 4:] == 0xDEADBEEF).all()
    dev.free()


# ---- the frame = the stages composed -----------------------------------------------------------------------------------------------------------------------
def staged_frame(ctx, world, which, cam, mode, max_rounds=8):
    """The frame from the public stage calls, with a readback per round: device generate, trace, shade; the records that continue are chosen on the host
    (tbvh_host_viewer_continue), traced and shaded as a batch of their own and scattered back; then the device's shadow rays, any-hit query, light and pack.
    Returns (pixels, rgb, final rays, rays traced per round, shadow rays that are not null, history: per round the pixel indices and their records after the
    trace)."""
    sc = world["sc"]
    scene, sh = pick(world, which)
    n = cam.width * cam.height
    dev = Dev(ctx)
    d_r, d_o, d_c, d_p = dev.room(n * 64), dev.room(n * 48), dev.room(n * 16), dev.room(n * 4)
    tb.viewer_generate(ctx, cam, d_r)
    scene.intersect_device(d_r, n)
    sh.ShadeHitsDevice(scene, d_r, n, d_o)
    rays, out = dev.get(d_r, n, tb.RAY_DTYPE), dev.get(d_o, (n, 12), np.float32)
    per_round, history = [n], [(np.arange(n), rays.copy())]
    if mode == tb.VIEWER_GLTF:
        live = np.arange(n)
        d_q, d_qo = dev.room(n * 64), dev.room(n * 48)
        for _ in range(1, max_rounds):
            sub = tb._aligned(rays[live].copy())
            went = tb.host_viewer_continue(sc.materials, sc.n_textures, sub, out[live])
            if not went.any():
                break
            live = live[went]
            q = np.ascontiguousarray(sub[went])
            ctx.to_device(d_q, q)
            scene.intersect_device(d_q, q.shape[0])
            sh.ShadeHitsDevice(scene, d_q, q.shape[0], d_qo)
            rays[live] = dev.get(d_q, q.shape[0], tb.RAY_DTYPE)
            out[live] = dev.get(d_qo, (q.shape[0], 12), np.float32)
            per_round.append(int(live.size))
            history.append((live.copy(), rays[live].copy()))
        ctx.to_device(d_r, rays); ctx.to_device(d_o, out)
    d_occ, real = 0, 0
    if mode == tb.VIEWER_FOLIAGE:
        d_s, d_occ = dev.room(n * 64), dev.room(n)
        tb.viewer_shadow_rays(ctx, d_r, n, d_s)
        scene.occluded_device(d_s, n, d_occ)
        real = int((rays["t"] < 10000).sum())
    tb.viewer_light(ctx, mode, world["sky"], d_r, d_o, n, d_c, d_occ=d_occ)
    tb.viewer_pack(ctx, d_c, n, d_p)
    pix, rgb = dev.get(d_p, n, np.uint32), dev.get(d_c, (n, 4), np.float32)
    dev.free()
    return pix, rgb, rays, per_round, real, history


CASES = [("omm", "gltf", (800, 600)), ("omm", "foliage", (800, 600)), ("blas_omm", "gltf", (160, 120)), ("blas_omm", "foliage", (160, 120)),
         ("tlas", "gltf", (800, 600)), ("tlas", "foliage", (800, 600)), ("blas", "gltf", (800, 600)), ("blas", "foliage", (160, 120)),
         ("tlas", "gltf", (1, 1)), ("tlas", "gltf", (3, 5)), ("tlas", "gltf", (70, 3)), ("tlas", "foliage", (70, 3))]


@pytest.mark.parametrize("which,mode_name,size", CASES)
def test_render_equals_the_staged_frame(ctx, world, which, mode_name, size):
    sc = world["sc"]
    scene, sh = pick(world, which)
    mode = tb.VIEWER_GLTF if mode_name == "gltf" else tb.VIEWER_FOLIAGE
    cam = sc.camera(*size)
    n = size[0] * size[1]
    want_pix, want_rgb, want_rays, per_round, real, _ = staged_frame(ctx, world, which, cam, mode)
    v = tb.Viewer(ctx, *size)
    st = v.Render(scene, sh, world["sky"], cam, mode=mode)
    pix, rgb, rays = v.Pixels().reshape(-1), v.RGB().reshape(-1, 4), v.Rays()
    assert np.array_equal(pix, want_pix), f"{int((pix != want_pix).sum())} of {n} pixels differ"
    assert np.array_equal(bits(rgb), bits(want_rgb))
    assert rays.tobytes() == want_rays.tobytes()
    assert st["rays"] == per_round + [0] * (8 - len(per_round)) and st["shadow_rays"] == real and st["frame_ms"] > 0
    # twice: the same bytes (the queue's order is free, the frame is not), also without waiting for the statistics
    assert v.Render(scene, sh, world["sky"], cam, mode=mode, stats=False) is None
    assert np.array_equal(v.Pixels().reshape(-1), pix) and np.array_equal(bits(v.RGB().reshape(-1, 4)), bits(rgb)) and v.Rays().tobytes() == rays.tobytes()
    assert ctx.time_last_ms() > 0
    if which == "omm" and mode == tb.VIEWER_FOLIAGE:                      # the micromaps are really in the traversal: the quad of alpha-0 texels is gone
        plain = tb.Viewer(ctx, *size)
        plain.Render(world["tlas"], sh, world["sky"], cam, mode=mode)
        a, b = plain.Rays(), rays
        gone = (a["t"] < 10000) & (a["inst"] == 5) & ((a["prim"] != b["prim"]) | (a["inst"] != b["inst"]) | (a["t"] != b["t"]))
        assert gone.sum() > 1000
        plain.free()
    if size == (800, 600):
        hit = rays["t"] < 10000
        assert hit.sum() > n // 20 and (~hit).sum() > n // 10
        if mode == tb.VIEWER_GLTF:                                         # the 8-round cap fixture: every round thins out, the last one still holds rays
            assert len(per_round) == 8 and all(a > b > 0 for a, b in zip(per_round, per_round[1:])), per_round
            moved = (rays["O"] != rays["O"][0]).any(1)
            assert (moved & ~hit).sum() > 100 and (moved & hit).sum() > 100
        else:
            assert 0 < real < n
    v.free()


@pytest.mark.parametrize("mode_name,kind", [(m, k) for m in ("gltf", "foliage") for k in ("tlas", "blas")])
def test_render_equals_the_cpu_frame(ctx, world, reference, mode_name, kind):
    """The 800 x 600 frame without the device: host generate -> oracle/_ref's traversal (the real tiny_bvh.h: ref_tlas_intersect for the TLAS, ref_intersect /
    ref_occluded for the single BLAS) per round -> tbvh_host_shade_hits -> tbvh_host_viewer_continue -> host light -> host pack.  That CPU frame equals the
    golden buf (WorkerThread's own, tools/make_viewer_golden.py).  The device frame equals it — pixels and colours — on every pixel whose per-round hit
    records are bit-equal (the device's per-round records are the staged frame's, which the render equals: test_render_equals_the_staged_frame); the pixels set
    aside number at most max( 4, n // 4000 ), the budget of tests/test_random_large.py (tests/test_viewer_host.py confirms on the CPU that the reference's own
    BVH_GPU traversal stays inside it on these rays)."""
    sc, sky = world["sc"], world["pixels"]
    mode = tb.VIEWER_GLTF if mode_name == "gltf" else tb.VIEWER_FOLIAGE
    size, n = (800, 600), 480000
    cam = sc.camera(*size)
    verts, fat, inst, lib_inst = F.scene_kind(sc, kind)
    trace, occluded = L.reference_tracers(reference, verts, inst, kind)
    cpu = L.cpu_frame(trace, occluded, sc, fat, lib_inst, cam, mode, sky)
    g = L.golden(f"frame_{mode_name}_{kind}")
    assert np.array_equal(cpu["pix"], g["buf"].reshape(-1)) and cpu["per_round"] == list(g["per_round"])
    scene, sh = pick(world, kind)
    staged = staged_frame(ctx, world, kind, cam, mode)
    v = tb.Viewer(ctx, *size)
    v.Render(scene, sh, world["sky"], cam, mode=mode)
    got_rgb, got_pix = v.RGB().reshape(-1, 4), v.Pixels().reshape(-1)
    assert np.array_equal(got_pix, staged[0])
    history = staged[5]
    if kind == "blas":                                                     # (a single BLAS's records carry ray.instIdx where a TLAS's carry hit.inst: not compared)
        for _, r in list(cpu["history"]) + list(history):
            r["inst"] = 0
    same = L.same_through_the_rounds(cpu["history"], history, n)
    if mode == tb.VIEWER_FOLIAGE:                                          # the shadow ray's flag is a hit record of this frame too
        d_occ = staged_occ(ctx, world, kind, cam)
        same &= (d_occ == cpu["occ"]) | (cpu["rays"]["t"] >= 10000)
    assert (~same).sum() <= max(4, n // 4000), f"{int((~same).sum())} of {n} pixels have a hit record that differs from the reference's"
    assert np.array_equal(bits(got_rgb[same]), bits(cpu["rgb"][same])) and np.array_equal(got_pix[same], cpu["pix"][same])
    assert (got_pix != g["buf"].reshape(-1)).sum() <= (~same).sum()
    v.free()


def staged_occ(ctx, world, which, cam):
    """the any-hit flags of the foliage frame's shadow rays, from the public stage calls"""
    scene, sh = pick(world, which)
    n = cam.width * cam.height
    dev = Dev(ctx)
    d_r, d_s, d_occ = dev.room(n * 64), dev.room(n * 64), dev.room(n)
    tb.viewer_generate(ctx, cam, d_r)
    scene.intersect_device(d_r, n)
    tb.viewer_shadow_rays(ctx, d_r, n, d_s)
    scene.occluded_device(d_s, n, d_occ)
    occ = dev.get(d_occ, n, np.uint8)
    dev.free()
    return occ


def test_round_cap_and_no_sky(ctx, world):
    sc, tlas, sh = world["sc"], world["tlas"], world["sh"]
    size = (160, 120)
    cam = sc.camera(*size)
    v = tb.Viewer(ctx, *size)
    full = v.Render(tlas, sh, world["sky"], cam)
    pix8 = v.Pixels().copy()
    assert all(x > 0 for x in full["rays"])
    for rounds in (1, 3):
        st = v.Render(tlas, sh, world["sky"], cam, max_rounds=rounds)
        assert st["rays"][:rounds] == full["rays"][:rounds] and not any(st["rays"][rounds:])
        want = staged_frame(ctx, world, "tlas", cam, tb.VIEWER_GLTF, max_rounds=rounds)
        assert np.array_equal(v.Pixels().reshape(-1), want[0]) and not np.array_equal(v.Pixels(), pix8)
    # no sky: every sample is 0 — a pixel that ends in the sky is black
    v.Render(tlas, sh, None, cam)
    miss = v.Rays()["t"] >= 10000
    assert miss.sum() > 1000 and not v.Pixels().reshape(-1)[miss].any() and v.Pixels().reshape(-1)[~miss].any()
    # a table without colour textures runs one round
    plain = sc.materials.copy(); plain["color_texture"] = tb.NO_TEXTURE
    sh2 = tb.Shading(ctx, plain, sc.textures)
    for k, f in enumerate(sc.fat):
        sh2.SetFatTris(k, f)
    st = v.Render(tlas, sh2, world["sky"], cam)
    assert st["rays"] == [size[0] * size[1]] + [0] * 7
    sh2.free(); v.free()


def test_refusals(ctx, world):
    sc, tlas, sh, sky = world["sc"], world["tlas"], world["sh"], world["sky"]
    v = tb.Viewer(ctx, 16, 8)
    cam = sc.camera(16, 8)
    dbl = tb.BVH_Double(ctx).Build(sc.verts[1][:, :3])
    dense = np.zeros((8, 8, 8), np.uint8); dense[2:5, 2:5, 2:5] = 1
    vox = tb.VoxelSet(ctx).Build(dense)
    sph = tb.SphereBVH(ctx).Build(np.array([[0, 0, 0, 1], [3, 0, 0, 1]], np.float32))
    for s in (dbl, vox, sph):
        with pytest.raises(tb.TbvhError) as e:
            v.Render(s, sh, sky, cam)
        assert e.value.code == -1, type(s).__name__
        s.free()
    for bad_cam in (sc.camera(8, 16), sc.camera(16, 4)):
        with pytest.raises(tb.TbvhError) as e:
            v.Render(tlas, sh, sky, bad_cam)
        assert e.value.code == -1
    for kw in ({"mode": 2}, {"max_rounds": 9}):
        with pytest.raises(tb.TbvhError) as e:
            v.Render(tlas, sh, sky, cam, **kw)
        assert e.value.code == -1
    other = tb.Context(0)
    try:
        sky2 = tb.SkyDome(other, world["pixels"])
        v2 = tb.Viewer(other, 16, 8)
        sh2 = tb.Shading(other, sc.materials, sc.textures)
        for args in ((v, tlas, sh, sky2), (v2, tlas, sh, sky), (v, tlas, sh2, sky)):
            with pytest.raises(tb.TbvhError) as e:
                args[0].Render(args[1], args[2], args[3], cam)
            assert e.value.code == -1
        with pytest.raises(tb.TbvhError) as e:
            tb.viewer_light(ctx, tb.VIEWER_GLTF, sky2, 256, 256, 1, 256)
        assert e.value.code == -1
    finally:
        other.close()                                                      # (frees its sky, viewer and table itself)
    for w, h in ((0, 4), (4, 0), (1 << 16, 1 << 16)):
        with pytest.raises(tb.TbvhError) as e:
            tb.Viewer(ctx, w, h)
        assert e.value.code == -1
    with pytest.raises(tb.TbvhError) as e:
        tb.viewer_light(ctx, tb.VIEWER_GLTF, sky, 256, 256, 1, 256, stride=72)
    assert e.value.code == -1
    with pytest.raises(tb.TbvhError) as e:
        tb.viewer_generate(ctx, cam, 256, 100, 100)
    assert e.value.code == -1
    assert v.Render(tlas, sh, sky, cam)["rays"][0] == 128                  # still in order after the refusals
    v.free()


def test_bad_device_indices_are_reported_and_never_used(ctx, world):
    """Device-resident FatTri records with a material index beyond the table on every triangle of the third slot: the shading kernel never uses it as an address
    (that hit is untextured with albedo 0), the gltf alpha rule compares it with the table's size before it looks at the material, the frame completes, and the
    status word makes the next synchronising call return TBVH_E_FORMAT — once."""
    sc, tlas, sky = world["sc"], world["tlas"], world["sky"]
    f = sc.fat[2].copy()
    f["material"] = 0x80000001
    d_f = ctx.malloc(f.nbytes); ctx.to_device(d_f, f)
    sh2 = tb.Shading(ctx, sc.materials, sc.textures).SetFatTris(0, sc.fat[0]).SetFatTris(1, sc.fat[1]).SetFatTris(2, d_fat_tris=d_f, n_tris=f.size)
    ctx.free(d_f)
    size = (160, 120)
    cam = sc.camera(*size)
    v = tb.Viewer(ctx, *size)
    with pytest.raises(tb.TbvhError) as e:
        v.Render(tlas, sh2, sky, cam)
    assert e.value.code == -5 and "shade" in str(e.value)
    pix, rays = v.Pixels().reshape(-1), v.Rays()                           # reported once, clear again; the frame is complete
    on_props = (rays["t"] < 10000) & (rays["inst"] == 5)
    assert on_props.sum() > 500 and not pix[on_props].any()                # albedo 0
    assert not (rays["O"] != rays["O"][0]).any()                           # nothing continued: no material, no mask
    st = v.Render(tlas, world["sh"], sky, cam)
    assert st["rays"][1] > 0
    v.free(); sh2.free()


def test_destroy_gives_everything_back(ctx, world):
    sc, tlas, sh = world["sc"], world["tlas"], world["sh"]
    cam = sc.camera(64, 48)
    warm = tb.Viewer(ctx, 64, 48)                                          # (the TLAS makes what its first any-hit query needs: not this test's subject)
    warm.Render(tlas, sh, None, cam, mode=tb.VIEWER_FOLIAGE); warm.Render(tlas, sh, None, cam, mode=tb.VIEWER_GLTF)
    warm.free()
    ctx.synchronize()
    before = allocations()
    for order in (0, 1):
        sky = tb.SkyDome(ctx, F.sky((5, 7)))
        v = tb.Viewer(ctx, 64, 48)
        created = allocations()
        v.Render(tlas, sh, sky, cam, mode=tb.VIEWER_GLTF)
        with_queues = allocations()
        v.Render(tlas, sh, sky, cam, mode=tb.VIEWER_FOLIAGE)
        with_shadow = allocations()
        v.Render(tlas, sh, sky, cam, mode=tb.VIEWER_GLTF); v.Render(tlas, sh, sky, cam, mode=tb.VIEWER_FOLIAGE)
        assert created[0] < with_queues[0] < with_shadow[0] and allocations() == with_shadow    # made once, by the first frame that needs them
        for x in ((v, sky) if order else (sky, v)):
            x.free()
        assert allocations() == before
