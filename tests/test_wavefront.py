"""Device-resident wavefront path tracer: queue bookkeeping and a
depth-1 frame re-computed on the host with the oracle (same RNG, same shading formulas)."""
import numpy as np
import pytest

import tinybvh_amd as tb
from tinybvh_amd import rays as R
from tinybvh_amd import scenes

pytestmark = pytest.mark.gpu


def wang(s):
    s = (s ^ np.uint32(61)) ^ (s >> np.uint32(16)); s = s * np.uint32(9); s = s ^ (s >> np.uint32(4)); s = s * np.uint32(0x27d4eb2d)
    return s ^ (s >> np.uint32(15))


def xorshift(s):
    s = s ^ (s << np.uint32(13)); s = s ^ (s >> np.uint32(17)); s = s ^ (s << np.uint32(5))
    return s


def test_frame_against_host_recomputation(ctx, oracle):
    verts = scenes.atrium(40_000, seed=1)
    verts[0::3, 3] = np.frombuffer(np.array([0x00C08040], np.uint32).tobytes(), np.float32)[0]   # albedo RGB8 in v0.w
    W, H = 256, 128
    sc = tb.BVH8_CWBVH(ctx).Build(verts)
    d_verts = ctx.malloc(verts.nbytes); ctx.to_device(d_verts, verts)
    eye, view = scenes.SPONZA_CAMERAS[0]
    cam = R.camera(eye, view, W, H, 1, 1)
    wf = tb.Wavefront(ctx, W, H)
    light, lcol, lo, hi, eps, seed = (0.0, 24.0, 0.0), (300.0, 280.0, 260.0), (0.6, 0.7, 0.8), (0.2, 0.4, 0.9), 1e-3, 5
    st = wf.render(sc, d_verts, cam, light, lcol, lo, hi, eps, max_depth=1, seed=seed)
    img = wf.read()
    n = W * H
    assert st["extend_rays"][0] == n
    # ---- host recomputation of the same frame -------------------------------------------------------
    with np.errstate(over="ignore"):
        i = np.arange(n, dtype=np.uint32)
        s = wang(np.uint32(seed) * np.uint32(9781) + i * np.uint32(6271) + np.uint32(1)); s = np.where(s == 0, np.uint32(1), s)
        s = xorshift(s); r0 = (s >> np.uint32(8)).astype(np.float32) * np.float32(1 / 16777216)
        s = xorshift(s); r1 = (s >> np.uint32(8)).astype(np.float32) * np.float32(1 / 16777216)
    in_tile = i & 15; tile = i >> 4; tiles_x = W // 4
    px = (tile % tiles_x) * 4 + (in_tile & 3); py = (tile // tiles_x) * 4 + (in_tile >> 2)
    u = (px.astype(np.float32) + r0) / np.float32(W); v = (py.astype(np.float32) + r1) / np.float32(H)
    e = np.array(cam.eye, np.float32); p1 = np.array(cam.p1, np.float32); p2 = np.array(cam.p2, np.float32); p3 = np.array(cam.p3, np.float32)
    P = p1 + u[:, None] * (p2 - p1) + v[:, None] * (p3 - p1)
    rays = tb.make_rays(np.broadcast_to(e, P.shape), P - e)
    h = sc.host
    hits = oracle.bvh2_intersect(h.bvh2_nodes(), h.bvh2_prim_idx(), verts, rays)
    hit = hits["t"] < 1e30
    want = np.zeros((n, 3), np.float64)
    k = 0.5 * (rays["D"][:, 1] + 1.0)
    sky = np.array(lo)[None, :] + k[:, None] * (np.array(hi) - np.array(lo))[None, :]
    want[~hit] = sky[~hit]
    tri = verts.reshape(-1, 3, 4)
    pr = hits["prim"][hit]
    v0, v1, v2 = tri[pr, 0, :3], tri[pr, 1, :3], tri[pr, 2, :3]
    N = np.cross(v1 - v0, v2 - v0); N /= np.linalg.norm(N, axis=1, keepdims=True)
    D = rays["D"][hit]
    N = np.where(((N * D).sum(1) > 0)[:, None], -N, N)
    I = rays["O"][hit] + hits["t"][hit][:, None] * D
    L = np.array(light)[None, :] - I; dist = np.linalg.norm(L, axis=1); L = L / dist[:, None]
    ndl = (N * L).sum(1)
    sh = tb.make_rays(I + L * eps, L, (dist - 2 * eps).astype(np.float32))
    occ = oracle.bvh2_occluded(h.bvh2_nodes(), h.bvh2_prim_idx(), verts, sh).astype(bool)
    albedo = np.array([0xC0, 0x80, 0x40], np.float64) * 0.00392
    g = ndl / dist ** 2 * 0.31830988
    c = albedo[None, :] * np.array(lcol)[None, :] * g[:, None]
    c[(ndl <= 0) | occ | (dist <= 2 * eps)] = 0
    want[hit] = c
    pix = (py * W + px).astype(np.int64)
    ref = np.zeros((n, 3)); np.add.at(ref, pix, want)
    got = img.reshape(-1, 4)[:, :3].astype(np.float64)
    # same pixels lit, same values up to float rounding of the shading math (sqrt / division order);
    # a few pixels may differ when a shadow ray grazes geometry
    bad = np.abs(got - ref).max(1) > 1e-3 * (1 + np.abs(ref).max(1))
    assert bad.sum() <= n // 2000, int(bad.sum())
    assert abs(got.mean() - ref.mean()) < 1e-3 * ref.mean()
    assert st["shadow_rays"][0] == int(((ndl > 0) & (dist > 2 * eps)).sum())      # (every decision held to the device's own: tests/test_wavefront_paths_gpu.py)
    wf.close(); ctx.free(d_verts)


def test_multi_bounce_bookkeeping(ctx):
    verts = scenes.atrium(40_000, seed=1)
    W, H = 512, 256
    sc = tb.BVH8_CWBVH(ctx).Build(verts)
    d_verts = ctx.malloc(verts.nbytes); ctx.to_device(d_verts, verts)
    eye, view = scenes.SPONZA_CAMERAS[1]
    cam = R.camera(eye, view, W, H, 1, 1)
    wf = tb.Wavefront(ctx, W, H)
    st = wf.render(sc, d_verts, cam, (0.0, 24.0, 0.0), (300.0, 300.0, 300.0), max_depth=3, seed=3)
    e, s = st["extend_rays"], st["shadow_rays"]
    assert e[0] == W * H and e[0] >= e[1] >= e[2] > 0          # only hit paths continue
    assert all(s[d] <= e[d] for d in range(3)) and s[0] > 0    # at most one shadow ray per live path
    a = wf.read()
    assert np.isfinite(a).all() and a[..., :3].min() >= 0 and a[..., :3].mean() > 0.01
    # accumulation over frames: a second frame without clearing roughly doubles the image
    wf.render(sc, d_verts, cam, (0.0, 24.0, 0.0), (300.0, 300.0, 300.0), max_depth=3, seed=4, clear=False)
    b = wf.read()
    assert 1.8 < b[..., :3].mean() / a[..., :3].mean() < 2.2
    wf.close(); ctx.free(d_verts)


# ---- materials (wavefront.cl:127-246): v0.w of a triangle's first vertex = type << 24 | RGB8 ------------------------

def quad(p0, du, dv, material):
    """Two triangles p0, p0+du, p0+du+dv / p0, p0+du+dv, p0+dv with the material word in v0.w of each."""
    p0, du, dv = (np.asarray(x, np.float32) for x in (p0, du, dv))
    v = np.zeros((6, 4), np.float32)
    v[0, :3], v[1, :3], v[2, :3] = p0, p0 + du, p0 + du + dv
    v[3, :3], v[4, :3], v[5, :3] = p0, p0 + du + dv, p0 + dv
    w = np.frombuffer(np.array([material], np.uint32).tobytes(), np.float32)[0]
    v[0, 3] = w; v[3, 3] = w
    return v


def down_camera(eye, half, W, H):
    """A pinhole at `eye` looking straight down at a (2 half)^2 patch one unit below it."""
    cam = tb.Camera()
    e = np.asarray(eye, np.float32)
    cam.eye[:] = [float(x) for x in e]
    cam.p1[:] = [float(e[0] - half), float(e[1] - 1), float(e[2] - half)]
    cam.p2[:] = [float(e[0] + half), float(e[1] - 1), float(e[2] - half)]
    cam.p3[:] = [float(e[0] - half), float(e[1] - 1), float(e[2] + half)]
    cam.width, cam.height, cam.spp_x, cam.spp_y = W, H, 1, 1
    return cam


def setup(ctx, verts, W, H):
    sc = tb.BVH8_CWBVH(ctx).Build(verts)
    d = ctx.malloc(verts.nbytes); ctx.to_device(d, verts)
    return sc, d, tb.Wavefront(ctx, W, H)


def test_emitter_seen_from_the_camera_and_finalize(ctx):
    """A MATERIAL_LIGHT triangle ends the path with T * lightColor (camera paths carry PATH_LAST_SPECULAR: no MIS)."""
    W = H = 64
    verts = quad((-50, 0, -50), (100, 0, 0), (0, 0, 100), (tb.MATERIAL_LIGHT << 24) | 0xFFFFFF)
    sc, d, wf = setup(ctx, verts, W, H)
    st = wf.render(sc, d, down_camera((0, 5, 0), 0.2, W, H), (0, 9, 0), (0.25, 0.5, 1.0), sky_lo=(0, 0, 0), sky_hi=(0, 0, 0), max_depth=3, light_size=(9, 5))
    img = wf.read()[..., :3]
    assert np.allclose(img, np.array([0.25, 0.5, 1.0], np.float32)[None, None, :], rtol=1e-6)
    assert st["extend_rays"] == [W * H, 0, 0] and st["shadow_rays"] == [0, 0, 0]      # the path ends there
    px = wf.finalize(1.0)
    assert px.shape == (H, W) and (px == ((127 << 16) | (180 << 8) | 255)).all()       # sqrt(0.25), sqrt(0.5), 1 -> 8 bit
    wf.close(); ctx.free(d)


def test_mirror_reflects_the_sky(ctx):
    """MATERIAL_SPECULAR: R = D - 2 N (N.D), throughput * colour, no shadow rays; the reflected ray leaves the scene
    and picks the sky colour of its direction."""
    W = H = 64
    verts = quad((-50, 0, -50), (100, 0, 0), (0, 0, 100), (tb.MATERIAL_SPECULAR << 24) | 0x8040FF)
    sc, d, wf = setup(ctx, verts, W, H)
    eye, view = (0.0, 3.0, -6.0), (0.0, -0.5, 1.0)
    cam = R.camera(eye, view, W, H, 1, 1)
    lo, hi = (0.9, 0.5, 0.1), (0.1, 0.3, 0.8)
    st = wf.render(sc, d, cam, (0, 9, 0), (1, 1, 1), sky_lo=lo, sky_hi=hi, max_depth=3, seed=2)
    img = wf.read()[..., :3].reshape(-1, 3).astype(np.float64)
    assert st["shadow_rays"] == [0, 0, 0]
    # host: the same jittered primary rays, reflected about +y
    n = W * H
    with np.errstate(over="ignore"):
        i = np.arange(n, dtype=np.uint32)
        s = wang(np.uint32(2) * np.uint32(9781) + i * np.uint32(6271) + np.uint32(1)); s = np.where(s == 0, np.uint32(1), s)
        s = xorshift(s); r0 = (s >> np.uint32(8)).astype(np.float32) * np.float32(1 / 16777216)
        s = xorshift(s); r1 = (s >> np.uint32(8)).astype(np.float32) * np.float32(1 / 16777216)
    in_tile = i & 15; tile = i >> 4; tiles_x = W // 4
    px = (tile % tiles_x) * 4 + (in_tile & 3); py = (tile // tiles_x) * 4 + (in_tile >> 2)
    u = (px.astype(np.float32) + r0) / np.float32(W); v = (py.astype(np.float32) + r1) / np.float32(H)
    e = np.array(cam.eye, np.float32); p1 = np.array(cam.p1, np.float32); p2 = np.array(cam.p2, np.float32); p3 = np.array(cam.p3, np.float32)
    D = p1 + u[:, None] * (p2 - p1) + v[:, None] * (p3 - p1) - e
    D = D / np.linalg.norm(D, axis=1, keepdims=True)
    hits_floor = D[:, 1] < 0
    t = -e[1] / np.where(hits_floor, D[:, 1], -1.0)
    P = e + t[:, None] * D
    hits_floor &= (np.abs(P[:, 0]) < 50) & (np.abs(P[:, 2]) < 50)
    Ry = np.where(hits_floor, -D[:, 1], D[:, 1])                                          # mirror about the floor, else straight to the sky
    k = 0.5 * (Ry + 1.0)
    sky = np.array(lo)[None, :] + k[:, None] * (np.array(hi) - np.array(lo))[None, :]
    col = np.array([0x80, 0x40, 0xFF], np.float64) * 0.00392
    want = np.where(hits_floor[:, None], sky * col[None, :], sky)
    ref = np.zeros((n, 3)); np.add.at(ref, (py * W + px).astype(np.int64), want)
    assert np.abs(img - ref).max() < 2e-4
    assert st["extend_rays"][:2] == [n, int(hits_floor.sum())] and st["extend_rays"][2] == 0
    wf.close(); ctx.free(d)


def test_area_light_with_mis_matches_the_irradiance_integral(ctx):
    """A diffuse floor under the reference's 9 x 5 rectangular light (wavefront.cl:208), light sampling + BSDF sampling
    combined by MIS: the radiance leaving the point below the light's centre is albedo / pi * E with
    E = Le * integral cos cos' / d^2 dA over the rectangle (direct light only: one plane, black sky)."""
    W = H = 128
    hgt, sx, sz, Le, rho = 4.0, 9.0, 5.0, np.array([6.0, 5.0, 4.0]), np.array([0xC0, 0xC0, 0x60]) * 0.00392
    floor = quad((-60, 0, -60), (120, 0, 0), (0, 0, 120), (tb.MATERIAL_DIFFUSE << 24) | 0xC0C060)
    # the emitter faces down: same rectangle the light sampling assumes, centred at light_pos
    lamp = quad((-sx / 2, hgt, -sz / 2), (0, 0, sz), (sx, 0, 0), (tb.MATERIAL_LIGHT << 24) | 0xFFFFFF)
    verts = np.concatenate([floor, lamp])
    sc, d, wf = setup(ctx, verts, W, H)
    cam = down_camera((0.0, 1.0, 0.0), 0.02, W, H)             # under the lamp, looking at the floor around the origin
    frames = 24
    for f in range(frames):
        wf.render(sc, d, cam, (0, hgt, 0), tuple(Le), sky_lo=(0, 0, 0), sky_hi=(0, 0, 0), eps=1e-3, max_depth=2, seed=11 + f, clear=(f == 0),
                  light_size=(sx, sz), stats=False)
    got = wf.read()[..., :3].reshape(-1, 3).astype(np.float64).mean(0) / frames
    # quadrature of the irradiance integral at the origin
    m = 600
    xs = (np.arange(m) + 0.5) / m * sx - sx / 2; zs = (np.arange(m) + 0.5) / m * sz - sz / 2
    X, Z = np.meshgrid(xs, zs, indexing="ij")
    d2 = X * X + Z * Z + hgt * hgt
    E = (hgt * hgt / (d2 * d2)).sum() * (sx / m) * (sz / m)    # cos = cos' = h / d
    want = rho / np.pi * Le * E
    assert np.all(np.abs(got - want) < 0.02 * want), (got, want)
    # light sampling alone (no bounce rays, so the BSDF-sampled half of the MIS pair is missing) must come out darker,
    # by what the bounce rays that reach the lamp carry: the two strategies really are weighted against each other
    wf.render(sc, d, cam, (0, hgt, 0), tuple(Le), sky_lo=(0, 0, 0), sky_hi=(0, 0, 0), eps=1e-3, max_depth=1, seed=5, light_size=(sx, sz), stats=False)
    nee_only = wf.read()[..., :3].reshape(-1, 3).astype(np.float64).mean(0)
    assert np.all(nee_only < 0.9 * want) and np.all(nee_only > 0.2 * want)
    wf.close(); ctx.free(d)


def test_one_diffuse_bounce_flag_is_the_references_path_length(ctx):
    """TBVH_WF_ONE_DIFFUSE_BOUNCE: a path ends at its second diffuse vertex (wavefront.cl:233), so an all-diffuse scene
    traces primary rays and one generation of bounce rays however large max_depth is."""
    verts = scenes.atrium(40_000, seed=1)
    W, H = 256, 128
    sc, d, wf = setup(ctx, verts, W, H)
    cam = R.camera(*scenes.SPONZA_CAMERAS[1], W, H, 1, 1)
    a = wf.render(sc, d, cam, (0.0, 24.0, 0.0), (300.0, 300.0, 300.0), max_depth=4, seed=3)
    b = wf.render(sc, d, cam, (0.0, 24.0, 0.0), (300.0, 300.0, 300.0), max_depth=4, seed=3, one_diffuse_bounce=True)
    assert a["extend_rays"][2] > 0 and a["extend_rays"][3] > 0
    assert b["extend_rays"][:2] == a["extend_rays"][:2] and b["extend_rays"][2:] == [0, 0]
    assert b["shadow_rays"][:2] == a["shadow_rays"][:2] and b["shadow_rays"][2:] == [0, 0]
    wf.close(); ctx.free(d)


# ---- the path tracer over a TLAS (tiny_bvh_gpu2.cpp / wavefront2.cl): vertices per BLAS, normals through the instance ----

def rot(axis, deg):
    a = np.deg2rad(deg); c, s = np.cos(a), np.sin(a)
    M = np.eye(4, dtype=np.float32)
    i, j = {"x": (1, 2), "y": (2, 0), "z": (0, 1)}[axis]
    M[i, i] = c; M[i, j] = -s; M[j, i] = s; M[j, j] = c
    return M


def test_tlas_scene_area_light_through_instances(ctx):
    """The MIS test again, but floor and lamp are instances: the lamp BLAS is a 5 x 9 rectangle at its local origin,
    turned 90 degrees about y and lifted by its instance transform into the 9 x 5 rectangle the light sampling assumes;
    the floor BLAS is a unit quad scaled 120 x 1 x 60."""
    W = H = 128
    hgt, sx, sz, Le, rho = 4.0, 9.0, 5.0, np.array([6.0, 5.0, 4.0]), np.array([0xC0, 0xC0, 0x60]) * 0.00392
    floor = quad((-0.5, 0, -0.5), (1, 0, 0), (0, 0, 1), (tb.MATERIAL_DIFFUSE << 24) | 0xC0C060)
    lamp = quad((-sz / 2, 0, -sx / 2), (0, 0, sx), (sz, 0, 0), (tb.MATERIAL_LIGHT << 24) | 0xFFFFFF)
    blas = [tb.BVH8_CWBVH(ctx).Build(floor), tb.BVH_GPU(ctx).Build(lamp)]            # mixed BLAS layouts while we are at it
    T = np.stack([np.diag([120.0, 1.0, 60.0, 1.0]).astype(np.float32), rot("y", 90.0)])
    T[1, 1, 3] = hgt
    inst = tb.make_instances(T, np.array([0, 1], np.uint32))
    tlas = tb.TLAS(ctx).Build(inst, blas)
    dv = []
    for v in (floor, lamp):
        d = ctx.malloc(v.nbytes); ctx.to_device(d, v); dv.append(d)
    wf = tb.Wavefront(ctx, W, H)
    wf.set_blas_vertices(dv)
    cam = down_camera((0.0, 1.0, 0.0), 0.02, W, H)
    frames = 24
    for f in range(frames):
        wf.render(tlas, 0, cam, (0, hgt, 0), tuple(Le), sky_lo=(0, 0, 0), sky_hi=(0, 0, 0), eps=1e-3, max_depth=2, seed=41 + f, clear=(f == 0),
                  light_size=(sx, sz), stats=False)
    got = wf.read()[..., :3].reshape(-1, 3).astype(np.float64).mean(0) / frames
    m = 600
    xs = (np.arange(m) + 0.5) / m * sx - sx / 2; zs = (np.arange(m) + 0.5) / m * sz - sz / 2
    X, Z = np.meshgrid(xs, zs, indexing="ij")
    d2 = X * X + Z * Z + hgt * hgt
    E = (hgt * hgt / (d2 * d2)).sum() * (sx / m) * (sz / m)
    want = rho / np.pi * Le * E
    assert np.all(np.abs(got - want) < 0.02 * want), (got, want)
    wf.close()
    for d in dv:
        ctx.free(d)


def test_tlas_scene_tilted_mirror_instance(ctx):
    """A mirror quad tilted 25 degrees about z by its instance transform (and scaled non-uniformly): the reflected sky
    colour follows the WORLD normal, i.e. the local normal through the transpose of the inverse transform."""
    W = H = 64
    mirror = quad((-0.5, 0, -0.5), (1, 0, 0), (0, 0, 1), (tb.MATERIAL_SPECULAR << 24) | 0xFFFFFF)
    blas = [tb.BVH4_GPU(ctx).Build(mirror)]
    M = rot("z", 25.0) @ np.diag([80.0, 3.0, 40.0, 1.0]).astype(np.float32)
    inst = tb.make_instances(M[None].astype(np.float32), np.array([0], np.uint32))
    tlas = tb.TLAS(ctx).Build(inst, blas)
    d = ctx.malloc(mirror.nbytes); ctx.to_device(d, mirror)
    wf = tb.Wavefront(ctx, W, H)
    wf.set_blas_vertices([d])
    cam = down_camera((0.0, 6.0, 0.0), 0.05, W, H)
    lo, hi = (0.9, 0.5, 0.1), (0.1, 0.3, 0.8)
    st = wf.render(tlas, 0, cam, (0, 9, 0), (1, 1, 1), sky_lo=lo, sky_hi=hi, max_depth=2, seed=2)
    img = wf.read()[..., :3].reshape(-1, 3).astype(np.float64)
    assert st["extend_rays"] == [W * H, W * H] and st["shadow_rays"] == [0, 0]
    N = (rot("z", 25.0)[:3, :3] @ np.array([0.0, 1.0, 0.0]))                       # world normal of the tilted plane
    Dc = np.array([0.0, -1.0, 0.0])                                                 # the narrow camera looks straight down
    Rc = Dc - 2.0 * N * (N @ Dc)
    k = 0.5 * (Rc[1] + 1.0)
    want = np.array(lo) + k * (np.array(hi) - np.array(lo))
    assert np.abs(img.mean(0) - want).max() < 0.01, (img.mean(0), want)            # +- the 0.05 field of view
    assert img.std(0).max() < 0.02
    wf.close(); ctx.free(d)
