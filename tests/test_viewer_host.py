"""The viewer frame's arithmetic on the CPU (DESIGN.md par. 22), no GPU: the library's host twins (viewer.h compiled for the host) against the plain-C
restatement with libm's atan2f / acosf (tests/oracle_viewer.c), and the restatement against the real reference (tests/viewer_ref_shim.cpp: the viewer files'
own SampleSky, Trace and WorkerThread over a TLAS the reference builds) on every ray of an 800 x 600 frame of each viewer, with zero exceptions.  The host
twins equal the restatement in all bits wherever SKY_EDGE is clear; where it is set the texel is one of the two across the near boundary.  The margin behind
SKY_EDGE comes from the measurement in profiles/viewer.txt (tests/viewer_lib.py: margins), and at most 1 / 2000 of a frame's pixels may carry it."""
import numpy as np
import pytest

import tinybvh_amd as tb
import shade_fixtures as SF
import viewer_fixtures as F
import viewer_lib as L
from native_build import NO_REFERENCE
from viewer_fixtures import viewer_oracle  # noqa: F401  (fixture)


def bits(a):
    return np.ascontiguousarray(np.asarray(a), np.float32).view(np.uint32)


def records(rays):
    return np.ascontiguousarray(rays).view(np.float32).reshape(rays.shape[0], -1)


LIGHT = None   # the default: normalize( 2, 4, 5 )


default_light = F.default_light


# ---- the margin is a measurement ---------------------------------------------------------------------------------------------------------------------
def test_margin_comes_from_the_measurement():
    atan2_ulp, acos_ulp = L.measured_ulps()
    assert 0.5 <= atan2_ulp < 8 and 0.5 <= acos_ulp < 8
    mu, mv = L.margins()
    assert mu == atan2_ulp + 5 and mv == acos_ulp + 4


# ---- generator -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", F.FRAME_SIZES)
def test_generate_equals_the_restatement(viewer_oracle, size):
    cam = F.scene().camera(*size)
    n = size[0] * size[1]
    got = tb.host_viewer_generate(cam)
    want = viewer_oracle.generate(cam)
    assert got.shape[0] == n and np.array_equal(bits(records(got)), bits(want))
    first = n // 3
    assert np.array_equal(bits(records(tb.host_viewer_generate(cam, first, n - first))), bits(want[first:]))
    assert (got["mask"] == 0xFFFF).all() and (got["t"] == np.float32(1e30)).all()
    if n > 1:                                                              # row-major: the second ray is the pixel to the right (or, one column wide, below)
        assert not np.array_equal(got["D"][0], got["D"][1])


def test_generate_refusals():
    cam = F.scene().camera(8, 4)
    for first, n in ((0, 33), (30, 3)):
        with pytest.raises(tb.TbvhError) as e:
            tb.host_viewer_generate(cam, first, n)
        assert e.value.code == -1
    import ctypes as C
    assert tb.lib.tbvh_host_viewer_generate(C.byref(cam), None, 1 << 63, 1 << 63) == -1    # first + n wraps
    cam.width = 0
    with pytest.raises(tb.TbvhError) as e:
        tb.host_viewer_generate(cam, 0, 1)
    assert e.value.code == -1


# ---- SampleSky -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", F.SKY_SHAPES)
def test_sky_equals_the_restatement_off_the_edges(viewer_oracle, shape):
    pixels = F.sky(shape)
    h, w = shape
    dirs, classes = F.sky_directions()
    for name in ("pole_up", "pole_down", "minus_x_plus_zero", "minus_x_minus_zero", "wrap", "atan2_zero_zero", "y_above_one", "nan", "random"):
        assert classes[name].size > 0, name
    got = tb.host_sky_sample(pixels, dirs)
    want, flags, ku, kv = viewer_oracle.sky(pixels, dirs, L.margins())
    idx, widx = bits(got[:, 3]), bits(want[:, 3])
    assert (idx < w * h).all()
    texels = pixels.reshape(-1, 3)
    assert np.array_equal(bits(got[:, :3]), bits(texels[idx][:, ::-1]))    # the texel as ( z, y, x )
    nan = (flags & L.SKY_NAN).astype(bool)
    assert np.array_equal(np.flatnonzero(nan), classes["nan"])
    edge = (flags & (L.SKY_EDGE_U | L.SKY_EDGE_V)).astype(bool)
    plain = ~edge & ~nan
    assert np.array_equal(idx[plain], widx[plain]), f"{int((idx[plain] != widx[plain]).sum())} directions off the edges differ"
    assert edge.sum() <= max(4, dirs.shape[0] // 200)
    # on an edge: u in { ku - 1, ku }, v in { kv - 1, kv }, whichever axis is flagged; the other axis as the restatement has it
    last = w * h - 1
    for i in np.flatnonzero(edge):
        u0, v0 = int(widx[i]) % w, int(widx[i]) // w
        us = {ku[i] - 1, ku[i]} if flags[i] & L.SKY_EDGE_U else {u0}
        vs = {kv[i] - 1, kv[i]} if flags[i] & L.SKY_EDGE_V else {v0}
        assert int(idx[i]) in {min(int(u + v * w), last) for u in us for v in vs} | {int(widx[i])}, (i, dirs[i])
    # a NaN converts to coordinate 0 on the axis it reaches; |D.y| beyond 1 is clamped: the poles' rows
    assert (idx[classes["nan"]] < w * h).all()
    up = classes["y_above_one"]
    assert (idx[up[[0, 2]]] // w == 0).all() and (idx[up[[1, 3]]] // w == (h - 1 if h > 1 else 0)).all()
    assert (flags[up] & L.SKY_CLAMPED_Y).all()
    # p = +-pi with D.x < 0 and D.z = +-0: the same column from both sides, the middle of the texture
    a, b = classes["minus_x_plus_zero"], classes["minus_x_minus_zero"]
    assert np.array_equal(idx[a] % w, idx[b] % w) and (np.abs(idx[a] % w - (w - 1) / 2) <= 0.5).all()


def test_no_sky_samples_zero_and_refusals():
    dirs, _ = F.sky_directions()
    out = tb.host_sky_sample(None, dirs)
    assert not out.any()
    for call in (lambda: tb.lib.tbvh_host_sky_sample(None, 4, 4, None, 0, None), lambda: tb.lib.tbvh_host_sky_sample(tb._ptr(F.sky((2, 2))), 0, 2, None, 0, None),
                 lambda: tb.lib.tbvh_host_sky_sample(tb._ptr(F.sky((2, 2))), 1 << 16, 1 << 16, None, 0, None)):
        assert call() == -1


def test_sky_prepare_is_the_two_passes_of_load():
    rng = np.random.default_rng(4)
    raw = rng.uniform(0, 9, (3, 5, 3)).astype(np.float32)
    scale = np.array([1.0, 0.5, 2.0], np.float32)
    s = np.sqrt(raw)                                                       # (float32 sqrt is correctly rounded in NumPy as in sqrtf)
    assert np.array_equal(bits(tb.host_sky_prepare(raw, scale, from_hdr=True)), bits((s * s) * scale))
    assert np.array_equal(bits(tb.host_sky_prepare(raw, scale, from_hdr=False)), bits((raw * raw) * scale))
    assert np.array_equal(bits(tb.host_sky_prepare(raw)), bits(raw * raw))


def test_load_sky_bin(tmp_path):
    p = F.sky((3, 4))
    path = tmp_path / "sky.hdr.bin"
    with open(path, "wb") as f:
        f.write(np.array([4, 3], "<i4").tobytes()); f.write(p.tobytes())
    assert np.array_equal(tb.load_sky_bin(str(path)), p)
    with open(path, "wb") as f:
        f.write(np.array([4, 3], "<i4").tobytes()); f.write(p.tobytes()[:-4])
    with pytest.raises(ValueError):
        tb.load_sky_bin(str(path))


# ---- the stages on synthetic records -----------------------------------------------------------------------------------------------------------------------
def test_continue_shadow_rays_and_pack_equal_the_restatement(viewer_oracle):
    sc = F.scene()
    r, o, occ = F.synthetic_lighting_records()
    want_r, want_went = viewer_oracle.continue_(sc.materials, sc.n_textures, r, o)
    got_r = tb._aligned(r.copy())
    went = tb.host_viewer_continue(sc.materials, sc.n_textures, got_r, o)
    assert np.array_equal(went, want_went) and np.array_equal(bits(records(got_r)), bits(want_r))
    assert 20 < went.sum() < r.shape[0] // 2
    assert not went[r["t"] >= 10000].any() and not went[o[:, 3] < 0].any()
    stayed = ~went
    assert np.array_equal(records(got_r)[stayed], records(r)[stayed])
    assert (got_r["t"][went] == np.float32(1e30)).all() and not got_r["prim"][went].any()
    for light in (None, np.array([0.3, -0.2, 0.9], np.float32)):
        l = default_light() if light is None else light
        assert np.array_equal(bits(records(tb.host_viewer_shadow_rays(r, light))), bits(viewer_oracle.shadow_rays(r, l)))
    sh = tb.host_viewer_shadow_rays(r)
    null = r["t"] >= 10000
    assert null.sum() > 100 and (sh["t"][null] == 0).all() and (sh["t"][~null] == 1000).all()
    rgb = np.zeros((64, 4), np.float32)
    rgb[:, :3] = np.random.default_rng(1).uniform(-0.5, 1.5, (64, 3))
    rgb[0, :3] = [np.nan, np.inf, -np.inf]; rgb[1, :3] = [1.0, 0.99999994, 0.0]; rgb[2, :3] = [-1e30, 2.0, 1 / 255]
    got = tb.host_viewer_pack(rgb)
    assert np.array_equal(got, viewer_oracle.pack(rgb))
    assert got[1] == 255 + (254 << 8) and (got[0] & 0xFFFF) == 0xFFFF


@pytest.mark.parametrize("mode", [tb.VIEWER_GLTF, tb.VIEWER_FOLIAGE])
def test_light_equals_the_restatement_off_the_edges(viewer_oracle, mode):
    r, o, occ = F.synthetic_lighting_records()
    pixels = F.sky(F.FRAME_SKY)
    for sky in (pixels, None):
        for light in (None, np.array([0.3, -0.2, 0.9], np.float32)):
            got = tb.host_viewer_light(mode, sky, r, o, occ, light)
            want, edge = viewer_oracle.light(mode, sky, r, o, occ, default_light() if light is None else light, L.margins())
            differ = (bits(got) != bits(want)).any(1)
            assert not (differ & (edge == 0)).any(), f"{int((differ & (edge == 0)).sum())} records off the edges differ"
            assert differ.sum() <= 4
    wide = SF.ShadeScene.stride128(r)
    assert np.array_equal(bits(tb.host_viewer_light(mode, pixels, wide, o, occ)), bits(tb.host_viewer_light(mode, pixels, r, o, occ)))
    with pytest.raises(tb.TbvhError) as e:
        tb.host_viewer_light(2, pixels, r, o, occ)
    assert e.value.code == -1


# ---- the frames: restatement = real reference, host twins = restatement ---------------------------------------------------------------------------------
# ---- the goldens (tools/make_viewer_golden.py, from the real reference): what runs without the checkout ----------------------------------------------------
FRAMES = [(m, k) for m in ("gltf", "foliage") for k in ("tlas", "blas")]


def mode_of(name):
    return tb.VIEWER_GLTF if name == "gltf" else tb.VIEWER_FOLIAGE


@pytest.mark.parametrize("mode_name,kind", FRAMES)
def test_goldens_equal_the_restatement(viewer_oracle, mode_name, kind):
    """The per-ray sets: every 131st pixel of the reference's own 800 x 600 frame.  From the stored final records the restatement's colour equals the file's
    Trace in all bits and its pack equals WorkerThread's word, with no exceptions; the host twins equal both wherever SKY_EDGE is clear; the host generator's
    directions are the records'."""
    sc, sky, mode = F.scene(), F.sky(F.FRAME_SKY), mode_of(mode_name)
    g = L.golden(f"frame_{mode_name}_{kind}")
    verts, fat, inst, lib_inst = F.scene_kind(sc, kind)
    pix, rays, occ, buf = g["pix"], tb._aligned(g["rays"]), g["occ"], g["buf"].reshape(-1)
    assert buf.size == 480000 and np.array_equal(pix, np.arange(0, 480000, L.GOLDEN_STEP)) and rays.dtype == tb.RAY_DTYPE
    gen = tb.host_viewer_generate(sc.camera(800, 600))
    assert np.array_equal(bits(gen["D"][pix]), bits(rays["D"]))
    out = np.array(tb.host_shade_hits(sc.materials, sc.textures, fat, rays, lib_inst))
    o = occ if mode == tb.VIEWER_FOLIAGE else None
    want, edge = viewer_oracle.light(mode, sky, rays, out, o, default_light(), L.margins())
    assert np.array_equal(bits(want[:, :3]), bits(g["rgb"]))
    assert np.array_equal(viewer_oracle.pack(want), buf[pix])
    got = tb.host_viewer_light(mode, sky, rays, out, o)
    differ = (bits(got) != bits(want)).any(1)
    assert not (differ & (edge == 0)).any()
    assert np.array_equal(tb.host_viewer_pack(got)[~differ], buf[pix][~differ])
    hit = rays["t"] < 10000
    assert hit.sum() > 300 and (~hit).sum() > 300
    if mode == tb.VIEWER_GLTF:
        assert list(g["per_round"])[0] == 480000 and len(g["per_round"]) == 8 and (rays["O"] != rays["O"][0]).any()
    else:
        assert occ[hit].any() and not occ[hit].all()


def test_sky_golden_equals_the_restatement(viewer_oracle):
    """the file's SampleSky on the fixture's well-defined directions (poles, p = +-pi, the wrap, atan2( 0, 0 ), random) = the restatement's libm sky, all bits"""
    g = L.golden("sky")
    dirs, classes = F.sky_directions()
    ok = g["defined"]
    assert np.array_equal(ok, F.defined_directions(dirs)) and ok.sum() > 3000 and not ok[classes["nan"]].any() and not ok[classes["y_above_one"]].any()
    for name in ("pole_up", "pole_down", "minus_x_plus_zero", "minus_x_minus_zero", "wrap", "atan2_zero_zero"):
        assert ok[classes[name]].all(), name
    for h, w in F.SKY_SHAPES:
        want, _, _, _ = viewer_oracle.sky(F.sky((h, w)), dirs[ok], L.margins())
        assert np.array_equal(bits(want[:, :3]), bits(g[f"sky_{h}x{w}"])), (h, w)


@pytest.mark.parametrize("mode_name,kind", FRAMES)
def test_cpu_frame_through_the_reference_build_equals_the_golden(reference, mode_name, kind):
    """The whole frame without the checkout: the host twins over oracle/_ref's traversal (the real tiny_bvh.h as the recipe under oracle/ builds it) give the
    golden buf on every pixel — the same frame tests/test_viewer_gpu.py holds the device against."""
    sc, sky, mode = F.scene(), F.sky(F.FRAME_SKY), mode_of(mode_name)
    g = L.golden(f"frame_{mode_name}_{kind}")
    verts, fat, inst, lib_inst = F.scene_kind(sc, kind)
    trace, occluded = L.reference_tracers(reference, verts, inst, kind)
    fr = L.cpu_frame(trace, occluded, sc, fat, lib_inst, sc.camera(800, 600), mode, sky)
    buf = g["buf"].reshape(-1)
    assert fr["per_round"] == list(g["per_round"])
    assert np.array_equal(fr["rays"][g["pix"]].view(np.uint32), g["rays"].view(np.uint32))
    assert np.array_equal(fr["pix"], buf), f"{int((fr['pix'] != buf).sum())} pixels of the CPU frame differ from the golden buf"


def test_reference_bvh_gpu_traversal_stays_inside_the_budget(reference):
    """the reference's own BVH_GPU traversal against its BVH::Intersect on the frame's camera rays: the records that differ (ties, edges) number at most
    max( 4, n // 4000 ), the budget tests/test_viewer_gpu.py gives the device frame"""
    sc = F.scene()
    rays = tb.host_viewer_generate(sc.camera(800, 600))
    n = rays.shape[0]
    for v in sc.verts:
        s = reference.build(v)
        a, b = s.intersect(1, rays), s.intersect(5, rays)
        differ = (a.view(np.uint32).reshape(n, 16) != b.view(np.uint32).reshape(n, 16)).any(1)
        assert differ.sum() <= max(4, n // 4000), int(differ.sum())


def filled_instances(sc):
    inst = sc.instances.copy()
    SF.host_tlas(inst, sc.verts)                                           # (fills the bounds and the inverses in place)
    return inst


def cpu_frame(ref, sc, inst, cam, mode, sky, max_rounds=8):
    """tests/viewer_lib.py: cpu_frame with the REFERENCE's own traversal for every Intersect / IsOccluded"""
    fr = L.cpu_frame(ref.intersect, ref.occluded, sc, sc.fat, inst, cam, mode, sky, max_rounds)
    return fr["pix"], fr["rgb"], fr["rays"], fr["out"], fr["occ"], fr["per_round"]


@pytest.fixture(scope="module", params=["gltf", "foliage"])
def reference_frame(request, tmp_path_factory):
    ref = L.compile_ref_shim(tmp_path_factory.mktemp("viewer_ref_" + request.param), foliage=request.param == "foliage")
    if ref is None:
        pytest.skip(NO_REFERENCE)
    sc = F.scene()
    inst = filled_instances(sc)
    sky = F.sky(F.FRAME_SKY)
    ref.scene(inst, sc.verts, sc.fat, sc.materials, sc.textures, sky)
    yield request.param, ref, sc, inst, sky
    ref.release()


def test_frames_equal_the_real_reference(viewer_oracle, reference_frame):
    name, ref, sc, inst, sky = reference_frame
    mode = tb.VIEWER_GLTF if name == "gltf" else tb.VIEWER_FOLIAGE
    cam = sc.camera(800, 600)
    n = 800 * 600
    pix, rgb, rays, out, occ, per_round = cpu_frame(ref, sc, inst, cam, mode, sky)
    # the fixture's classes are present
    hit = rays["t"] < 10000
    assert hit.sum() > n // 10 and (~hit).sum() > n // 10 and set(np.unique(rays["inst"][hit])) == {0, 1, 2, 3, 4, 5}
    if mode == tb.VIEWER_GLTF:
        assert len(per_round) == 8 and all(a > b > 0 for a, b in zip(per_round, per_round[1:])), per_round   # the 8-round cap is reached, every round thins out
        moved = (rays["O"] != rays["O"][0]).any(1)
        assert (moved & ~hit).sum() > 100                                  # masked, then sky
        assert (moved & hit).sum() > 100
        last_masked = moved & hit & (out.view(np.uint32)[:, 11] == F.TEXEL_GLTF_MASKED)
        assert last_masked.sum() > 100                                     # the 8th masked layer, shaded as it is
        assert (out.view(np.uint32)[hit, 11] == F.TEXEL_FOLIAGE_MASKED).any()   # judged opaque here, masked by the other viewer
    else:
        assert per_round == [n] and occ[hit].any() and not occ[hit].all()  # a shadowed and a lit region
        assert (hit & (out[:, 3] == 0)).sum() > 100 and (hit & (out.view(np.uint32)[:, 11] == F.TEXEL_GLTF_MASKED) & (out[:, 3] == 1)).sum() > 100
    # restatement (libm sky) = the reference's Trace on every ray, zero exceptions
    want_rgb, edge = viewer_oracle.light(mode, sky, rays, out, occ, default_light(), L.margins())
    ref_rgb, ref_rays = ref.trace(tb.host_viewer_generate(cam))
    assert np.array_equal(bits(want_rgb[:, :3]), bits(ref_rgb)), f"{int((bits(want_rgb[:, :3]) != bits(ref_rgb)).any(1).sum())} rays differ from the reference's Trace"
    same = ref_rays["t"] != np.float32(1e34)                               # (the reference steps on once more after its 8th masked layer; the library keeps that hit)
    assert np.array_equal(bits(ref_rays["D"]), bits(rays["D"])) and np.array_equal(bits(ref_rays["O"][same]), bits(rays["O"][same]))
    assert np.array_equal(bits(ref_rays["t"][same]), bits(rays["t"][same])) and np.array_equal(ref_rays["prim"][same], rays["prim"][same])
    # ... and = WorkerThread's buf, pixel for pixel
    buf = ref.frame(cam).reshape(-1)
    assert np.array_equal(viewer_oracle.pack(want_rgb), buf)
    # host twins = restatement wherever SKY_EDGE is clear; the cap on the pixels that carry it
    differ = (bits(rgb) != bits(want_rgb)).any(1)
    flagged = edge != 0
    assert not (differ & ~flagged).any()
    assert flagged.sum() <= n // 2000, f"{int(flagged.sum())} pixels carry SKY_EDGE"
    assert (pix != buf).sum() <= differ.sum()
    if name == "gltf":                                                     # the file's own SampleSky on the fixture's well-defined directions
        dirs, classes = F.sky_directions()
        ok = F.defined_directions(dirs)
        for shape in F.SKY_SHAPES:
            want_sky, _, _, _ = viewer_oracle.sky(F.sky(shape), dirs[ok], L.margins())
            assert np.array_equal(bits(want_sky[:, :3]), bits(ref.sky(F.sky(shape), dirs[ok])))
            assert np.array_equal(bits(ref.sky(F.sky(shape), dirs[ok])), bits(L.golden("sky")[f"sky_{shape[0]}x{shape[1]}"]))
    assert np.array_equal(buf, L.golden(f"frame_{name}_tlas")["buf"].reshape(-1))
    print(f"viewer frame {name}: {int(flagged.sum())} of {n} pixels carry SKY_EDGE, {int(differ.sum())} differ from the libm sky, rays per round {per_round}")
