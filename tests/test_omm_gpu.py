"""Opacity micromaps baked on the device (tbvh_bake_opacity_micromaps / tbvh_bake_set_opacity_micromaps; DESIGN.md par. 15): the words equal the real
reference's (the goldens under tests/golden/omm at N = 4 and 32; the host function, which tests/test_omm_host.py pins to the reference, at N = 1, 2, 8, 64)
word for word — host- and device-resident sources, flat and indexed, at triangle counts that leave waves and workgroups partly filled and at one that makes
the grid-stride loop go round; nothing behind the output is written; baking onto a scene gives exactly the answers of the oracle run with the
reference-pinned maps, per layout and under a TLAS; a bad device-resident index is reported, never used as an address."""
import ctypes as C

import numpy as np
import pytest

import tinybvh_amd as tb
from tinybvh_amd import rays as R
from tinybvh_amd import scenes
import omm_lib as O
from test_opacity_micromaps import check

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, O.GOLDEN_TRIS]
GUARD = 64
_want = {}


def source():
    """the golden mesh in both forms: (uv flat, uv shared, indices, tri_texture, textures)"""
    g = O.golden(4)
    return g["uv"], g["uv_shared"], g["indices"], g["tri_texture"], [g["tex0"], g["tex1"]]


def want_words(N):
    """the reference's words for the golden mesh: the golden itself where there is one, else the host function"""
    if N not in _want:
        uv, _, _, tt, tex = source()
        _want[N] = O.golden(N)["words"] if N in O.GOLDEN_N else tb.host_bake_opacity_micromaps(uv, tex, N, tri_texture=tt)
    return _want[N]


class _Dev:
    """device copies of host arrays, freed together"""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def __call__(self, a):
        a = np.ascontiguousarray(a)
        d = self.ctx.malloc(max(a.nbytes, 16)); self.ctx.to_device(d, a)
        self.ptrs.append(d)
        return d

    def free(self):
        self.ctx.synchronize()
        for d in self.ptrs:
            self.ctx.free(d)


def device_source(dev, uv, tex, indices, tri_texture):
    n_tris = tri_texture.size
    return tb.device_omm_source(dev(uv), uv.shape[0], n_tris, [(dev(t), t.shape[1], t.shape[0]) for t in tex],
                                d_indices=dev(indices.reshape(-1)) if indices is not None else 0, d_tri_texture=dev(tri_texture))


def bake_guarded(ctx, N, n, uv, textures=None, indices=None, tri_texture=None):
    """bake n triangles into a device buffer with GUARD words behind it: (the words, the guard words afterwards)"""
    W = O.words_per_tri(N)
    buf = np.full(n * W + GUARD, 0xDEADBEEF, np.uint32)
    d = ctx.malloc(buf.nbytes); ctx.to_device(d, buf)
    tb.bake_opacity_micromaps(ctx, uv, textures, N=N, indices=indices, tri_texture=tri_texture, d_out=d)
    ctx.from_device(buf, d); ctx.free(d)
    return buf[:n * W].reshape(n, W), buf[n * W:]


@pytest.mark.parametrize("form", ["flat", "indexed"])
@pytest.mark.parametrize("resident", ["host", "device"])
@pytest.mark.parametrize("N", O.ALL_N)
def test_device_bake_equals_the_reference(ctx, N, resident, form):
    uv, uvi, idx, tt, tex = source()
    want = want_words(N)
    dev = _Dev(ctx)
    for n in SIZES:
        u, ix = (uv[:3 * n], None) if form == "flat" else (uvi, idx[:n])
        if resident == "host":
            got, guard = bake_guarded(ctx, N, n, u, tex, ix, tt[:n])
        else:
            got, guard = bake_guarded(ctx, N, n, device_source(dev, u, tex, ix, tt[:n]))
        assert (guard == 0xDEADBEEF).all(), (n, "words behind the output were written")
        assert np.array_equal(got, want[:n]), (n, int((got != want[:n]).any(1).sum()), "triangles differ")
    dev.free()


@pytest.mark.parametrize("N", [1, 4])
def test_more_triangle_groups_than_the_grid(ctx, N):
    """the grid is capped (32 one-wave workgroups per CU): 70 001 triangles at N = 1 (8 per wave) and at N = 4 (one per wave) make every workgroup take
    several groups; one texture, every triangle textured, tri_texture = NULL"""
    uv, _ = O.mesh(1200, seed=21)
    uv = np.ascontiguousarray(np.tile(uv.reshape(-1, 3, 2), (59, 1, 1))[:70_001].reshape(-1, 2))
    uv += np.repeat(np.arange(70_001, dtype=np.float32) % 7, 3)[:, None] * np.float32(0.03125)
    tex = O.textures()[1]
    want = tb.host_bake_opacity_micromaps(uv, tex, N)
    got, guard = bake_guarded(ctx, N, 70_001, uv, tex)
    assert (guard == 0xDEADBEEF).all() and np.array_equal(got, want)
    share, mixed, clear, full = O.map_stats(want, np.zeros(70_001, np.uint32), N)
    assert 0.2 < share < 0.8


def test_device_bake_is_timed_and_returns_words(ctx):
    uv, _, _, tt, tex = source()
    ctx.set_timing(True)
    got = tb.bake_opacity_micromaps(ctx, uv, tex, N=32, tri_texture=tt)
    assert np.array_equal(got, want_words(32)) and 0 < ctx.time_last_ms() < 1000


def test_one_by_one_textures(ctx):
    uv, _, _, tt, _ = source()
    tex = [np.array([[(3 << 24) | 0x123456]], np.uint32), np.array([[(2 << 24) | 0xFFFFFF]], np.uint32)]
    got = tb.bake_opacity_micromaps(ctx, uv, tex, N=8, tri_texture=tt)
    assert np.array_equal(got, tb.host_bake_opacity_micromaps(uv, tex, 8, tri_texture=tt))
    assert (got[tt == 0] == 0xFFFFFFFF).all() and not got[tt == 1].any()


# ---- end to end: the baked maps on a scene -------------------------------------------------------------------------------------------------
def small_scene(seed=3, n=6000):
    """a blob of about 6 000 triangles, UVs and texture indices for each of them, the two textures"""
    verts = scenes.blob(n, seed=seed)
    uv, tt = O.mesh(verts.shape[0] // 3, seed=seed + 40)
    return verts, uv, tt, O.textures()


@pytest.mark.parametrize("layout", [tb.LAYOUT_BVH_GPU, tb.LAYOUT_BVH4_GPU, tb.LAYOUT_CWBVH])
def test_baked_maps_answer_like_the_oracle(ctx, oracle, layout):
    N = 8
    verts, uv, tt, tex = small_scene()
    sc = tb.LAYOUT_CLASSES[layout](ctx).Build(verts)
    h = sc.host
    om = tb.host_bake_opacity_micromaps(uv, tex, N, tri_texture=tt)   # (pinned to the reference by tests/test_omm_host.py)
    lo, hi = verts[:, :3].min(0) - 0.3, verts[:, :3].max(0) + 0.3
    rays = R.random_rays(40_000, lo, hi, seed=5)
    plain = oracle.bvh2_intersect(h.bvh2_nodes(), h.bvh2_prim_idx(), verts, rays)
    sh = R.shadow(plain, hi * 1.5, 1e-5)
    plain_occ = oracle.bvh2_occluded(h.bvh2_nodes(), h.bvh2_prim_idx(), verts, sh)
    oracle.set_opmap(om, N)
    try:
        want = oracle.bvh2_intersect(h.bvh2_nodes(), h.bvh2_prim_idx(), verts, rays)
        want_occ = oracle.bvh2_occluded(h.bvh2_nodes(), h.bvh2_prim_idx(), verts, sh)
    finally:
        oracle.set_opmap(None, 0)
    changed = int(((want["prim"] != plain["prim"]) | (want["t"] != plain["t"])).sum())
    assert changed >= 0.02 * rays.shape[0], changed        # at least 2 % of the rays change their answer against the plain scene
    assert int((want_occ != plain_occ).sum()) >= 0.02 * sh.shape[0]
    assert sc.BakeOpacityMicroMaps(uv, tex, N, tri_texture=tt) is None
    check(sc.Intersect(rays.copy()), want)
    assert int((sc.IsOccluded(sh).astype(bool) != want_occ.astype(bool)).sum()) <= 2
    # tbvh_bake_opacity_micromaps followed by tbvh_set_opacity_micromaps( on_device = 1 ) gives the same answers as the fused call
    fused = sc.Intersect(rays.copy())
    sc.SetOpacityMicroMaps(None, 0)                         # cleared: the plain answers again
    check(sc.Intersect(rays.copy()), plain)
    d = ctx.malloc(om.nbytes)
    tb.bake_opacity_micromaps(ctx, uv, tex, N=N, tri_texture=tt, d_out=d)
    tb.check(tb.lib.tbvh_set_opacity_micromaps(sc._h, C.c_void_p(d), N, om.shape[0], 1), "tbvh_set_opacity_micromaps")
    ctx.free(d)
    two_step = sc.Intersect(rays.copy())
    check(two_step, want)
    assert np.array_equal(two_step["t"], fused["t"])
    # baking again with another texture replaces the maps
    other = [tex[1], tex[0]]
    om2 = tb.host_bake_opacity_micromaps(uv, other, N, tri_texture=tt)
    assert not np.array_equal(om2, om)
    oracle.set_opmap(om2, N)
    try:
        want2 = oracle.bvh2_intersect(h.bvh2_nodes(), h.bvh2_prim_idx(), verts, rays)
    finally:
        oracle.set_opmap(None, 0)
    assert int((want2["prim"] != want["prim"]).sum()) > 100
    sc.BakeOpacityMicroMaps(uv, other, N, tri_texture=tt)
    check(sc.Intersect(rays.copy()), want2)
    sc.free()


def test_baked_maps_under_a_tlas(ctx, oracle):
    from test_tlas import grid_instances, oracle_tlas, check as check_tlas
    N = 8
    verts, uv, tt, tex = small_scene(seed=4, n=3000)
    blas = tb.BVH8_CWBVH(ctx).Build(verts)
    inst = grid_instances(3, 0.6, 5)
    tlas = tb.TLAS(ctx).Build(inst, [blas])                 # the TLAS is uploaded first: it sees the maps baked afterwards
    rays = R.random_rays(30_000, (-2, -2, -2), (6, 6, 6), seed=6)
    plain = oracle_tlas(oracle, tlas, [blas], rays)
    check_tlas(tlas.Intersect(rays.copy()), plain)
    blas.BakeOpacityMicroMaps(uv, tex, N, tri_texture=tt)
    oracle.set_opmap(tb.host_bake_opacity_micromaps(uv, tex, N, tri_texture=tt), N)
    try:
        want = oracle_tlas(oracle, tlas, [blas], rays)
    finally:
        oracle.set_opmap(None, 0)
    assert int(((want["prim"] != plain["prim"]) | (want["inst"] != plain["inst"])).sum()) >= 0.02 * rays.shape[0]
    check_tlas(tlas.Intersect(rays.copy()), want)
    blas.SetOpacityMicroMaps(None, 0)
    check_tlas(tlas.Intersect(rays.copy()), plain)
    tlas.free(); blas.free()


def test_refusals_on_scenes_that_take_no_maps(ctx):
    uv, _, _, tt, tex = source()
    verts = scenes.soup(300, seed=1)
    blas = tb.BVH8_CWBVH(ctx).Build(verts)
    tlas = tb.TLAS(ctx).Build(tb.make_instances(np.eye(4, dtype=np.float32)[None], [0]), [blas])
    dbl = tb.BVH_Double(ctx).Build(verts[:, :3])
    dense = np.zeros((8, 8, 8), np.uint8); dense[2:5, 2:5, 2:5] = 1
    vox = tb.VoxelSet(ctx).Build(dense)
    sph = tb.SphereBVH(ctx).Build(np.array([[0, 0, 0, 1], [3, 0, 0, 1]], np.float32))
    for sc in (tlas, dbl, vox, sph):
        with pytest.raises(tb.TbvhError) as e:
            sc.BakeOpacityMicroMaps(uv, tex, 4, tri_texture=tt)
        assert e.value.code == -1, type(sc).__name__
    for bad_n in (0, 5, 128):
        with pytest.raises(tb.TbvhError) as e:
            blas.BakeOpacityMicroMaps(uv, tex, bad_n, tri_texture=tt)
        assert e.value.code == -1
    bad = tt.copy(); bad[7] = 2
    with pytest.raises(tb.TbvhError) as e:                  # host-resident: refused before anything is launched
        tb.bake_opacity_micromaps(ctx, uv, tex, N=4, tri_texture=bad)
    assert e.value.code == -1 and "triangle 7" in str(e.value)
    for sc in (tlas, dbl, vox, sph, blas):
        sc.free()


# ---- last: device-resident arrays with an index that is no UV and a texture index that is no texture -------------------------------------------
def test_bad_device_indices_are_reported_and_never_used(ctx):
    """The kernel clamps a corner index to the last UV and takes a bad texture index as no texture before it forms an address (both stay inside the arrays
    that were passed): the words are those of the repaired source, the status word is raised, and the fused call reports TBVH_E_FORMAT and installs nothing."""
    N = 8
    _, uvi, idx, tt, tex = source()
    bad_idx = idx.copy(); bad_idx[40, 1] = uvi.shape[0] + 5; bad_idx[200, 0] = 0xFFFFFFFF
    bad_tt = tt.copy(); bad_tt[100] = 2; bad_tt[201] = 0xFFFFFFFE
    fixed_idx = np.minimum(bad_idx, uvi.shape[0] - 1).astype(np.uint32)
    fixed_tt = bad_tt.copy(); fixed_tt[[100, 201]] = O.NO_TEXTURE
    want = tb.host_bake_opacity_micromaps(uvi, tex, N, indices=fixed_idx, tri_texture=fixed_tt)
    verts = scenes.soup(tt.size, seed=2)
    sc = tb.BVH8_CWBVH(ctx).Build(verts)
    rays = R.random_rays(5000, verts[:, :3].min(0) - 0.3, verts[:, :3].max(0) + 0.3, seed=8)
    plain = sc.Intersect(rays.copy())
    dev = _Dev(ctx)
    got, guard = bake_guarded(ctx, N, tt.size, device_source(dev, uvi, tex, bad_idx, bad_tt))   # (asynchronous: the status word stays raised ...)
    assert (guard == 0xDEADBEEF).all() and np.array_equal(got, want)
    with pytest.raises(tb.TbvhError) as e:                                                       # (... until a call that reads it)
        sc.BakeOpacityMicroMaps(device_source(dev, uvi, tex, bad_idx, bad_tt), None, N)
    assert e.value.code == -5 and "micromap" in str(e.value)
    assert np.array_equal(sc.Intersect(rays.copy())["t"], plain["t"]), "nothing was installed"
    sc.BakeOpacityMicroMaps(device_source(dev, uvi, tex, idx, tt), None, N)   # the status word was reported once and is clear again
    assert int((sc.Intersect(rays.copy())["t"] != plain["t"]).sum()) > 50
    dev.free(); sc.free()
