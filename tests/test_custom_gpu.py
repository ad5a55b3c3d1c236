"""Custom-geometry sphere BLASes on the GPU (DESIGN.md par. 12): every record byte for byte against the library-rule restatement
(tests/oracle_custom.c), BLAS and TLAS, and every refusal."""
import ctypes as C
import os

import numpy as np
import pytest

import tinybvh_amd as tb
from custom_lib import GOLDEN, caterpillar, cu_oracle, decorate, mismatches, rays_for, shadow_rays, sphere_set  # noqa: F401
from test_custom_host import anim_scene, tlas_rays

pytestmark = pytest.mark.gpu
lib = tb.lib


@pytest.fixture(scope="module")
def ctx():
    c = tb.Context(0)
    yield c
    c.close()


def _rays(spheres, seed, n=4000):
    return np.concatenate([decorate(rays_for(spheres, n, seed, k), seed + i) for i, k in enumerate(("camera", "incoherent", "inside"))])


def _check_blas(ctx, cu_oracle, nodes, pi, sph, rays, scene=None):
    sc = scene or tb.SphereBVH(ctx).Upload(nodes, pi, sph)
    want, _ = cu_oracle.intersect(nodes, pi, sph, rays, rule=1)
    got = sc.Intersect(rays.copy())
    assert mismatches(got, want) == 0
    occ_want = cu_oracle.occluded(nodes, pi, sph, rays, rule=1)
    assert np.array_equal(sc.IsOccluded(rays), occ_want)
    sh = shadow_rays(want, sph[:, :3].mean(0) + np.float32(25))
    assert np.array_equal(sc.IsOccluded(sh), cu_oracle.occluded(nodes, pi, sph, sh, rule=1))
    return sc, want


@pytest.mark.parametrize("name", ["bunny", "soup", "atrium", "one", "dups"])
def test_host_built(ctx, cu_oracle, name):
    sph = sphere_set(name)
    nodes, pi = tb.host_build_custom_spheres(sph)
    sc, want = _check_blas(ctx, cu_oracle, nodes, pi, sph, _rays(sph, 17))
    assert tb.lib.tbvh_scene_layout(sc._h) == tb.LAYOUT_BVH2_WALD
    assert (want["t"] < np.float32(1e30)).sum() > 0
    sc.free()


@pytest.mark.parametrize("path", sorted(p for p in os.listdir(GOLDEN) if p.startswith("blas")) if os.path.isdir(GOLDEN) else [])
def test_reference_goldens(ctx, cu_oracle, path):
    """reference-built trees: the device = the library-rule restatement byte for byte, and = the reference's records wherever the rules agree"""
    g = np.load(os.path.join(GOLDEN, path))
    rays = g["rays"].view(tb.RAY_DTYPE).reshape(-1)
    sc, want = _check_blas(ctx, cu_oracle, g["nodes"], g["prim_idx"], g["spheres"], rays)
    ref = g["hits"].view(tb.RAY_DTYPE).reshape(-1)
    agree = (ref["prim"] == want["prim"]) & (ref["t"] == want["t"])
    assert agree.mean() > 0.99
    assert mismatches(sc.Intersect(rays.copy())[agree], ref[agree]) == 0
    assert np.array_equal(sc.IsOccluded(rays), g["occluded"])
    sc.free()


def test_deeper_than_lds(ctx, cu_oracle):
    nodes, pi, sph = caterpillar(100)
    O = np.tile(np.array([[-10.0, 0.0, 0.0]], np.float32), (256, 1)); O[:, 1:] += np.linspace(-0.5, 0.5, 256, dtype=np.float32)[:, None]
    r = tb.make_rays(O, np.tile(np.array([[1.0, 0.0, 0.0]], np.float32), (256, 1)))
    want, depth = cu_oracle.intersect(nodes, pi, sph, r, rule=1)
    assert depth == 100
    sc = tb.SphereBVH(ctx).Upload(nodes, pi, sph)
    assert mismatches(sc.Intersect(r.copy()), want) == 0
    sc.free()


def test_2_24_rays_host_device_fresh(ctx, cu_oracle):
    """one call over 2^24 rays, from host arrays; then device arrays, the fresh variant"""
    sph = sphere_set("soup")[:256]
    nodes, pi = tb.host_build_custom_spheres(sph)
    sc = tb.SphereBVH(ctx).Upload(nodes, pi, sph)
    n = 1 << 24
    rays = tb.make_rays(np.random.default_rng(1).uniform(-12, 12, (n, 3)), np.random.default_rng(2).normal(size=(n, 3)))
    want, _ = cu_oracle.intersect(nodes, pi, sph, rays, rule=1)
    assert mismatches(sc.Intersect(rays.copy()), want) == 0
    small = decorate(rays[:200_000], 3)
    want, _ = cu_oracle.intersect(nodes, pi, sph, small, rule=1)
    d = ctx.malloc(small.nbytes)
    try:
        ctx.to_device(d, small); sc.intersect_device(d, small.shape[0]); ctx.synchronize()
        got = np.empty_like(small); ctx.from_device(got, d)
        assert mismatches(got, want) == 0
        f = small.copy(); f["t"] = np.float32(6.0); f["u"] = 0; f["v"] = 0; f["prim"] = 0
        wantf, _ = cu_oracle.intersect(nodes, pi, sph, f, rule=1)
        ctx.to_device(d, small); sc.intersect_device_fresh(d, small.shape[0], 6.0); ctx.synchronize()
        ctx.from_device(got, d)
        hit = wantf["t"] < np.float32(6.0)
        assert mismatches(got[hit], wantf[hit]) == 0
        assert np.array_equal(got["t"][~hit], wantf["t"][~hit]) and (got["prim"][~hit] == 0).all()
        o = ctx.malloc(small.shape[0])
        try:
            ctx.to_device(d, small); sc.occluded_device(d, small.shape[0], o); ctx.synchronize()
            occ = np.empty(small.shape[0], np.uint8); ctx.from_device(occ, o)
            assert np.array_equal(occ, cu_oracle.occluded(nodes, pi, sph, small, rule=1))
        finally:
            ctx.free(o)
    finally:
        ctx.free(d)
    sc.free()


def test_sharded_two_contexts(cu_oracle):
    sph = sphere_set("bunny")
    nodes, pi = tb.host_build_custom_spheres(sph)
    c1, c2 = tb.Context(0), tb.Context(0)
    try:
        a, b = tb.SphereBVH(c1).Upload(nodes, pi, sph), tb.SphereBVH(c2).Upload(nodes, pi, sph)
        rays = _rays(sph, 23)
        want, _ = cu_oracle.intersect(nodes, pi, sph, rays, rule=1)
        assert mismatches(tb.intersect_sharded([a, b], rays.copy()), want) == 0
        assert np.array_equal(tb.occluded_sharded([a, b], rays), cu_oracle.occluded(nodes, pi, sph, rays, rule=1))
        a.free(); b.free()
    finally:
        c1.close(); c2.close()


# ---- TLAS ------------------------------------------------------------------------------------------------------------------------------
def _tri_blas(ctx, layout, tris):
    return tb.LAYOUT_CLASSES[layout](ctx).Build(tris)


def _oracle_blas(sphere_scene, tri_scene, sph, tris):
    out = [("sph", sphere_scene.nodes, sphere_scene.prim_idx, sph)]
    if tri_scene is not None:
        h = tri_scene.host
        out.append(("tri", h.bvh2_nodes(), h.bvh2_prim_idx(), tris))
    return out


def _check_tlas(ctx, cu_oracle, tl, blas_desc, rays, exact):
    tn, ti = tl.host.blob(2, np.uint32, 8), tl.host.blob(1, np.uint32, 1)
    return _check_tlas_arrays(cu_oracle, tl, tn, ti, tl.instances, blas_desc, rays, exact)


def _check_tlas_arrays(cu_oracle, tl, tn, ti, inst, blas_desc, rays, exact):
    want = cu_oracle.tlas_intersect(tn, ti, inst, blas_desc, rays, rule=1)
    got = tl.Intersect(rays.copy())
    n_sph_inst = int((inst["blasIdx"] == 0).sum())
    sphere_hit = (want["t"] < np.float32(1e30)) & (want["inst"] < n_sph_inst)
    if exact:
        assert mismatches(got, want) == 0
    else:   # triangle hits as the TLAS tests compare them (DESIGN.md par. 4); sphere hits byte for byte
        assert mismatches(got[sphere_hit], want[sphere_hit]) == 0
        from oracle_lib import compare_hits
        c = compare_hits(got, want)
        assert c["hitmiss"] <= 2 and c["prim_real"] == 0 and c["t_bad"] == 0, c
    occ_want = cu_oracle.tlas_occluded(tn, ti, inst, blas_desc, rays, rule=1)
    occ = tl.IsOccluded(rays)
    assert (occ != occ_want).sum() <= (0 if exact else 2)
    return want


def test_tlas_spheres_only(ctx, cu_oracle):
    sph, _, inst = anim_scene()
    inst = inst[inst["blasIdx"] == 0].copy()
    s = tb.SphereBVH(ctx).Build(sph)
    tl = tb.TLAS(ctx).Build(inst, [s])
    rays = tlas_rays(3000, 31)
    _check_tlas(ctx, cu_oracle, tl, _oracle_blas(s, None, sph, None), rays, exact=True)
    tl.free(); s.free()


@pytest.mark.parametrize("layout", [tb.LAYOUT_BVH_GPU, tb.LAYOUT_BVH4_GPU, tb.LAYOUT_CWBVH])
def test_tlas_mixed(ctx, cu_oracle, layout):
    """tiny_bvh_anim.cpp's scene: scaled / rotated sphere instances, one triangle BLAS per layout, masks; then tbvh_update_tlas with moved
    instances and tbvh_rebuild_tlas_device"""
    sph, tris, inst = anim_scene()
    s = tb.SphereBVH(ctx).Build(sph)
    t = _tri_blas(ctx, layout, tris)
    tl = tb.TLAS(ctx).Build(inst, [s, t])
    rays = tlas_rays(3000, 37)
    desc = _oracle_blas(s, t, sph, tris)
    _check_tlas(ctx, cu_oracle, tl, desc, rays, exact=False)
    # tbvh_update_tlas: moved instances, host-built again
    inst2 = inst.copy()
    inst2["transform"][:, 3] += np.float32(0.75)
    tl.Build(inst2, [s, t])
    _check_tlas(ctx, cu_oracle, tl, desc, rays, exact=False)
    # tbvh_rebuild_tlas_device: the device rebuilds from the transforms; its tree is downloaded and restated
    xf = inst2["transform"].copy(); xf[:, 7] -= np.float32(0.5)
    tl.RebuildOnDevice(xf)
    nodes64, idx, inst3 = tl.Download()
    wald = _al_to_wald(nodes64)
    _check_tlas_arrays(cu_oracle, tl, wald, idx, inst3, desc, rays, exact=False)
    tl.free(); t.free(); s.free()


def _al_to_wald(al):
    """BVH_GPU (Aila-Laine) TLAS nodes as Wald nodes: every AL interior node's two children become a sibling pair"""
    al = np.ascontiguousarray(al, np.uint32).reshape(-1, 16)
    f = al.view(np.float32)
    out = [np.zeros(8, np.uint32), np.zeros(8, np.uint32)]
    stack = [(0, 0)]
    while stack:
        a, w = stack.pop()
        if al[a, 11]:   # leaf: triCount, firstTri
            out[w][3] = al[a, 15]; out[w][7] = al[a, 11]
            continue
        first = len(out)
        out[w][3] = first
        for k, (lo, hi, child) in enumerate(((0, 4, al[a, 3]), (8, 12, al[a, 7]))):
            n = np.zeros(8, np.uint32)
            n[0:3] = al[a, lo:lo + 3]; n[4:7] = al[a, hi:hi + 3]
            out.append(n)
            stack.append((int(child), first + k))
    # the root's box is never tested
    return np.array(out, np.uint32)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def _err(rc):
    return rc, tb.lib.tbvh_last_error().decode() if rc else ""   # (the message of the calling thread's last failure)


def test_refusals(ctx):
    """every entry point without a sphere form refuses a sphere BLAS with TBVH_E_INVALID and says why (TBVH_REFUSE_CUSTOM), before it touches
    memory: the pointers passed are real allocations all the same"""
    sph = sphere_set("soup")[:64]
    nodes, pi = tb.host_build_custom_spheres(sph)
    s = tb.SphereBVH(ctx).Upload(nodes, pi, sph)
    h = s._h
    v = np.ascontiguousarray(tb.scenes.soup(64, seed=1), np.float32)
    out = np.zeros(8, np.uint8)
    ex = np.zeros(8 * 128, np.uint8)
    hint = (C.c_uint8 * 64)()
    d_buf, d_occ = ctx.malloc(1 << 16), ctx.malloc(256)
    tl = tb.TLAS(ctx).Build(tb.make_instances(np.eye(4, dtype=np.float32)[None], [0]), [s])
    dn, di, dinst = np.zeros(64, np.uint8), np.zeros(1, np.uint64), np.zeros(320, np.uint8)
    one = (C.c_void_p * 1)(h)
    calls = {
        "tbvh_refit": lambda: lib.tbvh_refit(h, tb._ptr(v), 64, 0),
        "tbvh_update_bvh_gpu": lambda: lib.tbvh_update_bvh_gpu(h, tb._ptr(v), 1, tb._ptr(pi), pi.size, tb._ptr(v), 64),
        "tbvh_update_bvh4_gpu": lambda: lib.tbvh_update_bvh4_gpu(h, tb._ptr(v), 4),
        "tbvh_update_cwbvh": lambda: lib.tbvh_update_cwbvh(h, tb._ptr(v), 5, tb._ptr(v), 3),
        "tbvh_set_opacity_micromaps": lambda: lib.tbvh_set_opacity_micromaps(h, tb._ptr(np.zeros(64, np.uint32)), 1, 64, 0),
        "tbvh_scene_download": lambda: lib.tbvh_scene_download(h, 0, None, 0, None),
        "tbvh_scene_get_schedule_hint": lambda: lib.tbvh_scene_get_schedule_hint(h, C.cast(hint, C.c_void_p)),
        "tbvh_scene_set_schedule_hint": lambda: lib.tbvh_scene_set_schedule_hint(h, C.cast(hint, C.c_void_p)),
        "tbvh_cwbvh_set_hybrid": lambda: lib.tbvh_cwbvh_set_hybrid(h, 0),
        "tbvh_intersect_spheres": lambda: lib.tbvh_intersect_spheres(h, tb._ptr(sph), 8, tb._ptr(v), 64, tb._ptr(out)),
        "tbvh_intersect_spheres_device": lambda: lib.tbvh_intersect_spheres_device(h, C.c_void_p(d_buf), 8, C.c_void_p(d_buf), 64, C.c_void_p(d_occ)),
        "tbvh_intersect_ex": lambda: lib.tbvh_intersect_ex(h, tb._ptr(ex), 8),
        "tbvh_occluded_ex": lambda: lib.tbvh_occluded_ex(h, tb._ptr(ex), 8, tb._ptr(out)),
        "tbvh_intersect_ex_device": lambda: lib.tbvh_intersect_ex_device(h, C.c_void_p(d_buf), 8),
        "tbvh_occluded_ex_device": lambda: lib.tbvh_occluded_ex_device(h, C.c_void_p(d_buf), 8, C.c_void_p(d_occ)),
        "tbvh_wavefront_render": lambda: lib.tbvh_wavefront_render(None, h, None, None, None, None),
        "tbvh_wavefront_render (a TLAS with sphere BLASes)": lambda: lib.tbvh_wavefront_render(None, tl._h, None, None, None, None),
        "tbvh_upload_tlas_double": lambda: lib.tbvh_upload_tlas_double(ctx._h, tb._ptr(dn), 1, tb._ptr(di), 1, tb._ptr(dinst), 1, one, 1,
                                                                      C.byref(C.c_void_p())),
    }
    try:
        for name, f in calls.items():
            rc = f()
            msg = lib.tbvh_last_error().decode()
            assert rc == -1, (name, rc, msg)   # TBVH_E_INVALID
            assert "(custom geometry)" in msg and name.split(" ")[0] in msg, (name, msg)
        # a TLAS mixing sphere BLASes with voxel sets
        vox = tb.VoxelSet(ctx).Build(np.ones((4, 4, 4), np.uint32))
        inst = tb.make_instances(np.eye(4, dtype=np.float32)[None].repeat(2, 0), [0, 1])
        with pytest.raises(Exception, match="voxel sets only"):
            tb.TLAS(ctx).Build(inst, [s, vox])
        vox.free()
    finally:
        ctx.free(d_buf); ctx.free(d_occ)
        tl.free()
    s.free()


def test_malformed_blobs(ctx):
    sph = sphere_set("soup")[:200]
    nodes, pi = tb.host_build_custom_spheres(sph)

    def up(n, p, s):
        sc = tb.SphereBVH(ctx)
        with pytest.raises(Exception) as e:
            sc.Upload(n, p, s)
        return str(e.value)

    interior = int(np.nonzero(nodes[:, 7] == 0)[0][0])
    leaf = int(np.nonzero(nodes[:, 7] > 0)[0][0])
    bad = nodes.copy(); bad[interior, 3] = nodes.shape[0] - 1
    assert "beyond" in up(bad, pi, sph)                                   # child pair out of range
    bad = nodes.copy(); bad[leaf, 7] = pi.size + 5
    assert "exceeds" in up(bad, pi, sph)                                  # leaf range beyond n_idx
    badp = pi.copy(); badp[3] = sph.shape[0]
    assert "primIdx[3]" in up(nodes, badp, sph)                           # primitive beyond n_spheres
    bad = nodes.copy(); kids = int(nodes[0, 3]); bad[kids, 3] = 0; bad[kids, 7] = 0
    assert "twice" in up(bad, pi, sph)                                    # a cycle back to the root
    assert "twice" in up(np.tile(np.array([0, 0, 0, 1, 0, 0, 0, 0], np.uint32), (3, 1)), pi, sph)   # a shared child pair
    assert "32-bit" in _err(lib.tbvh_upload_custom_spheres(ctx._h, tb._ptr(nodes), 1 << 33, tb._ptr(pi), pi.size, tb._ptr(sph), 200,
                                                           C.byref(C.c_void_p())))[1]


def test_reference_golden_tlas(ctx, cu_oracle):
    """the anim-like golden: the reference's TLAS and triangle BLAS as BVH_GPU::ConvertFrom blobs, its sphere BVH as built; the device =
    the library-rule restatement (sphere hits byte for byte), and = the reference's records wherever the rules agree"""
    g = np.load(os.path.join(GOLDEN, "tlas_anim.npz"))
    inst = g["instances"].view(tb.INSTANCE_DTYPE).reshape(-1).copy()
    s = tb.SphereBVH(ctx).Upload(g["sph_nodes"], g["sph_idx"], g["spheres"])
    t = tb.BVH_GPU(ctx).Upload(g["tri_nodes64"], g["tri_idx"], g["tri_verts"])
    tl = tb.TLAS(ctx).Upload(g["tlas_nodes64"], g["tlas_idx"], inst, [s, t])
    tl.instances = inst
    rays = g["rays"].view(tb.RAY_DTYPE).reshape(-1)
    desc = [("sph", g["sph_nodes"], g["sph_idx"], g["spheres"]), ("tri", g["tri_nodes"], g["tri_idx"], g["tri_verts"])]
    want = _check_tlas_arrays(cu_oracle, tl, g["tlas_nodes"], g["tlas_idx"], inst, desc, rays, exact=False)
    ref = g["hits"].view(tb.RAY_DTYPE).reshape(-1)
    agree = (ref["prim"] == want["prim"]) & (ref["t"] == want["t"]) & (ref["inst"] == want["inst"]) & (ref["u"] == want["u"]) & (ref["v"] == want["v"])
    assert agree.mean() > 0.98
    got = tl.Intersect(rays.copy())
    sph_hit = agree & (want["t"] < np.float32(1e30)) & (want["inst"] < int((inst["blasIdx"] == 0).sum()))
    assert mismatches(got[sph_hit], ref[sph_hit]) == 0
    tl.free(); t.free(); s.free()


def test_tiny_hip_sphere_binding_runs():
    """tinyhip::SphereBVH built, uploaded and traced from C++ (examples/sphere_bvh.cpp, built by __graft_entry__.build())"""
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "_build", "sphere_bvh")
    if not os.path.exists(exe):
        pytest.skip("examples/_build/sphere_bvh not built (needs the reference header at build time)")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, check=True).stdout.split("\n")
    rows = [l.split() for l in out[:3]]
    assert [int(r[0]) for r in rows] == [1, 1, 3] and [int(r[2]) for r in rows] == [1, 1, 3]
    assert float(rows[1][1]) == pytest.approx(5 - np.sqrt(0.75), abs=1e-5) and float(rows[2][3]) == pytest.approx(29.5, abs=1e-5)
    assert out[3].split() == ["occ", "1", "handle", "1"]
