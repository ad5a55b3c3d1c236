"""BVH_DOUBLE scenes on the GPU against the restated oracle (tests/oracle_double.c) under the library's tie rule: every record must come
back byte-identical (prim and inst exact, t / u / v bit-identical, misses untouched), every occlusion bit equal."""
import ctypes as C
import os

import numpy as np
import pytest

import tinybvh_amd as tb
from tinybvh_amd import lib, rays as R, scenes
from double_lib import bounce_rays_dbl, camera_rays_dbl, instance_scene, odbl, random_rays_dbl, rotated_soup, to_dbl  # noqa: F401 (odbl: fixture)

pytestmark = pytest.mark.gpu

SHIFT = np.array([1.3e7, 4.0e6, -7.0e6])


@pytest.fixture(scope="module")
def ctx():
    c = tb.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def atrium_f32():
    return scenes.atrium(262_267, seed=1)


def same_records(got: np.ndarray, want: np.ndarray, what: str):
    a = np.ascontiguousarray(got).view(np.uint8).reshape(-1, 128); b = np.ascontiguousarray(want).view(np.uint8).reshape(-1, 128)
    bad = np.nonzero((a != b).any(1))[0]
    assert bad.size == 0, f"{what}: {bad.size} of {got.shape[0]} records differ, first {bad[:5].tolist()}: got {got[bad[:2]]} want {want[bad[:2]]}"


def check_blas(ctx, odbl, verts, rays, what, occ_tmax=None):
    sc = tb.BVH_Double(ctx).Build(verts)
    nodes, idx = sc.host.nodes(), sc.host.prim_idx()
    want = odbl.intersect(nodes, idx, verts, rays, rule=1)
    got = sc.Intersect(rays.copy())
    same_records(got, want, what + " Intersect")
    sh = rays.copy()
    if occ_tmax is not None:
        sh["t"] = occ_tmax
    occ = sc.IsOccluded(sh)
    occ_want = odbl.occluded(nodes, idx, verts, sh, rule=1)
    assert np.array_equal(occ, occ_want), f"{what} IsOccluded: {int((occ != occ_want).sum())} differ"
    hits = int((want["t"] < 1e299).sum())
    assert hits > rays.shape[0] // 10, (what, hits)
    return sc, want


def test_atrium_double(ctx, odbl, atrium_f32):
    verts = to_dbl(atrium_f32)
    eye, view = scenes.SPONZA_CAMERAS[0]
    cam = camera_rays_dbl(eye, view, 256, 128)
    sc, traced = check_blas(ctx, odbl, verts, cam, "atrium camera", occ_tmax=30.0)
    check_blas(ctx, odbl, verts, bounce_rays_dbl(traced), "atrium bounce", occ_tmax=8.0)
    assert sc.device_bytes > 0 and lib.tbvh_scene_layout(sc._h) == tb.LAYOUT_BVH_DOUBLE


def test_atrium_far_from_origin(ctx, odbl, atrium_f32):
    """The atrium at 1/1000 scale, 1.3e7 units from the origin: fp32 spacing there is 1 unit, the scene is 0.07 units wide."""
    verts = to_dbl(atrium_f32) * 1e-3 + SHIFT
    assert np.unique(verts.astype(np.float32), axis=0).shape[0] < verts.shape[0] // 100   # (fp32 collapses the geometry to a few points)
    eye, view = scenes.SPONZA_CAMERAS[1]
    cam = camera_rays_dbl(eye, view, 256, 128, scale=1e-3, offset=SHIFT)
    sc, traced = check_blas(ctx, odbl, verts, cam, "shifted camera", occ_tmax=0.03)
    check_blas(ctx, odbl, verts, bounce_rays_dbl(traced, scale=1e-3), "shifted bounce", occ_tmax=0.008)


def test_rotated_soup(ctx, odbl):
    verts = rotated_soup(40_000)
    check_blas(ctx, odbl, verts, random_rays_dbl(32768, (-12, -12, -12), (12, 12, 12)), "rotated soup", occ_tmax=3.0)


def test_agrees_with_fp32_bvh_gpu(ctx, atrium_f32):
    """Float-exact vertices, the same rays: the fp64 path and the native BVH_GPU kernel report the same triangle for all but a few rays
    (those where fp32 and fp64 rounding decide an edge or a near tie differently)."""
    eye, view = scenes.SPONZA_CAMERAS[0]
    r32 = R.primary(R.camera(eye, view, 256, 256, 1, 1))
    g = tb.BVH_GPU(ctx).Build(atrium_f32)
    g.set_variant(1)
    h32 = g.Intersect(r32.copy())
    rd = tb.make_rays_ex(r32["O"].astype(np.float64), r32["D"].astype(np.float64))
    d = tb.BVH_Double(ctx).Build(to_dbl(atrium_f32))
    hd = d.Intersect(rd)
    hit32, hitd = h32["t"] < 1e29, hd["t"] < 1e299
    diff = np.nonzero((hit32 != hitd) | (hit32 & hitd & (h32["prim"].astype(np.uint64) != hd["prim"])))[0]
    print(f"fp32 / fp64 disagreements: {diff.size} of {r32.shape[0]}")
    for i in diff[:10]:
        print(f"  ray {i}: fp32 prim {h32['prim'][i]} t {h32['t'][i]!r}  fp64 prim {hd['prim'][i]} t {hd['t'][i]!r}")
    assert diff.size <= max(1, int(1e-4 * r32.shape[0])), diff[:20]


def test_tlas_instances(ctx, odbl):
    blas_verts, inst = instance_scene(500)
    blas = [tb.BVH_Double(ctx).Build(v) for v in blas_verts]
    tl = tb.TLAS_Double(ctx).Build(inst, blas)
    rays = random_rays_dbl(32768, (1.0e6 - 80, -2.0e6 - 80, 3.0e6 - 80), (1.0e6 + 80, -2.0e6 + 80, 3.0e6 + 80), seed=21)
    rays["mask"][::2] = 0x1   # half of the rays skip the instances with mask 0x2
    rays["instIdx"] = 7
    bl = [(b.host.nodes(), b.host.prim_idx(), b.verts) for b in blas]
    tn, ti = tl.host.nodes(), tl.host.prim_idx()
    want = odbl.intersect_tlas(tn, ti, inst, bl, rays, rule=1)
    got = tl.Intersect(rays.copy())
    same_records(got, want, "TLAS Intersect")
    hit = want["t"] < 1e299
    assert hit.sum() > 1000 and np.unique(want["inst"][hit]).size > 100
    masked = np.nonzero(inst["mask"] == 0x2)[0]
    assert not np.isin(want["inst"][hit & (rays["mask"] == 0x1)], masked).any()
    sh = rays.copy(); sh["t"] = 40.0
    occ = tl.IsOccluded(sh)
    occ_want = odbl.occluded_tlas(tn, ti, inst, bl, sh, rule=1)
    assert np.array_equal(occ, occ_want), int((occ != occ_want).sum())
    assert 0 < occ.sum() < occ.size


def chain_tree(lo: np.ndarray, hi: np.ndarray) -> np.ndarray:
    """Hand-made chain over len(lo) primitives with boxes [lo, hi]: every interior node has a leaf (primitive k) and the rest of the chain
    as children, so the tree is len(lo) - 1 levels deep; the root is 0, its children 1 and 2 as after the reference's builder."""
    n = lo.shape[0]
    nodes = np.zeros(2 * n - 1, tb.NODE_DBL_DTYPE)
    for k in range(n - 1):   # interior k at 2k (the root at 0), its leaf at 2k + 1, the rest of the chain at 2k + 2
        nodes[2 * k + 1]["aabbMin"], nodes[2 * k + 1]["aabbMax"], nodes[2 * k + 1]["leftFirst"], nodes[2 * k + 1]["triCount"] = lo[k], hi[k], k, 1
        nodes[2 * k]["leftFirst"] = 2 * k + 1
    nodes[2 * n - 2]["aabbMin"], nodes[2 * n - 2]["aabbMax"], nodes[2 * n - 2]["leftFirst"], nodes[2 * n - 2]["triCount"] = lo[n - 1], hi[n - 1], n - 1, 1
    for k in reversed(range(n - 1)):
        c = 2 * k + 1
        nodes[2 * k]["aabbMin"] = np.minimum(nodes[c]["aabbMin"], nodes[c + 1]["aabbMin"])
        nodes[2 * k]["aabbMax"] = np.maximum(nodes[c]["aabbMax"], nodes[c + 1]["aabbMax"])
    return nodes


def chain_scene(depth: int):
    """A chain `depth` levels deep over big triangles in the planes z = 0 .. depth."""
    n_tris = depth + 1
    verts = np.zeros((n_tris, 3, 3))
    for k in range(n_tris):
        verts[k] = [[-2.0, -2.0, k], [4.0, -2.0, k], [-2.0, 4.0, k]]
    tri = verts
    nodes = chain_tree(tri.min(1), tri.max(1))
    return nodes, np.arange(n_tris, dtype=np.uint64), verts.reshape(-1, 3)


def test_deep_chain_uses_the_spill_area(ctx, odbl):
    nodes, idx, verts = chain_scene(220)
    sc = tb.BVH_Double(ctx).Upload(nodes, idx, verts)
    rng = np.random.default_rng(4)
    n = 4096
    O = np.stack([rng.uniform(-1.5, 0.5, n), rng.uniform(-1.5, 0.5, n), np.full(n, 400.0)], 1)
    D = np.tile([0.0, 0.0, -1.0], (n, 1)) + np.concatenate([rng.normal(0, 1e-4, (n, 2)), np.zeros((n, 1))], 1)
    rays = tb.make_rays_ex(O, D)
    want = odbl.intersect(nodes, idx, verts, rays, rule=1)
    assert (want["prim"] == 220).mean() > 0.9   # the top plane, found after the whole chain has been pushed
    same_records(sc.Intersect(rays.copy()), want, "chain Intersect")
    sh = rays.copy(); sh["t"] = 150.0
    assert np.array_equal(sc.IsOccluded(sh), odbl.occluded(nodes, idx, verts, sh, rule=1))


def test_axis_parallel_face_and_short_tmax(ctx, odbl):
    verts = to_dbl(scenes.atrium(60_000, seed=3))
    sc = tb.BVH_Double(ctx).Build(verts)
    nodes, idx = sc.host.nodes(), sc.host.prim_idx()
    rng = np.random.default_rng(9)
    n = 8192
    # axis-parallel directions (rD = +-inf, NaN products where the origin lies on a slab plane), origins on node box faces
    axes = np.eye(3)[rng.integers(0, 3, n)] * rng.choice([-1.0, 1.0], (n, 1))
    pick = rng.integers(1, len(nodes), n)
    corner = np.where(rng.random((n, 3)) < 0.5, nodes["aabbMin"][pick], nodes["aabbMax"][pick])
    O = np.where(rng.random((n, 3)) < 0.5, corner, rng.uniform(-30, 30, (n, 3)))
    rays = tb.make_rays_ex(O, axes)
    assert np.isinf(rays["rD"]).any()
    want = odbl.intersect(nodes, idx, verts, rays, rule=1)
    same_records(sc.Intersect(rays.copy()), want, "axis-parallel Intersect")
    assert np.array_equal(sc.IsOccluded(rays), odbl.occluded(nodes, idx, verts, rays, rule=1))
    short = rays.copy(); short["t"] = 1e-9
    short["u"] = 0.25; short["prim"] = 12345   # a miss leaves every byte as it was (a few origins are triangle corners: hits at t < 1e-9)
    want = odbl.intersect(nodes, idx, verts, short, rule=1)
    miss = want["t"] == 1e-9
    assert miss.mean() > 0.9 and want[miss].tobytes() == short[miss].tobytes()
    same_records(sc.Intersect(short.copy()), want, "short tmax Intersect")


@pytest.mark.parametrize("n", [0, 1, 63, 65, 1 << 20])
def test_batch_sizes(ctx, odbl, n):
    big = test_batch_sizes.__dict__.setdefault("scene", None)
    if big is None:
        v = to_dbl(scenes.street(1_050_000, seed=2))
        sc = tb.BVH_Double(ctx).Build(v)
        big = test_batch_sizes.__dict__["scene"] = (v, sc)
    v, sc = big
    rays = random_rays_dbl(n, (-60, 0.5, -10), (60, 12, 10), seed=n + 1)
    got = sc.Intersect(rays.copy())
    occ = sc.IsOccluded(rays)
    if n == 0:
        return
    step = 64 if n > 4096 else 1
    want = odbl.intersect(sc.host.nodes(), sc.host.prim_idx(), v, rays[::step], rule=1)
    same_records(got[::step], want, f"batch {n}")
    assert np.array_equal(occ[::step], odbl.occluded(sc.host.nodes(), sc.host.prim_idx(), v, rays[::step], rule=1))


def test_device_resident_queries(ctx, odbl):
    verts = rotated_soup(5000, seed=5)
    sc = tb.BVH_Double(ctx).Build(verts)
    rays = random_rays_dbl(10000, (-12, -12, -12), (12, 12, 12), seed=3)
    d = ctx.malloc(rays.nbytes); docc = ctx.malloc(rays.shape[0])
    try:
        ctx.to_device(d, rays)
        sc.occluded_device(d, rays.shape[0], docc)
        sc.intersect_device(d, rays.shape[0])
        out = np.zeros_like(rays); occ = np.zeros(rays.shape[0], np.uint8)
        ctx.from_device(out, d); ctx.from_device(occ, docc)
    finally:
        ctx.free(d); ctx.free(docc)
    same_records(out, odbl.intersect(sc.host.nodes(), sc.host.prim_idx(), verts, rays, rule=1), "device Intersect")
    assert np.array_equal(occ, odbl.occluded(sc.host.nodes(), sc.host.prim_idx(), verts, rays, rule=1))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def _upload_rc(ctx, nodes, n_nodes, idx, verts, n_tris):
    h = C.c_void_p()
    rc = lib.tbvh_upload_bvh_double(ctx._h, nodes.ctypes.data, n_nodes, idx.ctypes.data, idx.size, verts.ctypes.data, n_tris, C.byref(h))
    if rc == 0:
        lib.tbvh_free_scene(h)
    return rc, lib.tbvh_last_error().decode()


def test_malformed_blobs_are_refused(ctx):
    verts = rotated_soup(200, seed=1)
    host = tb.host_build_double(verts)
    nodes, idx = host.nodes().copy(), host.prim_idx().copy()
    assert _upload_rc(ctx, nodes, len(nodes), idx, verts, 200)[0] == 0
    interior = int(np.nonzero(nodes["triCount"] == 0)[0][0]); leaf = int(np.nonzero(nodes["triCount"] > 0)[0][0])
    cases = []
    n = nodes.copy(); n[interior]["leftFirst"] = len(nodes) - 1; cases.append(("child", n, len(nodes), idx, 200, f"node {interior}"))
    n = nodes.copy(); n[leaf]["leftFirst"] = idx.size - 1; n[leaf]["triCount"] = 2; cases.append(("leaf range", n, len(nodes), idx, 200, f"node {leaf}"))
    i = idx.copy(); i[17] = 200; cases.append(("primIdx", nodes, len(nodes), i, 200, "primIdx[17]"))
    cases.append(("2^32 nodes", nodes, 1 << 32, idx, 200, "4294967296 nodes"))
    cases.append(("no nodes", nodes, 0, idx, 200, "empty"))
    for what, n, nn, i, nt, msg in cases:
        rc, err = _upload_rc(ctx, n, nn, i, verts, nt)
        assert rc == -5 and msg in err, (what, rc, err)
    # TLAS: blasIdx beyond the BLAS list, instance index beyond the instances
    blas = tb.BVH_Double(ctx).Build(verts)
    inst = tb.make_instances_ex(np.tile(np.eye(4), (4, 1, 1)), 0)
    th = tb.host_build_tlas_double(inst, blas.bounds[None, :])
    tn, ti = th.nodes().copy(), th.prim_idx().copy()
    arr = (C.c_void_p * 1)(blas._h)
    def tl_rc(inst_, ti_):
        h = C.c_void_p()
        rc = lib.tbvh_upload_tlas_double(ctx._h, tn.ctypes.data, len(tn), ti_.ctypes.data, ti_.size, inst_.ctypes.data, inst_.shape[0], arr, 1, C.byref(h))
        if rc == 0:
            lib.tbvh_free_scene(h)
        return rc, lib.tbvh_last_error().decode()
    assert tl_rc(inst, ti)[0] == 0
    bad = inst.copy(); bad["blasIdx"][2] = 1
    rc, err = tl_rc(bad, ti); assert rc == -5 and "instance 2: blasIdx 1" in err, err
    bi = ti.copy(); bi[0] = 4
    rc, err = tl_rc(inst, bi); assert rc == -5 and "primIdx[0] = 4 >= n_inst" in err, err


def test_other_entry_points_refuse_double_scenes(ctx):
    verts = rotated_soup(300, seed=2)
    sc = tb.BVH_Double(ctx).Build(verts)
    inst = tb.make_instances_ex(np.eye(4)[None], 0)
    tl = tb.TLAS_Double(ctx).Build(inst, [sc])
    r32 = R.random_rays(64, (-5, -5, -5), (5, 5, 5))
    v4 = np.zeros((900, 4), np.float32)
    d = ctx.malloc(64 * 128); dout = ctx.malloc(64)
    s = sc._h
    arr = (C.c_void_p * 1)(s)
    hint = (C.c_uint8 * 8)()
    buf = np.zeros(1 << 16, np.uint8)
    nb = C.c_uint64(0)
    wf = tb.Wavefront(ctx, 64, 64)
    cam = R.camera((0, 0, -20), (0, 0, 1), 64, 64, 1, 1)
    params = tb._capi.WfParams()
    try:
        calls = {
            "tbvh_intersect": lambda h: lib.tbvh_intersect(h, r32.ctypes.data, 64, 64),
            "tbvh_occluded": lambda h: lib.tbvh_occluded(h, r32.ctypes.data, 64, 64, buf.ctypes.data),
            "tbvh_intersect_device": lambda h: lib.tbvh_intersect_device(h, d, 64),
            "tbvh_intersect_device_fresh": lambda h: lib.tbvh_intersect_device_fresh(h, d, 64, 1e30),
            "tbvh_occluded_device": lambda h: lib.tbvh_occluded_device(h, d, 64, dout),
            "tbvh_intersect_sharded": lambda h: lib.tbvh_intersect_sharded((C.c_void_p * 1)(h), 1, r32.ctypes.data, 64, 64),
            "tbvh_occluded_sharded": lambda h: lib.tbvh_occluded_sharded((C.c_void_p * 1)(h), 1, r32.ctypes.data, 64, 64, buf.ctypes.data),
            "tbvh_intersect_sharded_device": lambda h: lib.tbvh_intersect_sharded_device((C.c_void_p * 1)(h), 1, (C.c_void_p * 1)(d), (C.c_uint64 * 1)(64), 1, 1e30, None, None),
            "tbvh_occluded_sharded_device": lambda h: lib.tbvh_occluded_sharded_device((C.c_void_p * 1)(h), 1, (C.c_void_p * 1)(d), (C.c_uint64 * 1)(64), (C.c_void_p * 1)(dout), None, None),
            "tbvh_refit": lambda h: lib.tbvh_refit(h, v4.ctypes.data, 300, 0),
            "tbvh_update_bvh_gpu": lambda h: lib.tbvh_update_bvh_gpu(h, buf.ctypes.data, 1, buf.ctypes.data, 1, v4.ctypes.data, 1),
            "tbvh_update_bvh4_gpu": lambda h: lib.tbvh_update_bvh4_gpu(h, buf.ctypes.data, 4),
            "tbvh_update_cwbvh": lambda h: lib.tbvh_update_cwbvh(h, buf.ctypes.data, 5, buf.ctypes.data, 3),
            "tbvh_update_tlas": lambda h: lib.tbvh_update_tlas(h, buf.ctypes.data, 1, buf.ctypes.data, 1, buf.ctypes.data, 1),
            "tbvh_set_opacity_micromaps": lambda h: lib.tbvh_set_opacity_micromaps(h, buf.ctypes.data, 1, 300, 0),
            "tbvh_scene_download": lambda h: lib.tbvh_scene_download(h, 0, None, 0, C.byref(nb)),
            "tbvh_cwbvh_set_hybrid": lambda h: lib.tbvh_cwbvh_set_hybrid(h, 0),
            "tbvh_scene_get_schedule_hint": lambda h: lib.tbvh_scene_get_schedule_hint(h, C.cast(hint, C.c_void_p)),
            "tbvh_scene_set_schedule_hint": lambda h: lib.tbvh_scene_set_schedule_hint(h, C.cast(hint, C.c_void_p)),
            "tbvh_upload_tlas (double BLAS)": lambda h: lib.tbvh_upload_tlas(ctx._h, buf.ctypes.data, 1, buf.ctypes.data, 1, buf.ctypes.data, 1, (C.c_void_p * 1)(h), 1, C.byref(C.c_void_p())),
            "tbvh_rebuild_tlas_device": lambda h: lib.tbvh_rebuild_tlas_device(h, None, 0, None, 0),
            "tbvh_tlas_download": lambda h: lib.tbvh_tlas_download(h, None, 0, None, 0, None, 0, C.byref(nb)),
            "tbvh_wavefront_render": lambda h: lib.tbvh_wavefront_render(wf._h, h, v4.ctypes.data, C.byref(cam), C.byref(params), None),
        }
        for name, call in calls.items():
            for h in (sc._h, tl._h):
                assert call(h) == -1, (name, h == tl._h)
        # ... and the RayEx queries refuse an fp32 scene
        g = tb.BVH_GPU(ctx).Build(scenes.soup(100))
        rx = tb.make_rays_ex(np.zeros((4, 3)), np.ones((4, 3)))
        assert lib.tbvh_intersect_ex(g._h, rx.ctypes.data, 4) == -1 and b"BVH_DOUBLE" in lib.tbvh_last_error()
        assert lib.tbvh_occluded_ex(g._h, rx.ctypes.data, 4, buf.ctypes.data) == -1
        assert lib.tbvh_intersect_ex_device(g._h, d, 4) == -1
        assert lib.tbvh_occluded_ex_device(g._h, d, 4, dout) == -1
        # the double scenes still answer afterwards
        got = sc.Intersect(random_rays_dbl(256, (-12, -12, -12), (12, 12, 12)))
        assert (got["t"] < 1e299).any()
    finally:
        wf.close()
        ctx.free(d); ctx.free(dout)


def test_tlas_stack_overflow_is_an_error_not_a_wild_access(odbl):
    """A TLAS chain 40 levels deep over instances of a BLAS chain 30 levels deep, traced with a stack of 18 entries (TBVH_SPILL_ENTRIES=2):
    rays travelling in -z leave one pending TLAS leaf per level and enter the instances with the stack full.  The query must end in
    TBVH_E_FORMAT ("traversal stack overflow"), the other direction (far subtrees pushed one at a time) must still be right, and the context
    must trace correctly afterwards."""
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
        bn, bi, bv = chain_scene(30)
        blas = tb.BVH_Double(c).Upload(bn, bi, bv)
        n_inst = 41
        T = np.tile(np.eye(4), (n_inst, 1, 1))
        T[:, 2, 3] = 100.0 * np.arange(n_inst)
        inst = tb.make_instances_ex(T, 0)
        tb.host_build_tlas_double(inst, blas.bounds[None, :])   # (fills invTransform and the instance boxes, BLASInstanceEx::Update)
        tn, ti = chain_tree(inst["aabbMin"], inst["aabbMax"]), np.arange(n_inst, dtype=np.uint64)
        tl = tb.TLAS_Double(c).Upload(tn, ti, inst, [blas])
        rng = np.random.default_rng(8)
        n = 256
        xy = np.stack([rng.uniform(-1.5, 0.5, n), rng.uniform(-1.5, 0.5, n)], 1)
        bl = [(bn, bi, bv)]
        errors = 0
        for z0, dz in ((100.0 * n_inst + 50.0, -1.0), (-50.0, 1.0)):
            rays = tb.make_rays_ex(np.concatenate([xy, np.full((n, 1), z0)], 1), np.tile([1e-5, 2e-5, dz], (n, 1)))
            for query in ("Intersect", "IsOccluded"):
                try:
                    if query == "Intersect":
                        same_records(tl.Intersect(rays.copy()), odbl.intersect_tlas(tn, ti, inst, bl, rays, rule=1), f"dz {dz} Intersect")
                    else:
                        assert np.array_equal(tl.IsOccluded(rays), odbl.occluded_tlas(tn, ti, inst, bl, rays, rule=1))
                    assert dz > 0, "the -z direction must overflow an 18-entry stack"
                except tb.TbvhError as e:
                    assert dz < 0 and e.code == -5 and "stack overflow" in str(e), e
                    errors += 1
        assert errors == 2
        # the context is usable afterwards
        verts = rotated_soup(2000, seed=3)
        sc = tb.BVH_Double(c).Build(verts)
        rays = random_rays_dbl(4096, (-12, -12, -12), (12, 12, 12), seed=9)
        same_records(sc.Intersect(rays.copy()), odbl.intersect(sc.host.nodes(), sc.host.prim_idx(), verts, rays, rule=1), "after overflow")
    finally:
        c.close()
