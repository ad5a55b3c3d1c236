"""The device SAH builder over boxes (tbvh_build_bvh2_sah_device_aabbs, tbvh_build_device_custom_spheres_sah, the TLAS rebuild behind
tbvh_tlas_set_builder with the device Aila-Laine encode; csrc/kernels_sahbuild.hip) and its
one-workgroup path (k_sah_one_group, tbvh_debug_set_sah_one_group) against the sequential CPU twins over the same csrc/sah_split.h and against the
recorded reference trees of tests/golden/boxbuild: byte for byte.  The twins themselves are held to the real reference in
tests/test_boxbuild_host.py (DESIGN.md par. 20).  No test here feeds NaNs: termination on such input is shown on the twin, which shares the header."""
import ctypes as C

import numpy as np
import pytest

import tinybvh_amd as tb
import boxbuild_lib as bl
import sahbuild_lib as sl
from custom_dynamic_lib import check_boxes, check_structure
from custom_lib import cu_oracle, decorate, mismatches, rays_for  # noqa: F401  (cu_oracle: fixture)

pytestmark = pytest.mark.gpu
lib = tb.lib
INVALID = -1
FORCED = 1 << 14   # csrc/sahbuild.h: kSahOneGroupMax: every set here goes through the one-workgroup kernel
_twin = {}


def twin(kind, name, k=0):
    """the host twin's tree of a set, built once"""
    if (kind, name, k) not in _twin:
        _twin[(kind, name, k)] = (tb.host_build_bvh2_sah_boxes(bl.boxes(name), max_leaf=k) if kind == "boxes"
                                  else tb.host_build_bvh2_sah_spheres(bl.spheres(name), max_leaf=k))
    return _twin[(kind, name, k)]


def same(got, want, what):
    assert got[0].shape == want[0].shape, f"{what}: {got[0].shape[0]} nodes on the device, {want[0].shape[0]} on the host"
    if not np.array_equal(got[0], want[0]):
        bad = np.nonzero((got[0] != want[0]).any(axis=1))[0]
        raise AssertionError(f"{what}: {bad.size} of {got[0].shape[0]} nodes differ, first {bad[0]}: {got[0][bad[0]]} != {want[0][bad[0]]}")
    assert np.array_equal(got[1], want[1]), f"{what}: primIdx differs"


@pytest.fixture
def paths(ctx):
    """sets the one-workgroup threshold and the small-subtree threshold of the shared context for one test and puts both back"""
    saved = (C.c_uint32 * 2)()
    tb.check(lib.tbvh_debug_get_sah_thresholds(ctx._h, saved), "tbvh_debug_get_sah_thresholds")

    def set_(one_group, small_subtree=64):
        tb.check(lib.tbvh_debug_set_sah_one_group(ctx._h, one_group), "tbvh_debug_set_sah_one_group")
        tb.check(lib.tbvh_debug_set_sah_small_subtree(ctx._h, small_subtree), "tbvh_debug_set_sah_small_subtree")
    yield set_
    set_(saved[1], saved[0])


PATHS = {"one_group": (FORCED, 64), "levels_T0": (0, 0), "levels_T64": (0, 64)}


# ---- boxes ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", bl.SETS)
def test_box_tree_is_the_twin_s_and_the_recorded_reference_tree(ctx, paths, name, path):
    paths(*PATHS[path])
    got = tb.build_bvh2_sah_boxes(ctx, bl.boxes(name))
    same(got, twin("boxes", name), f"{name}, {path}")
    bl.assert_matches_golden(f"boxes_{name}", got[0], got[1], f"device, {path}")
    assert ctx.time_last_ms() > 0


def test_default_context_builds_the_same_tree(ctx):
    for name in ("MIXED65", "MIXED1000", "GEO256"):
        same(tb.build_bvh2_sah_boxes(ctx, bl.boxes(name)), twin("boxes", name), name)


def test_switch_between_the_paths(ctx, paths):
    """n = L builds in one workgroup, n = L + 1 by the levels: the same trees as with the other path"""
    paths(256)
    for n in (255, 256, 257):
        b = np.array(bl.boxes("MIXED1000")[:n])
        same(tb.build_bvh2_sah_boxes(ctx, b), tb.host_build_bvh2_sah_boxes(b), f"first {n} of MIXED1000, L = 256")


@pytest.mark.parametrize("path", ["one_group", "levels_T64"])
@pytest.mark.parametrize("k", [1, 3])
def test_split_leafs_over_boxes(ctx, paths, path, k):
    paths(*PATHS[path])
    for name in ("IDENT700", "MIXED1000", "MIXED3"):
        same(tb.build_bvh2_sah_boxes(ctx, bl.boxes(name), max_leaf=k), twin("boxes", name, k), f"{name}, SplitLeafs({k}), {path}")


@pytest.mark.parametrize("path", ["one_group", "levels_T64"])
def test_everything_on_the_device(ctx, paths, path):
    paths(*PATHS[path])
    b = bl.boxes("MIXED1025")
    n = b.shape[0]
    d_b = ctx.malloc(b.nbytes); d_n = ctx.malloc(2 * n * 32); d_i = ctx.malloc(n * 4)
    try:
        ctx.to_device(d_b, b)
        nn = C.c_uint64(0)
        tb.check(lib.tbvh_build_bvh2_sah_device_aabbs(ctx._h, C.c_void_p(d_b), n, 1, 0, C.c_void_p(d_n), 2 * n, C.c_void_p(d_i), n, 1, C.byref(nn)),
                 "tbvh_build_bvh2_sah_device_aabbs")
        want = twin("boxes", "MIXED1025")
        assert nn.value == want[0].shape[0]
        nodes = np.zeros((nn.value, 8), np.uint32); idx = np.zeros(n, np.uint32)
        ctx.from_device(nodes, d_n); ctx.from_device(idx, d_i)
        same((nodes, idx), want, f"MIXED1025, device in and out, {path}")
        same(tb.build_bvh2_sah_boxes(ctx, (d_b, n)), want, f"MIXED1025, device in, host out, {path}")
    finally:
        for d in (d_b, d_n, d_i):
            ctx.free(d)


# ---- triangles: the triangle path shares the new kernel ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["SOUP500", "FLAT", "QUADS"])
def test_triangles_in_one_workgroup_match_the_recorded_reference_tree(ctx, paths, name):
    paths(FORCED)
    nodes, idx = tb.build_bvh2_sah(ctx, sl.scene(name))
    sl.assert_matches_golden(name, nodes, idx, "device, one workgroup")
    same(tb.build_bvh2_sah(ctx, sl.scene(name), max_leaf_tris=3), tb.host_build_bvh2_sah(sl.scene(name), max_leaf_tris=3), f"{name}, SplitLeafs(3)")


# ---- spheres ---------------------------------------------------------------------------------------------------------------------------------
def _rays(sph):
    return np.concatenate([decorate(rays_for(sph, 8192, 17, k), 17 + i) for i, k in enumerate(("camera", "incoherent"))])


@pytest.mark.parametrize("path", ["one_group", "levels_T64"])
@pytest.mark.parametrize("name", bl.SETS)
def test_sphere_scene_is_the_twin_s_and_the_recorded_reference_tree(ctx, paths, name, path):
    paths(*PATHS[path])
    sph = bl.spheres(name)
    sc = tb.SphereBVH(ctx).BuildOnDevice(sph, builder="sah")
    try:
        assert lib.tbvh_scene_layout(sc._h) == tb.LAYOUT_BVH2_WALD
        nodes, pi, gathered = sc.Download()
        same((nodes, pi), twin("spheres", name), f"{name} as spheres, {path}")
        bl.assert_matches_golden(f"spheres_{name}", nodes, pi, f"device, {path}")
        assert np.array_equal(gathered.view(np.uint32), sph[pi].view(np.uint32))
    finally:
        sc.free()


def test_sphere_queries_rebuild_and_refit(ctx, paths, cu_oracle):
    """hit parity with the restated sphere oracle over the downloaded arrays, byte for byte; a rebuild after motion equals a fresh build of the moved
    set, and a TLAS over the scene traces the new tree without a new upload; a refit passes the box checks"""
    paths(FORCED)
    sph = np.array(bl.spheres("MIXED1000"))
    sc = tb.SphereBVH(ctx).BuildOnDevice(sph, builder="sah")
    fresh = None
    try:
        nodes, pi, _ = sc.Download()
        check_structure(nodes, pi, sph.shape[0], sph.shape[0]); check_boxes(nodes, pi, sph)
        rays = _rays(sph)
        want, _ = cu_oracle.intersect(nodes, pi, sph, rays, rule=1)
        assert mismatches(sc.Intersect(rays.copy()), want) == 0
        assert np.array_equal(sc.IsOccluded(rays), cu_oracle.occluded(nodes, pi, sph, rays, rule=1))
        assert (want["t"] < np.float32(1e30)).sum() > 1000
        inst = tb.make_instances(np.eye(4, dtype=np.float32)[None], [0])
        tlas = tb.TLAS(ctx).Build(inst, [sc])
        # motion, then a rebuild in place with the builder the scene remembers
        rng = np.random.default_rng(5)
        moved = sph.copy()
        moved[:, :3] += rng.normal(0, 2.0, (sph.shape[0], 3)).astype(np.float32)
        sc.RebuildOnDevice(moved)
        nodes2, pi2, gathered2 = sc.Download()
        fresh = tb.SphereBVH(ctx).BuildOnDevice(moved, builder="sah")
        same((nodes2, pi2), fresh.Download()[:2], "rebuilt in place against a fresh SAH build")
        same((nodes2, pi2), tb.host_build_bvh2_sah_spheres(moved), "rebuilt in place against the twin")
        assert np.array_equal(gathered2.view(np.uint32), moved[pi2].view(np.uint32))
        rays2 = _rays(moved)
        want2, _ = cu_oracle.intersect(nodes2, pi2, moved, rays2, rule=1)
        assert mismatches(sc.Intersect(rays2.copy()), want2) == 0
        tlas.RebuildOnDevice()                 # (the instance box follows the new root box; no new upload of the BLAS)
        got_t = tlas.Intersect(rays2.copy())   # (identity instance 0: the same records, inst = 0)
        assert np.array_equal(got_t["t"], want2["t"]) and np.array_equal(got_t["prim"], want2["prim"])
        tlas.free()
        # a refit keeps the topology and gives every node the box of its spheres
        again = moved.copy()
        again[:, :3] += rng.normal(0, 0.3, (sph.shape[0], 3)).astype(np.float32)
        sc.Refit(again)
        nodes3, pi3, _ = sc.Download()
        assert np.array_equal(nodes3[:, 3], nodes2[:, 3]) and np.array_equal(nodes3[:, 7], nodes2[:, 7]) and np.array_equal(pi3, pi2)
        check_boxes(nodes3, pi3, again)
    finally:
        sc.free()
        if fresh is not None:
            fresh.free()


def test_sphere_split_leafs_and_device_resident_spheres(ctx, paths):
    paths(FORCED)
    sph = bl.spheres("IDENT700")
    d = ctx.malloc(sph.nbytes)
    try:
        ctx.to_device(d, sph)
        sc = tb.SphereBVH(ctx).BuildOnDevice((d, sph.shape[0]), builder="sah", max_leaf=4)
        nodes, pi, _ = sc.Download()
        same((nodes, pi), twin("spheres", "IDENT700", 4), "IDENT700 as spheres, SplitLeafs(4), device-resident")
        check_structure(nodes, pi, 700, 4)
        sc.free()
    finally:
        ctx.free(d)


# ---- refusals and accounting -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_and_the_scene_answering(ctx, cu_oracle):
    b = bl.boxes("MIXED65"); sph = bl.spheres("MIXED65")
    n = b.shape[0]
    nn = C.c_uint64(0)
    out = C.c_void_p()
    f = lib.tbvh_build_bvh2_sah_device_aabbs
    for args in ((None, b.ctypes.data, n, 0, 0, None, 0, None, 0, 0, C.byref(nn)), (ctx._h, None, n, 0, 0, None, 0, None, 0, 0, C.byref(nn)),
                 (ctx._h, b.ctypes.data, n, 0, 0, None, 0, None, 0, 0, None), (ctx._h, b.ctypes.data, 0, 0, 0, None, 0, None, 0, 0, C.byref(nn)),
                 (ctx._h, b.ctypes.data, 1 << 31, 0, 0, None, 0, None, 0, 0, C.byref(nn))):
        assert f(*args) == INVALID and b"tbvh_build_bvh2_sah_device_aabbs" in lib.tbvh_last_error()
    # the count alone, then a capacity that is too small: the need is reported, nothing is written
    assert f(ctx._h, b.ctypes.data, n, 0, 0, None, 0, None, 0, 0, C.byref(nn)) == 0
    need = nn.value
    assert need == twin("boxes", "MIXED65")[0].shape[0]
    nodes = np.zeros((need - 1, 8), np.uint32); idx = np.zeros(n, np.uint32)
    nn.value = 0
    assert f(ctx._h, b.ctypes.data, n, 0, 0, nodes.ctypes.data, need - 1, idx.ctypes.data, n, 0, C.byref(nn)) == INVALID
    assert nn.value == need and not nodes.any()
    g = lib.tbvh_build_device_custom_spheres_sah
    for args in ((None, sph.ctypes.data, n, 0, 0, C.byref(out)), (ctx._h, None, n, 0, 0, C.byref(out)), (ctx._h, sph.ctypes.data, n, 0, 0, None),
                 (ctx._h, sph.ctypes.data, 0, 0, 0, C.byref(out)), (ctx._h, sph.ctypes.data, 1 << 31, 0, 0, C.byref(out)),
                 (ctx._h, sph.ctypes.data, n, 0, 5, C.byref(out))):
        assert g(*args) == INVALID and b"tbvh_build_device_custom_spheres_sah" in lib.tbvh_last_error()
    assert lib.tbvh_debug_set_sah_one_group(None, 4) == INVALID and b"tbvh_debug_set_sah_one_group" in lib.tbvh_last_error()
    # the triangle calls on an SAH-built sphere scene, and a rebuild with another count: refused, and the scene answers as before
    sc = tb.SphereBVH(ctx).BuildOnDevice(sph, builder="sah")
    try:
        nodes, pi, _ = sc.Download()
        v = np.zeros((3, 4), np.float32)
        assert lib.tbvh_refit(sc._h, v.ctypes.data, 1, 0) == INVALID and b"tbvh_refit" in lib.tbvh_last_error()
        assert lib.tbvh_rebuild_custom_spheres_device(sc._h, sph.ctypes.data, n - 1, 0) == INVALID
        rays = decorate(rays_for(sph, 1000, 17, "camera"), 17)
        want, _ = cu_oracle.intersect(nodes, pi, sph, rays, rule=1)
        assert mismatches(sc.Intersect(rays.copy()), want) == 0
    finally:
        sc.free()
    same(tb.build_bvh2_sah_boxes(ctx, b), twin("boxes", "MIXED65"), "after the errors")


def test_scene_bytes_count_the_sah_scratch_and_freeing_returns_everything(paths):
    """a context of its own, so that the counters of tbvh_debug_device_allocations start and end at the same values"""
    def allocations():
        out = (C.c_uint64 * 2)()
        tb.check(lib.tbvh_debug_device_allocations(out), "tbvh_debug_device_allocations")
        return out[0], out[1]
    c = tb.Context(0)
    try:
        sph = bl.spheres("MIXED1000")
        n = sph.shape[0]
        tb.SphereBVH(c).BuildOnDevice(sph, builder="sah").free()   # (what a context allocates for itself on first use is there before the counters are read)
        before = allocations()
        for one_group in (0, FORCED):
            tb.check(lib.tbvh_debug_set_sah_one_group(c._h, one_group), "tbvh_debug_set_sah_one_group")
            sc = tb.SphereBVH(c).BuildOnDevice(sph, builder="sah")
            # 2 n nodes, n records, primIdx, and the builder's scratch (fragments, both index arrays, temporary nodes, sort keys: well above 100 bytes a sphere)
            assert sc.device_bytes >= 2 * n * 32 + n * 32 + n * 4 + n * 100
            tb.build_bvh2_sah_boxes(c, bl.boxes("MIXED1025"))   # (transient: everything goes with the call)
            assert allocations()[1] - before[1] == sc.device_bytes
            sc.free()
            assert allocations() == before
    finally:
        c.close()


# ---- TLAS: tbvh_tlas_set_builder( tlas, 2 ) --------------------------------------------------------------------------------------------------
from tinybvh_amd import rays as R  # noqa: E402
from tinybvh_amd import scenes  # noqa: E402
from test_tlas import check as check_records, grid_instances, oracle_tlas  # noqa: E402


def _two_small_blases(ctx):
    """two BLASes whose root boxes are declared as boxbuild_lib.BLAS_BOUNDS (what the fixtures' instance records were updated with)"""
    blas = [tb.BVH8_CWBVH(ctx).Build(scenes.soup(40, seed=1)), tb.BVH8_CWBVH(ctx).Build(scenes.soup(40, seed=2))]
    for b, box in zip(blas, bl.BLAS_BOUNDS):
        b._bounds = box.copy()
    return blas


def _same_records(a, b):
    for fld in ("transform", "invTransform", "aabbMin", "aabbMax", "blasIdx", "mask"):
        assert np.array_equal(np.ascontiguousarray(a[fld]).view(np.uint32), np.ascontiguousarray(b[fld]).view(np.uint32)), fld


@pytest.mark.parametrize("path", ["one_group", "levels_T64"])
@pytest.mark.parametrize("n", bl.TLAS_SIZES)
def test_sah_tlas_download_is_the_twin_s_and_the_recorded_reference_tree(ctx, paths, n, path):
    paths(*PATHS[path])
    want_inst = bl.instances(n)
    inst = tb.make_instances(np.array(want_inst["transform"]), np.array(want_inst["blasIdx"]))
    blas = _two_small_blases(ctx)
    tlas = tb.TLAS(ctx).Build(inst, blas)
    d_t = ctx.malloc(n * 64)
    try:
        lbvh0 = tlas.RebuildOnDevice().Download()
        want = tb.host_build_tlas_sah(want_inst)
        ctx.to_device(d_t, np.ascontiguousarray(want_inst["transform"]))
        for how, args in (("None", ()), ("host", (np.array(want_inst["transform"]),)), ("device", (d_t, True))):   # transforms: kept, from the host, from the device
            nodes, idx, dev_inst = tlas.RebuildOnDevice(*args, builder="sah").Download()
            same((nodes, idx), want, f"SAH TLAS over {n} instances, transforms {how}, {path}")
            bl.assert_matches_golden(f"tlas_{n}", nodes, idx, f"device, {path}")
            _same_records(dev_inst, want_inst)
        assert tlas.device_bytes >= nodes.shape[0] * 64 + n * 4 + n * 192 + n * 100   # (the SAH scratch is counted)
        # back to builder 0: today's LBVH bytes again
        back = tlas.RebuildOnDevice(builder="lbvh").Download()
        assert back[0].shape[0] == 2 * n - 1
        for a, b in zip(back, lbvh0):
            assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
    finally:
        ctx.free(d_t)
        tlas.free()
        for b in blas:
            b.free()


def _tlas_rays():
    cam = R.primary(R.camera((-6.0, 3.0, -5.0), (0.62, -0.1, 0.62), 128, 64, 1, 1))
    return np.concatenate([cam, R.random_rays(8192, (-2, -2, -2), (8, 8, 8), seed=6)])


@pytest.mark.parametrize("layout", [tb.LAYOUT_BVH_GPU, tb.LAYOUT_BVH4_GPU, tb.LAYOUT_CWBVH])
def test_sah_tlas_traces_what_the_oracle_traces(ctx, oracle, layout):
    """Intersect / IsOccluded through the device-built SAH TLAS against the oracle over the host-built TLAS, with the comparison of
    tests/test_tlas_device_build.py; then over the downloaded SAH tree itself"""
    verts = scenes.blob(3000, seed=3)
    verts2 = scenes.soup(1000, seed=9, extent=1.6, size=0.25); verts2[:, :3] -= 0.8
    cls = tb.LAYOUT_CLASSES[layout]
    blas = [cls(ctx).Build(verts), cls(ctx).Build(verts2)]
    inst = grid_instances(4, 0.55, 2, n_blas=2)
    inst["transform"][::9, 0:3] *= 3.0   # some instances three times as wide: boxes of mixed sizes
    tlas = tb.TLAS(ctx).Build(inst, blas)
    try:
        rays = _tlas_rays()
        want = oracle_tlas(oracle, tlas, blas, rays)
        tlas.RebuildOnDevice(builder="sah")
        nodes, idx, dev_inst = tlas.Download()
        same((nodes, idx), tb.host_build_tlas_sah(dev_inst), f"SAH TLAS, layout {layout}")
        c = check_records(tlas.Intersect(rays.copy()), want)
        assert c["hits"] > 1000, c
        occ = tlas.IsOccluded(rays.copy())
        assert int((occ.astype(bool) != (want["t"] < 1e30)).sum()) <= 2
        # moved instances, transforms from the host
        inst2 = inst.copy()
        inst2["transform"][:, 3] += 0.37; inst2["transform"][:, 11] -= 0.21
        tlas.RebuildOnDevice(inst2["transform"])
        ref = tb.TLAS(ctx).Build(inst2.copy(), blas)
        check_records(tlas.Intersect(rays.copy()), oracle_tlas(oracle, ref, blas, rays))
        ref.free()
    finally:
        tlas.free()
        for b in blas:
            b.free()


def test_sah_tlas_with_a_sphere_blas_mixed_in(ctx):
    """hit records do not depend on the TLAS's shape: the SAH tree answers as the LBVH tree over the same records does"""
    sph = np.array(bl.spheres("MIXED65")); sph[:, :3] *= 0.02; sph[:, 3] *= 0.05
    blas = [tb.BVH8_CWBVH(ctx).Build(scenes.blob(1500, seed=5)), tb.SphereBVH(ctx).BuildOnDevice(sph, builder="sah")]
    inst = grid_instances(3, 0.5, 4, n_blas=2)
    tlas = tb.TLAS(ctx).Build(inst, blas)
    try:
        rays = _tlas_rays()
        tlas.RebuildOnDevice()
        lb, lb_occ = tlas.Intersect(rays.copy()), tlas.IsOccluded(rays.copy())
        tlas.RebuildOnDevice(builder="sah")
        nodes, idx, dev_inst = tlas.Download()
        same((nodes, idx), tb.host_build_tlas_sah(dev_inst), "SAH TLAS with a sphere BLAS")
        got = tlas.Intersect(rays.copy())
        for fld in ("t", "prim", "inst"):
            assert np.array_equal(got[fld], lb[fld]), fld
        assert np.array_equal(tlas.IsOccluded(rays.copy()), lb_occ)
        assert (got["t"] < 1e30).sum() > 500
    finally:
        tlas.free()
        for b in blas:
            b.free()


def test_tlas_builder_refusals(ctx):
    blas = _two_small_blases(ctx)
    inst = tb.make_instances(np.array(bl.instances(3)["transform"]), [0, 1, 0])
    tlas = tb.TLAS(ctx).Build(inst, blas)
    try:
        for scene, builder in ((blas[0]._h, 2), (tlas._h, 1), (tlas._h, 3), (None, 2)):
            assert lib.tbvh_tlas_set_builder(scene, builder) == INVALID and b"tbvh_tlas_set_builder" in lib.tbvh_last_error()
        with pytest.raises(ValueError):
            tlas.SetBuilder("ploc")
        nodes, idx, _ = tlas.RebuildOnDevice(builder="sah").Download()   # the TLAS answers on
        same((nodes, idx), tb.host_build_tlas_sah(bl.instances(3)), "after the refusals")
    finally:
        tlas.free()
        for b in blas:
            b.free()
