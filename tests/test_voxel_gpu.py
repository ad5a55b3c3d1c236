"""VoxelSet scenes on the GPU (kernels_voxel.hip) against the restatement (tests/oracle_voxel.c) under the library's acceptance rule (rule 1):
every record must come back byte-identical (t bit for bit, prim, inst, u / v and misses untouched), every occlusion byte equal.  Where the
reference's own behaviour (rule 0) agrees with rule 1, the records must also equal the goldens the real reference wrote
(tests/golden/voxels, tools/make_voxel_golden.py); every ray where the two rules part is a finite-tmax, nearer-hit or equal-t case."""
import ctypes as C
import os

import numpy as np
import pytest

import tinybvh_amd as tb
from tinybvh_amd import lib, rays as R, scenes
from voxel_lib import GOLDEN, hit_bytes, scene_dense, vox_oracle, voxel_rays   # noqa: F401 (vox_oracle: fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = tb.Context(0)
    yield c
    c.close()


def golden(case):
    return np.load(os.path.join(GOLDEN, case + ".npz"))


def same_hits(got, want, what):
    a, b = hit_bytes(got), hit_bytes(want)
    bad = np.nonzero((a != b).any(1))[0]
    assert bad.size == 0, f"{what}: {bad.size} of {got.shape[0]} records differ, first {bad[:5].tolist()}: got {a[bad[:2]]} want {b[bad[:2]]}"


def deviation_report(what, rays, r0, r1):
    """rays where the reference's behaviour (rule 0) and the library's (rule 1) part: each must be a finite tmax, a nearer hit kept, or a tie"""
    diff = np.nonzero((hit_bytes(r0) != hit_bytes(r1)).any(1))[0]
    print(f"{what}: {diff.size} of {rays.shape[0]} rays in the deviation class")
    ok = (rays["t"][diff] < np.float32(1e30)) | (r1["t"][diff] <= r0["t"][diff])
    assert ok.all(), (what, diff[~ok][:5])
    return diff


@pytest.mark.parametrize("case", ["blas_legocar", "blas_rock"])
def test_blas_against_restatement_and_goldens(ctx, vox_oracle, case):
    g = golden(case)
    dense = scene_dense(case[5:])
    sc = tb.VoxelSet(ctx).Build(dense)
    s = sc.arrays
    assert lib.tbvh_scene_layout(sc._h) == tb.LAYOUT_VOXELSET and sc.device_bytes == (16 + 32768 + s[1].size) * 4
    rays = g["rays"]
    r1 = vox_oracle.intersect(s, rays, rule=1)
    r0 = vox_oracle.intersect(s, rays, rule=0)
    got = sc.Intersect(rays.copy())                       # host array, stride 64, direct path (<= 16384 rays)
    same_hits(got, r1, case + " Intersect")
    assert (got["t"] != rays["t"]).sum() > rays.shape[0] // 20
    keep = ~(hit_bytes(r0) != hit_bytes(r1)).any(1)
    same_hits(got[keep], g["hits"][keep], case + " goldens")
    dev = deviation_report(case, rays, g["hits"], got)
    assert dev.size == (~keep).sum()
    occ = sc.IsOccluded(rays)
    assert np.array_equal(occ, vox_oracle.occluded(s, rays)) and np.array_equal(occ, g["occ"])
    # records of more than 64 bytes (tinybvh::Ray is 128): only the first 64 are read, bytes 44..63 written
    wide = np.zeros((rays.shape[0], 128), np.uint8)
    wide[:, :64] = rays.view(np.uint8).reshape(-1, 64)
    wide[:, 64:] = 0xA5
    sc.Intersect(wide)
    same_hits(wide[:, :64].copy().view(tb.RAY_DTYPE).reshape(-1), r1, case + " stride 128")
    assert (wide[:, 64:] == 0xA5).all()
    wide[:, :64] = rays.view(np.uint8).reshape(-1, 64)
    assert np.array_equal(sc.IsOccluded(wide), occ)


def test_set_and_update_top_grid(ctx, vox_oracle):
    """VoxelSet.Set / UpdateTopGrid (Python) give the arrays of a dense build and trace like them; later Set calls win, 0 clears"""
    v = tb.VoxelSet(ctx)
    v.Set([1, 2, 200, 9], [3, 4, 100, 9], [5, 6, 255, 9], [7, 8, 9, 10])
    v.Set(2, 4, 6, 0)
    v.Set(9, 9, 9, 11)
    v.UpdateTopGrid()
    dense = np.zeros((256, 256, 256), np.uint32)
    dense[5, 3, 1] = 7; dense[255, 100, 200] = 9; dense[9, 9, 9] = 11
    want = tb.host_build_voxelset(dense)
    for a, b in zip(v.arrays, want):
        assert np.array_equal(a, b)
    rays = tb.make_rays(np.array([[-1, (3.5) / 256, (5.5) / 256], [(200.5) / 256, (100.5) / 256, 2.0]], np.float32),
                        np.array([[1, 0, 0], [0, 0, -1]], np.float32))
    got = v.Intersect(rays.copy())
    assert got["prim"].tolist() == [7, 9]
    same_hits(got, vox_oracle.intersect(want, rays, rule=1), "Set / UpdateTopGrid")


def test_device_arrays_and_fresh(ctx, vox_oracle):
    dense = scene_dense("rock")
    sc = tb.VoxelSet(ctx).Build(dense)
    s = sc.arrays
    rays = voxel_rays(50000, seed=21, dense=dense)       # (beyond the direct path: the pipelined host path below)
    n = rays.shape[0]
    d = ctx.malloc(n * 64); dout = ctx.malloc(n)
    try:
        ctx.to_device(d, rays)
        sc.intersect_device(d, n)
        got = np.zeros_like(rays); ctx.synchronize(); ctx.from_device(got, d)
        r1 = vox_oracle.intersect(s, rays, rule=1)
        same_hits(got, r1, "device Intersect")
        ctx.to_device(d, rays)
        sc.occluded_device(d, n, dout)
        occ = np.zeros(n, np.uint8); ctx.synchronize(); ctx.from_device(occ, dout)
        assert np.array_equal(occ, vox_oracle.occluded(s, rays))
        # fresh: every record starts from {tmax, 0, 0, 0} and is written, hit or miss
        ctx.to_device(d, rays)
        sc.intersect_device_fresh(d, n, 0.75)
        ctx.synchronize(); ctx.from_device(got, d)
        start = rays.copy(); start["t"] = np.float32(0.75); start["u"] = 0; start["v"] = 0; start["prim"] = 0
        same_hits(got, vox_oracle.intersect(s, start, rule=1), "device fresh")
    finally:
        ctx.free(d); ctx.free(dout)
    same_hits(sc.Intersect(rays.copy()), r1, "host pipelined")


def test_large_batch(ctx, vox_oracle):
    """2^24 rays through the pipelined host path and the ray pool: the golden rays tiled, every tile as the restatement says"""
    g = golden("blas_legocar")
    sc = tb.VoxelSet(ctx).Build(scene_dense("legocar"))
    base = g["rays"]
    want = hit_bytes(vox_oracle.intersect(sc.arrays, base, rule=1))
    reps = (1 << 24) // base.shape[0]
    rays = np.tile(base, reps)
    sc.Intersect(rays)
    got = hit_bytes(rays).reshape(reps, base.shape[0], 5)
    bad = np.nonzero((got != want[None]).any(2).any(1))[0]
    assert bad.size == 0, f"{bad.size} of {reps} tiles differ"
    occ = sc.IsOccluded(np.tile(base, reps)).reshape(reps, -1)
    assert (occ == vox_oracle.occluded(sc.arrays, base)[None]).all()


def _random_instances(n, seed, n_sets, spread=6.0):
    rng = np.random.default_rng(seed)
    T = np.zeros((n, 4, 4), np.float32)
    for i in range(n):
        a = rng.normal(size=3); a /= np.linalg.norm(a)
        ang = rng.uniform(0, 2 * np.pi)
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        Rm = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K
        T[i, :3, :3] = Rm * rng.uniform(0.5, 2.0, 3)[None, :]
        T[i, :3, 3] = rng.uniform(-spread, spread, 3)
        T[i, 3, 3] = 1
    inst = tb.make_instances(T, rng.integers(0, n_sets, n).astype(np.uint32))
    inst["mask"] = rng.choice([0xFFFF, 0x1, 0x2, 0x100], n).astype(np.uint32)
    return inst


def test_tlas_goldens(ctx, vox_oracle):
    """the reference's own TLAS (its BVH_GPU conversion and BLASInstance records) uploaded as it is"""
    g = golden("tlas")
    sets = [tb.VoxelSet(ctx).Build(scene_dense(n)) for n in ("legocar", "rock")]
    arrs = [s.arrays for s in sets]
    inst = g["instances"].copy()
    tl = tb.TLAS(ctx).Upload(g["tlas_nodes"], g["tlas_idx"], inst, sets)
    rays = g["rays"]
    r1 = vox_oracle.intersect_tlas(None, None, inst, arrs, rays, rule=1)
    r0 = vox_oracle.intersect_tlas(g["tlas_wald"], g["tlas_idx"], inst, arrs, rays, rule=0)
    same_hits(r0, g["hits"], "rule 0 = reference")
    got = tl.Intersect(rays.copy())
    same_hits(got, r1, "TLAS Intersect")
    keep = ~(hit_bytes(r0) != hit_bytes(r1)).any(1)
    same_hits(got[keep], g["hits"][keep], "TLAS goldens")
    deviation_report("tlas golden", rays, g["hits"], got)
    occ = tl.IsOccluded(rays)
    assert np.array_equal(occ, g["occ"]) and np.array_equal(occ, vox_oracle.occluded_tlas(None, None, inst, arrs, rays, rule=1))


def test_tlas_1000_instances_update_and_rebuild(ctx, vox_oracle):
    names = ("legocar", "rock", "block64")
    sets = [tb.VoxelSet(ctx).Build(scene_dense(n)) for n in names]
    arrs = [s.arrays for s in sets]
    inst = _random_instances(1000, 31, len(names))
    tl = tb.TLAS(ctx).Build(inst, sets)
    rays = voxel_rays(16384, seed=32, lo=(-7, -7, -7), hi=(7, 7, 7))

    def check(what, inst_now):
        r1 = vox_oracle.intersect_tlas(None, None, inst_now, arrs, rays, rule=1)
        got = tl.Intersect(rays.copy())
        same_hits(got, r1, what + " Intersect")
        assert (got["t"] != rays["t"]).sum() > rays.shape[0] // 10, what
        assert np.array_equal(tl.IsOccluded(rays), vox_oracle.occluded_tlas(None, None, inst_now, arrs, rays, rule=1)), what

    check("upload", inst)
    # tbvh_update_tlas: the instances moved, the tree rebuilt on the host
    moved = _random_instances(1000, 33, len(names))
    inst["transform"] = moved["transform"]
    tl.Build(inst, sets)
    check("update", inst)
    # tbvh_rebuild_tlas_device: instance records and tree made on the device; the restatement reads the records back
    again = _random_instances(1000, 34, len(names))
    tl.RebuildOnDevice(np.ascontiguousarray(again["transform"]))
    _, _, inst_dev = tl.Download()
    assert np.array_equal(inst_dev["transform"], again["transform"])
    check("device rebuild", inst_dev)


def test_two_contexts_sharded(ctx, vox_oracle):
    dense = scene_dense("legocar")
    c2 = tb.Context(0)
    try:
        a = tb.VoxelSet(ctx).Build(dense)
        b = tb.VoxelSet(c2).Build(dense)
        rays = voxel_rays(40000, seed=41, dense=dense)
        got = tb.intersect_sharded([a, b], rays.copy())
        same_hits(got, vox_oracle.intersect(a.arrays, rays, rule=1), "sharded")
        assert np.array_equal(tb.occluded_sharded([a, b], rays), vox_oracle.occluded(a.arrays, rays))
        b.free()
    finally:
        c2.close()


def _upload_rc(ctx, grid, bricks, n_bricks, top):
    h = C.c_void_p()
    rc = lib.tbvh_upload_voxelset(ctx._h, grid.ctypes.data, bricks.ctypes.data, n_bricks, top.ctypes.data, C.byref(h))
    if rc == 0:
        lib.tbvh_free_scene(h)
    return rc, lib.tbvh_last_error().decode()


def test_malformed_sets_are_refused(ctx):
    grid, bricks, top = tb.host_build_voxelset(scene_dense("rock"))
    nb = bricks.size // 512
    assert _upload_rc(ctx, grid, bricks, nb, top)[0] == 0
    rc, err = _upload_rc(ctx, grid, bricks, 0, top)
    assert rc == -5 and "n_bricks = 0" in err, err
    g = grid.copy(); first = int(np.nonzero(g)[0][0]); g[first] = nb
    rc, err = _upload_rc(ctx, g, bricks, nb, top)
    assert rc == -5 and f"grid[{first}] = {nb} >= n_bricks = {nb}" in err, err
    rc, err = _upload_rc(ctx, grid, bricks, nb - 1, top)   # (the last brick is in use)
    assert rc == -5 and "grid[" in err, err
    assert lib.tbvh_upload_voxelset(ctx._h, None, bricks.ctypes.data, nb, top.ctypes.data, C.byref(C.c_void_p())) == -1
    # the dense upload and its extent check
    d = np.zeros((4, 4, 300), np.uint32)
    assert lib.tbvh_upload_voxelset_dense(ctx._h, d.ctypes.data, 300, 4, 4, C.byref(C.c_void_p())) == -1
    h = C.c_void_p()
    dense = scene_dense("rock")
    assert lib.tbvh_upload_voxelset_dense(ctx._h, dense.ctypes.data, 48, 48, 48, C.byref(h)) == 0
    assert lib.tbvh_scene_layout(h) == tb.LAYOUT_VOXELSET
    lib.tbvh_free_scene(h)


def test_other_entry_points_refuse_voxel_scenes(ctx):
    sc = tb.VoxelSet(ctx).Build(scene_dense("rock"))
    inst = tb.make_instances(np.eye(4, dtype=np.float32)[None], 0)
    tl = tb.TLAS(ctx).Build(inst, [sc])
    v4 = np.zeros((900, 4), np.float32)
    d = ctx.malloc(64 * 128); dout = ctx.malloc(64)
    buf = np.zeros(1 << 16, np.uint8)
    nb = C.c_uint64(0)
    hint = (C.c_uint8 * 8)()
    wf = tb.Wavefront(ctx, 64, 64)
    cam = R.camera((0, 0, -20), (0, 0, 1), 64, 64, 1, 1)
    params = tb._capi.WfParams()
    try:
        blas_only = {
            "tbvh_refit": lambda h: lib.tbvh_refit(h, v4.ctypes.data, 300, 0),
            "tbvh_update_bvh_gpu": lambda h: lib.tbvh_update_bvh_gpu(h, buf.ctypes.data, 1, buf.ctypes.data, 1, v4.ctypes.data, 1),
            "tbvh_update_bvh4_gpu": lambda h: lib.tbvh_update_bvh4_gpu(h, buf.ctypes.data, 4),
            "tbvh_update_cwbvh": lambda h: lib.tbvh_update_cwbvh(h, buf.ctypes.data, 5, buf.ctypes.data, 3),
            "tbvh_set_opacity_micromaps": lambda h: lib.tbvh_set_opacity_micromaps(h, buf.ctypes.data, 1, 300, 0),
            "tbvh_scene_download": lambda h: lib.tbvh_scene_download(h, 0, None, 0, C.byref(nb)),
            "tbvh_cwbvh_set_hybrid": lambda h: lib.tbvh_cwbvh_set_hybrid(h, 0),
            "tbvh_scene_get_schedule_hint": lambda h: lib.tbvh_scene_get_schedule_hint(h, C.cast(hint, C.c_void_p)),
            "tbvh_scene_set_schedule_hint": lambda h: lib.tbvh_scene_set_schedule_hint(h, C.cast(hint, C.c_void_p)),
            "tbvh_upload_tlas_double (voxel BLAS)": lambda h: lib.tbvh_upload_tlas_double(ctx._h, buf.ctypes.data, 1, buf.ctypes.data, 1, buf.ctypes.data, 1,
                                                                                          (C.c_void_p * 1)(h), 1, C.byref(C.c_void_p())),
            "tbvh_intersect_ex": lambda h: lib.tbvh_intersect_ex(h, buf.ctypes.data, 4),
            "tbvh_occluded_ex": lambda h: lib.tbvh_occluded_ex(h, buf.ctypes.data, 4, buf.ctypes.data),
            "tbvh_intersect_ex_device": lambda h: lib.tbvh_intersect_ex_device(h, d, 4),
            "tbvh_occluded_ex_device": lambda h: lib.tbvh_occluded_ex_device(h, d, 4, dout),
        }
        both = {"tbvh_wavefront_render": lambda h: lib.tbvh_wavefront_render(wf._h, h, v4.ctypes.data, C.byref(cam), C.byref(params), None)}
        for name, call in blas_only.items():
            assert call(sc._h) == -1, name
            assert lib.tbvh_last_error(), name
        for name, call in both.items():
            for h in (sc._h, tl._h):
                assert call(h) == -1, (name, h == tl._h)
        # a TLAS mixing voxel sets and triangle BLASes
        tri = tb.BVH_GPU(ctx).Build(scenes.soup(100))
        inst2 = tb.make_instances(np.tile(np.eye(4, dtype=np.float32), (2, 1, 1)), np.array([0, 1], np.uint32))
        for order in ([sc, tri], [tri, sc]):
            with pytest.raises(tb.TbvhError) as e:
                tb.TLAS(ctx).Build(inst2.copy(), order)
            assert e.value.code == -1 and "voxel" in str(e.value)
        # the voxel scenes still answer afterwards
        rays = voxel_rays(2048, seed=5)
        assert (sc.Intersect(rays.copy())["t"] != rays["t"]).any()
        assert (tl.Intersect(rays.copy())["t"] != rays["t"]).any()
    finally:
        wf.close()
        ctx.free(d); ctx.free(dout)
