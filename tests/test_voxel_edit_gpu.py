"""Editing a voxel set on the GPU (kernels_voxel_edit.hip): the batched Set, UpdateTopGrid, growth under a live TLAS and GetNormal.  The device
arrays must equal the CPU twin's byte for byte (tests/test_voxel_edit_host.py holds the twin to the real reference), queries on an edited set
must equal queries on a fresh upload of its arrays, and the normals must equal the goldens the real reference wrote
(tests/golden/voxeledit, tools/make_voxel_edit_golden.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import tinybvh_amd as tb
from tinybvh_amd import lib
from voxel_lib import hit_bytes, voxel_rays
from voxel_edit_lib import (GOLDEN_EDIT, SET_CASES, VOXELIZE_CASES, VOXELIZE_COLOUR, VOXELIZE_MAX_HITS, host_twin, legocar_records, normal_rays, same_arrays,
                            set_case, voxelize_instances, voxelize_scene)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = tb.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def rays8k():
    return voxel_rays(8192, seed=71)


def same_queries(ctx, sc, rays, what):
    """Intersect and IsOccluded on the edited set equal those on a fresh upload of its downloaded arrays, byte for byte"""
    fresh = tb.VoxelSet(ctx).Upload(*sc.Arrays())
    try:
        a, b = sc.Intersect(rays.copy()), fresh.Intersect(rays.copy())
        assert np.array_equal(hit_bytes(a), hit_bytes(b)), what
        assert np.array_equal(sc.IsOccluded(rays), fresh.IsOccluded(rays)), what
        return a
    finally:
        fresh.free()


def device_records(ctx, recs):
    d = ctx.malloc(recs.nbytes)
    ctx.to_device(d, recs)
    return d


@pytest.mark.parametrize("on_device", [False, True], ids=["host_records", "device_records"])
@pytest.mark.parametrize("case", SET_CASES)
def test_set_matches_host_twin(ctx, rays8k, case, on_device):
    batches = set_case(case)
    if case == "legocar_100k":            # on top of the uploaded car: capacity = used bricks, so the batch has to grow the set
        sc = tb.VoxelSet(ctx).Upload(*host_twin(batches[:1]))
        todo = batches[1:]
        assert sc.Capacity()[0] == sc.Capacity()[1]
    else:
        sc = tb.VoxelSet(ctx).CreateOnDevice(4 if case == "bricks_65_out_of_order" else 64)
        todo = batches
    try:
        for b in todo:
            if on_device:
                d = device_records(ctx, b)
                try:
                    sc.SetOnDevice(d, n=b.shape[0])
                finally:
                    ctx.free(d)
            else:
                sc.SetOnDevice(b)
        want = host_twin(batches, top=False)
        got = sc.Arrays()
        if case == "legocar_100k":        # (the upload carried the car's top grid; nothing has updated it since)
            want = (want[0], want[1], host_twin(batches[:1])[2])
        same_arrays(got, want, case + " before UpdateTopGrid")
        sc.UpdateTopGridOnDevice()
        same_arrays(sc.Arrays(), host_twin(batches), case)
        cap, used = sc.Capacity()
        assert used == want[1].size // 512 and cap >= used
        hits = same_queries(ctx, sc, rays8k, case)
        if case == "legocar_100k":
            assert (hits["t"] != rays8k["t"]).sum() > 1000
    finally:
        sc.free()


def test_device_bytes_follow_what_the_set_holds(ctx):
    sc = tb.VoxelSet(ctx).CreateOnDevice(10)
    try:
        base = (16 + 32768 + 10 * 512) * 4
        assert sc.device_bytes == base and sc.Capacity() == (10, 1)
        sc.SetOnDevice(np.array([[1, 2, 3, 4]], np.uint32))
        words = sc.debug_bytes()
        assert words[0] == base and words[6] >= 10 * 512 * 4 + 4 * 32768 * 4 and sc.device_bytes == sum(words[:7])
        sc.Reserve(100)
        assert sc.Capacity() == (100, 2) and sc.debug_bytes()[0] == (16 + 32768 + 100 * 512) * 4
        sc.Reserve(50)                     # never shrinks
        assert sc.Capacity() == (100, 2)
    finally:
        sc.free()


def test_growth_under_a_live_tlas(ctx):
    """a TLAS snapshots its BLASes' pointers: after the set reallocates, the TLAS traces the new arrays"""
    rng = np.random.default_rng(81)
    first = np.concatenate([rng.integers(0, 128, (2000, 3)), rng.integers(1, 1 << 32, (2000, 1), dtype=np.uint64)], 1).astype(np.uint32)
    sc = tb.VoxelSet(ctx).CreateOnDevice(8)
    other = tb.VoxelSet(ctx).Upload(*host_twin([legocar_records()]))
    T = np.tile(np.eye(4, dtype=np.float32), (3, 1, 1))
    T[0, :3, :3] = np.array([[0, -2, 0], [1.5, 0, 0], [0, 0, 1]], np.float32); T[0, :3, 3] = (-1, 0.25, 0)
    T[1, :3, 3] = (1.5, 0, 0.5)
    T[2, :3, :3] *= 0.5; T[2, :3, 3] = (0, 1.5, -1)
    blas_idx = np.array([0, 1, 0], np.uint32)
    rays = voxel_rays(8192, seed=82, lo=(-3, -1, -2), hi=(3, 3, 2))
    try:
        sc.SetOnDevice(first).UpdateTopGridOnDevice()
        inst = tb.make_instances(T, blas_idx)
        tl = tb.TLAS(ctx).Build(inst, [sc, other])
        before = tl.Intersect(rays.copy())
        cap0 = sc.Capacity()[0]
        more = np.concatenate([rng.integers(0, 256, (5000, 3)), rng.integers(1, 1 << 32, (5000, 1), dtype=np.uint64)], 1).astype(np.uint32)
        xs, ys, zs = np.meshgrid(np.arange(128, 256), np.arange(128, 256), np.arange(128, 132), indexing="ij")   # and a slab no ray through it can miss
        slab = np.stack([xs.ravel(), ys.ravel(), zs.ravel(), np.full(xs.size, 0xABCDEF)], 1).astype(np.uint32)
        more = np.concatenate([more, slab])
        sc.SetOnDevice(more)
        assert sc.Capacity()[0] > cap0                                # at least one reallocation
        sc.UpdateTopGridOnDevice()
        got = tl.Intersect(rays.copy())
        occ = tl.IsOccluded(rays)
        fresh = tb.VoxelSet(ctx).Upload(*sc.Arrays())
        inst2 = tb.make_instances(T, blas_idx)
        tl2 = tb.TLAS(ctx).Build(inst2, [fresh, other])
        want = tl2.Intersect(rays.copy())
        assert np.array_equal(hit_bytes(got), hit_bytes(want))
        assert np.array_equal(occ, tl2.IsOccluded(rays))
        assert (hit_bytes(got) != hit_bytes(before)).any(1).sum() > 100  # the new voxels are seen
        same_arrays(sc.Arrays(), host_twin([first, more]), "grown set")
        tl2.free(); fresh.free(); tl.free()
    finally:
        sc.free(); other.free()


def test_stale_top_grid(ctx):
    """a Set without UpdateTopGrid: where the top-grid bit was 0 the queries answer as before, exactly as on the CPU"""
    first = np.array([[x, y, 3, 7] for x in range(0, 32) for y in range(0, 32)], np.uint32)           # top cell (0, 0, 0) only
    added = np.array([[x, y, 200, 9] for x in range(128, 160) for y in range(128, 160)], np.uint32)   # top cell (4, 4, 6): bit was 0
    O = np.stack([np.linspace(0.01, 0.7, 2048), np.linspace(0.02, 0.69, 2048), np.full(2048, -1.0)], 1).astype(np.float32)
    rays = tb.make_rays(O, np.tile(np.array([[0, 0, 1]], np.float32), (2048, 1)))
    sc = tb.VoxelSet(ctx).CreateOnDevice(64)
    try:
        sc.SetOnDevice(first).UpdateTopGridOnDevice()
        before = sc.Intersect(rays.copy())
        occ_before = sc.IsOccluded(rays)
        sc.SetOnDevice(added)
        stale = sc.Intersect(rays.copy())
        assert np.array_equal(hit_bytes(stale), hit_bytes(before)) and np.array_equal(sc.IsOccluded(rays), occ_before)
        assert np.array_equal(sc.Arrays()[2], host_twin([first])[2])
        sc.UpdateTopGridOnDevice()
        now = sc.Intersect(rays.copy())
        assert ((now["prim"] == 9) & (before["prim"] != 9)).sum() > 100
        same_arrays(sc.Arrays(), host_twin([first, added]), "after UpdateTopGrid")
    finally:
        sc.free()


def test_set_refusals(ctx):
    sc = tb.VoxelSet(ctx).CreateOnDevice(16)
    tri = tb.LAYOUT_CLASSES[tb.LAYOUT_BVH_GPU](ctx).Build(np.array([[0, 0, 0, 0], [1, 0, 0, 0], [0, 1, 0, 0]], np.float32))
    good = np.array([[1, 2, 3, 4], [9, 9, 9, 9]], np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    try:
        sc.SetOnDevice(good)
        before = sc.Arrays()
        for bad in ([256, 0, 0, 1], [0, 300, 0, 1], [0, 0, 0xFFFFFFFF, 1]):
            with pytest.raises(tb.TbvhError) as e:
                sc.SetOnDevice(np.array([[7, 7, 7, 7], bad], np.uint32))
            assert e.value.code == -1 and "record 1" in str(e.value)
            same_arrays(sc.Arrays(), before, "unchanged after a refused host batch")
        assert lib.tbvh_voxelset_set(sc._h, None, 2, 0) == -1
        assert lib.tbvh_voxelset_set(sc._h, None, 0, 0) == 0                       # n = 0 is a no-op
        assert lib.tbvh_voxelset_set(None, p(good), 2, 0) == -1
        assert lib.tbvh_voxelset_set(tri._h, p(good), 2, 0) == -1                  # not a voxel set
        assert lib.tbvh_voxelset_update_top_grid(tri._h) == -1 and lib.tbvh_voxelset_reserve(tri._h, 4) == -1
        assert lib.tbvh_voxelset_download(tri._h, None, None, 0, None, None) == -1
        assert lib.tbvh_voxelset_reserve(sc._h, (1 << 22) + 1) == -5
        bricks = np.zeros(512, np.uint32)
        assert lib.tbvh_voxelset_download(sc._h, None, p(bricks), 1, None, None) == -1   # the set uses 3 bricks
        # device records: misaligned array refused; records out of range are skipped and counted, the others applied
        recs = np.array([[20, 20, 20, 5], [256, 0, 0, 6], [21, 20, 20, 7], [0, 0, 999, 8]], np.uint32)
        d = device_records(ctx, recs)
        try:
            assert lib.tbvh_voxelset_set(sc._h, C.c_void_p(d + 4), 1, 1) == -1
            with pytest.raises(tb.TbvhError) as e:
                sc.SetOnDevice(d, n=4)
            assert e.value.code == -5 and "2 of 4" in str(e.value)
        finally:
            ctx.free(d)
        same_arrays(sc.Arrays(), host_twin([good, recs[[0, 2]]], top=False), "the records in range were applied")
    finally:
        sc.free(); tri.free()


def golden(case):
    return np.load(os.path.join(GOLDEN_EDIT, case + ".npz"))


def test_normals_one_set_golden(ctx):
    g = golden("normals")
    rays, want = g["rays"], g["normals"]
    hit = rays["t"] < np.float32(1e30)
    sc = tb.VoxelSet(ctx).CreateOnDevice(1)
    try:
        for scene in (None, sc):
            got = tb.voxel_normals(ctx, scene, rays)
            assert np.array_equal(got[hit].view(np.uint32), want[hit].view(np.uint32)) and not got[~hit].view(np.uint32).any()
        # device-resident records with a stride, through the method
        wide = np.zeros((rays.shape[0], 96), np.uint8)
        wide[:, :64] = rays.view(np.uint8).reshape(-1, 64)
        d_r, d_o = ctx.malloc(wide.nbytes), ctx.malloc(rays.shape[0] * 16)
        try:
            ctx.to_device(d_r, wide)
            sc.Normals(d_r, n=rays.shape[0], d_out=d_o, stride=96)
            got = np.zeros((rays.shape[0], 4), np.float32)
            ctx.from_device(got, d_o)
            assert np.array_equal(got[hit].view(np.uint32), want[hit].view(np.uint32)) and not got[~hit].any()
        finally:
            ctx.free(d_r); ctx.free(d_o)
        assert np.array_equal(got, tb.host_voxel_normals(rays))
    finally:
        sc.free()


def _rotated_instances(n, seed):
    rng = np.random.default_rng(seed)
    T = np.zeros((n, 4, 4), np.float32)
    for i in range(n):
        a = rng.normal(size=3); a /= np.linalg.norm(a)
        ang = rng.uniform(0, 2 * np.pi)
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        Rm = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K
        T[i, :3, :3] = Rm * rng.uniform(0.5, 2.0, 3)[None, :]
        T[i, :3, 3] = rng.uniform(-3, 3, 3)
        T[i, 3, 3] = 1
    return tb.make_instances(T, np.zeros(n, np.uint32))


def test_normals_tlas_golden_and_twin(ctx):
    g = golden("normals_tlas")
    rays, want = g["rays"], g["normals"]
    hit = rays["t"] < np.float32(1e30)
    sc = tb.VoxelSet(ctx).CreateOnDevice(1)
    tri = tb.LAYOUT_CLASSES[tb.LAYOUT_BVH_GPU](ctx).Build(np.array([[0, 0, 0, 0], [1, 0, 0, 0], [0, 1, 0, 0]], np.float32))
    try:
        inst = tb.make_instances(g["transforms"].reshape(-1, 4, 4), np.zeros(g["transforms"].shape[0], np.uint32))
        tl = tb.TLAS(ctx).Build(inst, [sc])
        got = tb.voxel_normals(ctx, tl, rays)
        assert np.array_equal(got[hit].view(np.uint32), want[hit].view(np.uint32)) and not got[~hit].view(np.uint32).any()
        tl.free()
        # rotated, scaled instances: the device against the CPU twin over the instance records the TLAS holds
        inst = _rotated_instances(50, seed=91)
        tl = tb.TLAS(ctx).Build(inst, [sc])
        wr = normal_rays(8192, seed=92)
        wr["O"] = wr["O"] * np.float32(8) - np.float32(4)
        wr["inst"] = np.random.default_rng(93).integers(0, 50, 8192).astype(np.uint32)
        got = tb.voxel_normals(ctx, tl, wr)
        assert np.array_equal(got.view(np.uint32), tb.host_voxel_normals(wr, tl.Download()[2]).view(np.uint32))
        assert (np.abs(got[:, :3]).sum(1) == 1).sum() == (wr["t"] < np.float32(1e30)).sum()
        # a hit.inst beyond the instances: zeros for that record, TBVH_E_FORMAT, nothing read out of range
        bad = wr.copy()
        k = int(np.nonzero(wr["t"] < np.float32(1e30))[0][5])
        bad["inst"][k] = 50
        with pytest.raises(tb.TbvhError) as e:
            tb.voxel_normals(ctx, tl, bad)
        assert e.value.code == -5
        # refused: any other scene, bad strides
        out = np.zeros((4, 4), np.float32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
        assert lib.tbvh_voxel_normals(ctx._h, tri._h, p(wr), 64, 4, p(out)) == -1
        assert lib.tbvh_voxel_normals(ctx._h, None, p(wr), 60, 4, p(out)) == -1
        assert lib.tbvh_voxel_normals_device(ctx._h, None, C.c_void_p(16), 72, 4, C.c_void_p(16)) == -1
        assert lib.tbvh_voxel_normals(None, None, p(wr), 64, 4, p(out)) == -1
        tl.free()
    finally:
        sc.free(); tri.free()


# ---- voxelising a traced scene: the device's set against the one the reference's loop left (tests/golden/voxeledit/voxelize_*.npz) ------------------
@pytest.fixture(scope="module")
def vox_world(ctx):
    verts, fat, mats, texs = voxelize_scene()
    blas = tb.LAYOUT_CLASSES[tb.LAYOUT_CWBVH](ctx).Build(verts)
    inst = voxelize_instances()
    tlas = tb.TLAS(ctx).Build(inst, [blas])
    sh = tb.Shading(ctx, mats, texs).SetFatTris(0, fat)
    yield {"blas": blas, "tlas": tlas, "shading": sh}
    sh.free(); tlas.free(); blas.free()


def run_voxelize(ctx, w, case, g, max_hits):
    vs = tb.VoxelSet(ctx).CreateOnDevice(256)
    st = vs.Voxelize(w["tlas"] if case == "tlas" else w["blas"], g["bmin"], g["max_size"], g["ext"], shading=None if case == "colour" else w["shading"],
                     color=VOXELIZE_COLOUR, max_hits_per_ray=max_hits)
    return vs, st


@pytest.mark.parametrize("case", VOXELIZE_CASES)
def test_voxelize_equals_the_reference_loop(ctx, vox_world, case):
    g = golden("voxelize_" + case)
    assert int(g["max_hits"]) <= VOXELIZE_MAX_HITS                  # the reference alone stays within the cap (asserted by the golden tool, stored)
    vs, st = run_voxelize(ctx, vox_world, case, g, VOXELIZE_MAX_HITS)
    try:
        print(case, st, "reference: records", int(g["records"]), "max hits", int(g["max_hits"]))
        assert st["rays_cut"] == 0
        same_arrays(vs.Arrays(), (g["grid"], g["bricks"], g["top"]), "voxelize " + case)
        assert st["records"] == int(g["records"]) and st["bricks"] == g["bricks"].size // 512 and st["rounds"] == int(g["max_hits"]) + 1
    finally:
        vs.free()


def test_voxelize_cut_rays_and_adding_to_a_set(ctx, vox_world):
    g = golden("voxelize_table")
    vs, st = run_voxelize(ctx, vox_world, "table", g, 2)
    try:
        assert st["rays_cut"] == int(g["rays_over_2"]) and st["rounds"] == 3 and 0 < st["records"] < int(g["records"])
        # records are added to what the set holds: the full run on top of the cut one leaves the full run's voxels (every voxel is written again);
        # the bricks were numbered by the cut run first, so only the voxel contents are compared, through a dense view
        st2 = vs.Voxelize(vox_world["blas"], g["bmin"], g["max_size"], g["ext"], shading=vox_world["shading"], max_hits_per_ray=VOXELIZE_MAX_HITS)
        assert st2["rays_cut"] == 0 and st2["records"] == int(g["records"]) and st2["bricks"] == g["bricks"].size // 512
        grid, bricks, top = vs.Arrays()
        assert np.array_equal(top, g["top"]) and np.array_equal(grid != 0, g["grid"] != 0)
        cells = np.nonzero(grid)[0]
        assert np.array_equal(bricks.reshape(-1, 512)[grid[cells]], g["bricks"].reshape(-1, 512)[g["grid"][cells]])
    finally:
        vs.free()


def test_voxelize_refusals(ctx, vox_world):
    from tinybvh_amd._capi import VoxelizeParams
    vs = tb.VoxelSet(ctx).CreateOnDevice(4)
    sph = tb.SphereBVH(ctx).Build(np.array([[0, 0, 0, 1], [3, 0, 0, 1]], np.float32))
    p = VoxelizeParams((C.c_float * 3)(0, 0, 0), 1.0, (C.c_float * 3)(1, 1, 1), 1, 4)
    blas = vox_world["blas"]
    try:
        f = lib.tbvh_voxelize_device
        assert f(None, None, C.byref(p), vs._h, None) == -1 and f(blas._h, None, None, vs._h, None) == -1 and f(blas._h, None, C.byref(p), None, None) == -1
        assert f(vs._h, None, C.byref(p), vs._h, None) == -1          # voxel content as the traced scene
        assert f(sph._h, None, C.byref(p), vs._h, None) == -1         # sphere content
        assert f(blas._h, None, C.byref(p), blas._h, None) == -1      # not a voxel set to write to
        for bad in ((0.0, 1, 1), (1, -2.0, 1), (1, 1, float("inf"))):
            q = VoxelizeParams((C.c_float * 3)(0, 0, 0), 1.0, (C.c_float * 3)(*bad), 1, 4)
            assert f(blas._h, None, C.byref(q), vs._h, None) == -1
        assert vs.Capacity() == (4, 1)
    finally:
        vs.free(); sph.free()
