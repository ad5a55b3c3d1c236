"""Every device allocation the library makes is given back: tbvh_debug_device_allocations (live allocations and their bytes, over the whole
process) returns to its earlier values, exactly, once the scenes, the wavefront object and the context made since are gone.  The cycle below
goes through every place the library owns device memory — the scene arrays of every layout, the derived copies and wide TLAS trees, the
staging and scratch areas that grow on demand, the context's own buffers — on the smallest geometry there is: a lifetime bug does not need a
large one."""
import ctypes as C
import gc
import os

import numpy as np
import pytest

import tinybvh_amd as tb
from tinybvh_amd import rays as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def live():
    out = (C.c_uint64 * 2)()
    tb.check(tb.lib.tbvh_debug_device_allocations(out), "tbvh_debug_device_allocations")
    return int(out[0]), int(out[1])


def instances(n, extent):
    t = np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))
    t[:, 0, 3] = np.arange(n, dtype=np.float32) * 1.5 * extent
    return tb.make_instances(t, np.arange(n, dtype=np.uint32) % 3)


def cycle(g, monkeypatch):
    verts = g["verts"]
    lo, hi = verts[:, :3].min(0), verts[:, :3].max(0)
    pos, inv = np.unique(verts, axis=0, return_inverse=True)
    pos = np.ascontiguousarray(pos, np.float32); idx = np.ascontiguousarray(inv.reshape(-1, 3).astype(np.uint32))
    before = live()
    ctx = tb.Context(0)
    assert live()[0] > before[0]   # (the context's own buffers)

    # one BLAS per triangle layout, one of them from an indexed mesh (it keeps an index buffer); spheres, voxels, fp64
    blas = [tb.BVH_GPU(ctx).Build(pos, indices=idx, threads=1), tb.BVH4_GPU(ctx).Build(verts, threads=1), tb.BVH8_CWBVH(ctx).Build(verts, threads=1)]
    rng = np.random.default_rng(3)
    sph = np.concatenate([rng.uniform(lo, hi, (200, 3)), rng.uniform(0.01, 0.05, (200, 1))], axis=1).astype(np.float32)
    spheres = tb.SphereBVH(ctx).Build(sph)
    voxels = tb.VoxelSet(ctx).Build(tb.load_voxel_file(os.path.join(GOLDEN, "voxels", "rock.bin")))
    dbl = tb.BVH_Double(ctx).Build(verts[:, :3].astype(np.float64))
    tdbl = tb.TLAS_Double(ctx).Build(tb.make_instances_ex(np.tile(np.eye(4), (2, 1, 1)), np.zeros(2, np.uint64)), [dbl])
    rex = tb.make_rays_ex(rng.uniform(lo, hi, (256, 3)), rng.normal(size=(256, 3)))
    tdbl.Intersect(rex.copy()); tdbl.IsOccluded(rex)
    r256 = R.random_rays(256, lo, hi, seed=2)
    spheres.Intersect(r256.copy()); voxels.IsOccluded(R.random_rays(256, (0, 0, 0), (1, 1, 1), seed=2))

    # a TLAS of 8 instances over the three (their 4-wide copies are made here); resident rays: the first any-hit query makes the 8-wide
    # copies and the second wide tree
    ext = float(hi[0] - lo[0])
    tl = tb.TLAS(ctx).Build(instances(8, ext), blas)
    n = 4096
    rays = R.random_rays(n, lo, hi + np.array([8 * 1.5 * ext, 0, 0], np.float32), seed=5)
    d_rays, d_out, d_occ = ctx.malloc(n * 64), ctx.malloc(n * 64), ctx.malloc(n)
    ctx.to_device(d_rays, rays)
    bytes_tlas = tl.device_bytes
    tl.intersect_device(d_rays, n); tl.occluded_device(d_rays, n, d_occ)
    ctx.synchronize()
    assert tl.device_bytes > bytes_tlas
    tl.Intersect(R.random_rays(20000, lo, hi, seed=6))   # above the direct limit: the pipelined host path and its buffers
    tl.Build(instances(40, ext), blas)                     # (an update: the TLAS arrays grow)
    tl.RebuildOnDevice(np.tile(np.eye(4, dtype=np.float32).reshape(16), (40, 1)))
    tl.occluded_device(d_rays, n, d_occ)

    n_tris = verts.shape[0] // 3
    blas[2].SetOpacityMicroMaps(np.full((n_tris, 1), 0xFFFF, np.uint32), 4); blas[2].SetOpacityMicroMaps(None, 0)
    blas[1].Refit(verts)
    blas[0].intersect_spheres(sph, pos, indices=idx)
    ctx.bin_rays(d_rays, d_out, n, np.concatenate([lo, hi]))

    # a scene of its own whose direct query makes its 8-wide copy; an update drops it
    monkeypatch.setenv("TBVH_WIDE_COPY_MIN", "64")
    solo = tb.BVH4_GPU(ctx).Upload(g["bvh4_0"])
    bytes_solo = solo.device_bytes
    solo.intersect_device(d_rays, n)
    ctx.synchronize()
    assert solo.device_bytes > bytes_solo
    solo.Update(g["bvh4_0"])
    assert solo.device_bytes == bytes_solo
    monkeypatch.delenv("TBVH_WIDE_COPY_MIN")

    wf = tb.Wavefront(ctx, 64, 64)
    wf.set_blue_noise(np.zeros(128 * 128 * 8, np.uint32))
    assert live()[0] > before[0] and live()[1] > before[1]
    wf.close()

    for p in (d_rays, d_out, d_occ):
        ctx.free(p)
    blas[0].free()   # still under the TLAS: it goes with the TLAS
    tl.free()
    for s in (blas[1], blas[2], solo, spheres, voxels, tdbl, dbl):
        s.free()
    ctx.close()
    return before, live()


@pytest.mark.gpu
def test_every_device_allocation_is_given_back(monkeypatch):
    g = np.load(os.path.join(GOLDEN, "soup_2k.npz"))
    gc.collect()   # (scenes earlier tests dropped are freed by their finalizers: not in the middle of the count)
    first = None
    for _ in range(3):
        before, after = cycle(g, monkeypatch)
        first = first or before
        assert after == before == first
