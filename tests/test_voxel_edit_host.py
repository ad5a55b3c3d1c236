"""Editing a voxel set, on the host: the library's CPU twins (tbvh_host_voxelset_create / _set / _update_top_grid, tbvh_host_voxel_normals)
against the real reference's VoxelSet::Set / UpdateTopGrid / GetNormal, arrays byte for byte and normals bit for bit, and the committed goldens
against what the reference gives now.  The tests that run the reference skip when its checkout is absent (TBVH_REFERENCE); the refusals need
neither the reference nor a GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import tinybvh_amd as tb
from voxel_edit_lib import edit_ref   # noqa: F401 (fixture)
from voxel_edit_lib import GOLDEN_EDIT, SET_CASES, VOXELIZE_CASES, exact_instances, exact_world_rays, host_twin, normal_rays, same_arrays, set_case

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))


@pytest.mark.parametrize("case", SET_CASES)
def test_host_set_matches_reference(case, edit_ref):
    batches = set_case(case)
    same_arrays(host_twin(batches), edit_ref.run(batches), case)


def test_host_set_without_top_grid_leaves_it(edit_ref):
    """UpdateTopGrid is a call of its own: Set alone leaves the top grid as it was"""
    h = tb.HostVoxelEdit().Set(set_case("two_batches")[0]).UpdateTopGrid()
    top = h.arrays()[2].copy()
    h.Set(np.array([[255, 255, 255, 1]], np.uint32))
    assert np.array_equal(h.arrays()[2], top)
    h.UpdateTopGrid()
    assert h.arrays()[2][15] >> 31 == 1


def test_host_set_refusals():
    h = tb.HostVoxelEdit()
    before = [a.copy() for a in h.arrays()]
    assert before[1].size == 512 and not before[0].any() and not before[2].any()      # the reference's constructor: freeBrickPtr = 1
    for bad in ([256, 0, 0, 1], [0, 256, 0, 1], [0, 0, 256, 1], [0xFFFFFFFF, 0, 0, 1]):
        recs = np.array([[1, 2, 3, 4], bad, [5, 6, 7, 8]], np.uint32)
        with pytest.raises(tb.TbvhError) as e:
            h.Set(recs)
        assert e.value.code == -1 and "record 1" in str(e.value)
        same_arrays(h.arrays(), before, "unchanged after a refusal")
    lib = tb.lib
    assert lib.tbvh_host_voxelset_set(h._h, None, 3) == -1
    assert lib.tbvh_host_voxelset_set(None, None, 0) == -1
    assert lib.tbvh_host_voxelset_set(h._h, None, 0) == 0                              # n = 0 is a no-op
    assert lib.tbvh_host_voxelset_update_top_grid(None) == -1
    assert lib.tbvh_host_voxelset_create(None) == -1
    tri = tb.HostBVH(np.array([[0, 0, 0, 0], [1, 0, 0, 0], [0, 1, 0, 0]], np.float32), tb.LAYOUT_BVH_GPU)
    r = np.array([[1, 2, 3, 4]], np.uint32)
    assert lib.tbvh_host_voxelset_set(tri._h, r.ctypes.data_as(C.c_void_p), 1) == -1   # not a voxel set
    same_arrays(h.arrays(), before, "unchanged")


def test_host_normals_match_reference(edit_ref):
    rays = normal_rays(1 << 16, seed=5)
    got = tb.host_voxel_normals(rays)
    want = edit_ref.normals(rays)
    hit = rays["t"] < np.float32(1e30)
    assert hit.sum() > 50000 and (~hit).sum() > 3000
    assert np.array_equal(got[hit].view(np.uint32), want[hit].view(np.uint32))
    assert not got[~hit].view(np.uint32).any()                                         # the stated deviation: a miss gets zeros
    for axis in range(3):                                                              # every face answers
        assert (got[hit][:, axis] == 1).sum() > 1000 and (got[hit][:, axis] == -1).sum() > 1000
    # a zero or negative-zero component on the answering axis gives +1
    k = rays.shape[0] // 4
    z = rays["D"][2 * k:3 * k] == 0
    n = got[2 * k:3 * k, :3]
    assert (n[z] != -1).all() and (n[z] == 1).sum() > 1000


def test_host_normals_tlas_match_reference(edit_ref):
    rays = normal_rays(1 << 14, seed=6)
    inst = exact_instances(24, seed=7)
    world, obj = exact_world_rays(rays, inst, seed=8)
    got = tb.host_voxel_normals(world, inst)
    want = edit_ref.normals(obj)
    hit = rays["t"] < np.float32(1e30)
    assert np.array_equal(got[hit].view(np.uint32), want[hit].view(np.uint32)) and not got[~hit].any()
    # a hit.inst beyond the instances is reported and read through by nobody; a miss's hit.inst is not looked at
    bad = world.copy()
    first_hit, first_miss = int(np.nonzero(hit)[0][0]), int(np.nonzero(~hit)[0][0])
    bad["inst"][first_miss] = 0xFFFFFFFF
    assert np.array_equal(tb.host_voxel_normals(bad, inst), got)
    bad["inst"][first_hit] = 24
    with pytest.raises(tb.TbvhError) as e:
        tb.host_voxel_normals(bad, inst)
    assert e.value.code == -5


def test_host_normals_refusals():
    lib = tb.lib
    rays = normal_rays(64, seed=9)
    out = np.zeros((64, 4), np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    assert lib.tbvh_host_voxel_normals(None, 0, p(rays), 63, 64, p(out)) == -1
    assert lib.tbvh_host_voxel_normals(None, 0, p(rays), 66, 64, p(out)) == -1
    assert lib.tbvh_host_voxel_normals(None, 0, None, 64, 64, p(out)) == -1
    assert lib.tbvh_host_voxel_normals(None, 0, p(rays), 64, 64, None) == -1
    assert lib.tbvh_host_voxel_normals(p(rays), 0, p(rays), 64, 64, p(out)) == -1      # an instance array without instances
    assert lib.tbvh_host_voxel_normals(None, 0, None, 64, 0, None) == 0


@pytest.mark.parametrize("case", ["normals", "normals_tlas"] + ["voxelize_" + c for c in VOXELIZE_CASES])
def test_goldens_are_what_the_reference_gives(case, edit_ref):
    """every committed golden regenerated from the reference and compared byte for byte; the voxelise ones also state the reference loop's own maximum
    hits per ray, which the golden tool asserts to lie within the cap the GPU tests run with"""
    import make_voxel_edit_golden as G
    assert case in G.CASES
    want = G.make(case, edit_ref)
    with np.load(os.path.join(GOLDEN_EDIT, case + ".npz")) as g:
        assert sorted(g.files) == sorted(want)
        for k in want:
            assert g[k].dtype == np.asarray(want[k]).dtype and g[k].tobytes() == np.asarray(want[k]).tobytes(), (case, k)


def test_voxelize_helpers():
    bmin, m, ext = tb.voxelize_bounds([-6.3, -5.1, -4.7, 7.9, 6.2, 5.3])
    lo, hi = np.array([-6.3, -5.1, -4.7], np.float32), np.array([7.9, 6.2, 5.3], np.float32)
    assert np.array_equal(ext, hi - lo) and m == ext[0] and m.dtype == np.float32
    assert np.array_equal(bmin, (hi + lo) * np.float32(0.5) - np.float32(0.525) * m)
    T = tb.voxelize_matrix(bmin, m)
    assert T.shape == (4, 4) and T[0, 0] == T[1, 1] == T[2, 2] == np.float32(1) / m and T[3, 3] == 1
    assert np.array_equal(T[:3, 3], -bmin * (np.float32(1) / m)) and not T[3, :3].any() and T[0, 1] == 0
    centre = T @ np.append((hi + lo) * np.float32(0.5), np.float32(1))
    assert np.allclose(centre[:3], 0.525, atol=1e-6)                                    # the scene's centre lands in the cube's
