"""VoxelSet on the host: the library's builder against the real reference's arrays, the restatement (oracle_voxel.c) against the real
reference's Intersect / IsOccluded and TLAS traversals bit for bit, and the committed goldens against the reference's output.  Every test
that runs the reference skips when its checkout is absent (TBVH_REFERENCE); the builder's refusals need no reference and no GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import tinybvh_amd as tb
from voxel_lib import (GOLDEN, hit_bytes, scene_dense, voxel_rays, vox_oracle, vox_ref)   # noqa: F401 (fixtures)

SCENES = ["legocar", "rock", "sparse", "block64"]
N_RAYS = 1 << 16


@pytest.mark.parametrize("name", SCENES)
def test_host_builder_matches_reference(name, vox_ref, vox_oracle):
    dense = scene_dense(name)
    h = vox_ref.new_set(dense)
    try:
        rg, rb, rt = vox_ref.arrays(h)
    finally:
        vox_ref.lib.vref_free(h)
    g, b, t = tb.host_build_voxelset(dense)
    assert g.tobytes() == rg.tobytes()
    assert t.tobytes() == rt.tobytes()
    assert b.size == rb.size and b.tobytes() == rb.tobytes()   # the used bricks, brick 0 included
    og, ob, ot = vox_oracle.build(dense)                        # ... and the restatement's Set / UpdateTopGrid
    assert og.tobytes() == rg.tobytes() and ob.tobytes() == rb.tobytes() and ot.tobytes() == rt.tobytes()


def test_host_builder_refusals():
    with pytest.raises(tb.TbvhError):
        tb.host_build_voxelset(np.zeros((1, 1, 257), np.uint32))
    with pytest.raises(tb.TbvhError):
        tb.host_build_voxelset(np.zeros((257, 1, 1), np.uint32))
    h = C.c_void_p()
    assert tb.lib.tbvh_host_build_voxelset(None, 4, 4, 4, C.byref(h)) == -1
    v = np.zeros(8, np.uint32)
    assert tb.lib.tbvh_host_build_voxelset(v.ctypes.data_as(C.c_void_p), 0, 2, 4, C.byref(h)) == -1
    g, b, t = tb.host_build_voxelset(np.zeros((4, 4, 4), np.uint32))   # empty: brick 0 only
    assert b.size == 512 and not g.any() and not t.any()


def test_voxel_file_reader():
    d = tb.load_voxel_file(os.path.join(GOLDEN, "legocar.bin"))
    assert d.shape == (128, 128, 128) and int((d != 0).sum()) == 44692
    d = tb.load_voxel_file(os.path.join(GOLDEN, "rock.bin"))
    assert d.shape == (48, 48, 48) and int((d != 0).sum()) == 2802


@pytest.mark.parametrize("name", SCENES)
def test_restatement_rule0_matches_reference(name, vox_ref, vox_oracle):
    dense = scene_dense(name)
    s = vox_oracle.build(dense)
    h = vox_ref.new_set(dense)
    try:
        rays = voxel_rays(N_RAYS, seed=11, dense=dense)
        ref = vox_ref.intersect(h, rays)
        mine = vox_oracle.intersect(s, rays, rule=0)
        assert np.array_equal(hit_bytes(ref), hit_bytes(mine))
        assert (hit_bytes(ref)[:, 1] != hit_bytes(rays)[:, 1]).sum() > N_RAYS // 20   # (the set is hit)
        assert np.array_equal(vox_ref.occluded(h, rays), vox_oracle.occluded(s, rays))
        # rule 1 differs only where the reference records a hit that does not beat the incoming tmax
        r1 = vox_oracle.intersect(s, rays, rule=1)
        diff = np.nonzero((hit_bytes(r1) != hit_bytes(ref)).any(1))[0]
        assert np.all(rays["t"][diff] < np.float32(1e30))
        assert np.all(~(ref["t"][diff] < rays["t"][diff]))
    finally:
        vox_ref.lib.vref_free(h)


def _tlas_instances(n, seed, n_sets):
    rng = np.random.default_rng(seed)
    T = np.zeros((n, 4, 4), np.float32)
    for i in range(n):
        a = rng.normal(size=3); a /= np.linalg.norm(a)
        ang = rng.uniform(0, 2 * np.pi)
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        R = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K
        sc = rng.uniform(0.5, 2.0, 3)
        T[i, :3, :3] = R * sc[None, :]
        T[i, :3, 3] = rng.uniform(-2.5, 2.5, 3)
        T[i, 3, 3] = 1
    mask = rng.choice([0xFFFF, 0x1, 0x2, 0x100], n)
    inst = tb.make_instances(T, rng.integers(0, n_sets, n).astype(np.uint32))
    inst["mask"] = mask.astype(np.uint32)
    return inst


def test_restatement_tlas_matches_reference(vox_ref, vox_oracle):
    names = ["legocar", "rock", "block64"]
    denses = [scene_dense(n) for n in names]
    sets = [vox_oracle.build(d) for d in denses]
    hs = [vox_ref.new_set(d) for d in denses]
    inst = _tlas_instances(96, 5, len(names))
    th, gpu_nodes, idx, wald = vox_ref.tlas(inst, hs)
    try:
        rays = voxel_rays(N_RAYS, seed=12, lo=(-3, -3, -3), hi=(3, 3, 3))
        ref = vox_ref.tlas_intersect(th, rays)
        r0 = vox_oracle.intersect_tlas(wald, idx, inst, sets, rays, rule=0)
        assert np.array_equal(hit_bytes(ref), hit_bytes(r0))
        assert (hit_bytes(ref)[:, 1] != hit_bytes(rays)[:, 1]).sum() > N_RAYS // 20
        occ = vox_ref.tlas_occluded(th, rays)
        assert np.array_equal(occ, vox_oracle.occluded_tlas(wald, idx, inst, sets, rays, rule=0))
        assert np.array_equal(occ, vox_oracle.occluded_tlas(None, None, inst, sets, rays, rule=1))
        # rule 1 over every instance in index order: a subset of the rays changes, each one a nearer / tie / finite-tmax case
        r1 = vox_oracle.intersect_tlas(None, None, inst, sets, rays, rule=1)
        diff = np.nonzero((hit_bytes(r1) != hit_bytes(ref)).any(1))[0]
        print(f"TLAS: {diff.size} of {N_RAYS} rays differ between rule 0 and rule 1")
        assert diff.size < N_RAYS // 4
        assert np.all((rays["t"][diff] < np.float32(1e30)) | (r1["t"][diff] <= ref["t"][diff]))   # finite tmax, a nearer hit kept, or a tie
        # the library's host TLAS builder fills the instance records as BLASInstance::Update does in the reference
        mine = _tlas_instances(96, 5, len(names))
        tb.lib.tbvh_host_free(_update(mine, len(names)))
        assert mine.tobytes() == inst.tobytes()
    finally:
        vox_ref.lib.vref_tlas_free(th)
        for h in hs:
            vox_ref.lib.vref_free(h)


def test_rule1_does_not_depend_on_visit_order(vox_oracle):
    """rule 1 over the instances in index order and in reverse order gives the same records: what lets the device walk its TLAS in
    another order than the restatement"""
    denses = [scene_dense(n) for n in ("rock", "block64")]
    sets = [vox_oracle.build(d) for d in denses]
    inst = _tlas_instances(64, 9, 2)
    for f in ("transform", "blasIdx", "mask"):   # instances 32..63 repeat 0..31: exact ties between instances
        inst[f][32:] = inst[f][:32]
    tb.lib.tbvh_host_free(_update(inst, 2))
    rays = voxel_rays(1 << 14, seed=3, lo=(-3, -3, -3), hi=(3, 3, 3))
    a = vox_oracle.intersect_tlas(None, None, inst, sets, rays, rule=1)
    b = vox_oracle.intersect_tlas(None, None, inst, sets, rays, rule=2)
    assert np.array_equal(hit_bytes(a), hit_bytes(b))
    assert np.all(a["inst"][a["t"] != rays["t"]] < 32)   # the tied copies lose to the smaller instance


def _update(inst, n_sets):
    h = C.c_void_p()
    bounds = np.tile(np.array([0, 0, 0, 1, 1, 1], np.float32), (n_sets, 1))
    tb.check(tb.lib.tbvh_host_build_tlas(inst.ctypes.data_as(C.c_void_p), inst.shape[0], bounds.ctypes.data_as(C.c_void_p), n_sets, C.byref(h)), "tbvh_host_build_tlas")
    return h


@pytest.mark.parametrize("case", ["blas_legocar", "blas_rock", "tlas"])
def test_goldens_match_reference(case, vox_ref):
    """the committed ray sets and records are what the reference produces today (tools/make_voxel_golden.py)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_voxel_golden", os.path.join(os.path.dirname(__file__), "..", "tools", "make_voxel_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    g = np.load(os.path.join(GOLDEN, case + ".npz"))
    fresh = mod.make(vox_ref, case)
    assert sorted(g.files) == sorted(fresh)
    for k in g.files:
        assert np.array_equal(g[k], fresh[k]), (case, k)
