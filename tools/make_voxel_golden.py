"""Writes the VoxelSet goldens under tests/golden/voxels/: seeded ray sets and the records the REAL reference produced for them
(tests/voxel_ref_shim.cpp, compiled from $TBVH_REFERENCE/tiny_bvh.h).  The GPU tests read these files and never the reference;
tests/test_voxel_host.py regenerates every case with make() and compares, so the files cannot go stale.

    python tools/make_voxel_golden.py            (needs the reference checkout)
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, os.path.join(HERE, ".."))

import tinybvh_amd as tb  # noqa: E402
import voxel_lib as V  # noqa: E402

CASES = ["blas_legocar", "blas_rock", "tlas"]
N_RAYS = 8192
TLAS_SETS = ["legocar", "rock"]


def tlas_instances(n, seed, n_sets):
    """rotated, scaled, translated instances with a mix of masks"""
    rng = np.random.default_rng(seed)
    T = np.zeros((n, 4, 4), np.float32)
    for i in range(n):
        a = rng.normal(size=3); a /= np.linalg.norm(a)
        ang = rng.uniform(0, 2 * np.pi)
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        R = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K
        T[i, :3, :3] = R * rng.uniform(0.5, 2.0, 3)[None, :]
        T[i, :3, 3] = rng.uniform(-2.5, 2.5, 3)
        T[i, 3, 3] = 1
    inst = tb.make_instances(T, rng.integers(0, n_sets, n).astype(np.uint32))
    inst["mask"] = rng.choice([0xFFFF, 0x1, 0x2, 0x100], n).astype(np.uint32)
    return inst


def make(ref, case):
    """the golden of one case as a dict of arrays: rays (as given), hits (rays after the reference's Intersect), occ (IsOccluded)"""
    out = {"case": np.array(case)}
    if case.startswith("blas_"):
        dense = V.scene_dense(case[5:])
        h = ref.new_set(dense)
        try:
            rays = V.voxel_rays(N_RAYS, seed=101 + CASES.index(case), dense=dense)
            out.update(rays=rays, hits=ref.intersect(h, rays), occ=ref.occluded(h, rays))
        finally:
            ref.lib.vref_free(h)
        return out
    hs = [ref.new_set(V.scene_dense(n)) for n in TLAS_SETS]
    inst = tlas_instances(64, 7, len(TLAS_SETS))
    th, gpu_nodes, idx, wald = ref.tlas(inst, hs)   # (inst: BLASInstance::Update's records)
    try:
        rays = V.voxel_rays(N_RAYS, seed=150, lo=(-3, -3, -3), hi=(3, 3, 3))
        out.update(rays=rays, hits=ref.tlas_intersect(th, rays), occ=ref.tlas_occluded(th, rays), instances=inst, tlas_nodes=gpu_nodes,
                   tlas_idx=idx, tlas_wald=wald)
    finally:
        ref.lib.vref_tlas_free(th)
        for h in hs:
            ref.lib.vref_free(h)
    return out


def main():
    with tempfile.TemporaryDirectory() as d:
        ref = V.compile_ref_shim(d)
        if ref is None:
            sys.exit("the reference checkout is absent (set TBVH_REFERENCE)")
        for case in CASES:
            g = make(ref, case)
            path = os.path.join(V.GOLDEN, case + ".npz")
            np.savez_compressed(path, **g)
            print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
