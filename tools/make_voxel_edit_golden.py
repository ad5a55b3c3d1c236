"""Writes the voxel editing goldens under tests/golden/voxeledit/: seeded hit records and the normals the REAL reference's VoxelSet::GetNormal
gave for them (tests/voxel_edit_ref_shim.cpp, compiled from $TBVH_REFERENCE/tiny_bvh.h).  The GPU tests read these files and never the
reference; tests/test_voxel_edit_host.py regenerates every case with make() and compares, so the files cannot go stale.

    python tools/make_voxel_edit_golden.py            (needs the reference checkout)

  voxelize_*    the voxel set tiny_bvh_foliage.cpp's scene-to-voxels loop leaves for a closed box, three tilted quads and an alpha-cut quad: with a
                shading table, with a constant colour (both with dyadic bounds, for which the ray origins are exact whatever is contracted), as a
                two-instance TLAS and with the demo's own cube of the scene's bounds (where the origin's fused multiply-add matters); plus the
                records made, the reference's maximum hits per ray and its number of rays with more than two hits
  normals       hit records of one set (object space)
  normals_tlas  hit records of a TLAS of rotated (quarter turns), scaled, translated instances, in world space, with the instances' transforms;
                the reference's normal is GetNormal of the same record in the hit instance's space.  The transforms, origins and directions lie on
                dyadic grids, so taking a record into the instance's space is exact whatever a compiler contracts: the golden holds the
                reference's answer and nobody's rounding.  (General rotations are compared between the device and the CPU twin instead.)
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, os.path.join(HERE, ".."))

import voxel_edit_lib as E  # noqa: E402

CASES = ["normals", "normals_tlas"] + ["voxelize_" + c for c in E.VOXELIZE_CASES]
N_RAYS = 4096
N_INST = 24


def make(case, ref):
    rays = E.normal_rays(N_RAYS, seed=51)
    if case == "normals":
        return {"rays": rays, "normals": ref.normals(rays)}
    if case == "normals_tlas":
        inst = E.exact_instances(N_INST, seed=52)
        world, obj = E.exact_world_rays(rays, inst, seed=53)
        return {"rays": world, "transforms": inst["transform"].copy(), "normals": ref.normals(obj)}
    if case.startswith("voxelize_"):
        # the set the reference's loop leaves (tiny_bvh_foliage.cpp:222-258 over voxel_edit_lib.voxelize_scene), with the loop's own statistics.  The scene
        # is chosen so that the reference alone stays within the device's cap of the tests: asserted here, and stored
        g = E.reference_voxelize(ref, case[9:])
        assert int(g["max_hits"]) <= E.VOXELIZE_MAX_HITS, (case, int(g["max_hits"]))
        assert int(g["rays_over_2"]) > 0 and int(g["records"]) > 0
        return g
    raise KeyError(case)


def main():
    ref = E.compile_edit_ref_shim(tempfile.mkdtemp())
    assert ref is not None, "the reference checkout (TBVH_REFERENCE) is needed"
    os.makedirs(E.GOLDEN_EDIT, exist_ok=True)
    for case in CASES:
        path = os.path.join(E.GOLDEN_EDIT, case + ".npz")
        np.savez_compressed(path, **make(case, ref))
        print(case, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
