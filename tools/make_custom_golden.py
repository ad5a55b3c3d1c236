"""Writes tests/golden/custom/*.npz: trees the real reference built over sphere sets (BVH::Build( customGetAABB, n ), tests/custom_ref_shim.cpp),
the rays, and the reference's own records (BVH::Intersect / IsOccluded with the anim demo's sphere callback); and an anim-like TLAS (scaled and
rotated sphere-bunny instances plus a triangle BLAS, some masked) with its TLAS and triangle BLAS also as BVH_GPU::ConvertFrom of the reference's
trees (the form tbvh_upload_tlas takes).  Needs the reference checkout (TBVH_REFERENCE).  Usage: python tools/make_custom_golden.py"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tinybvh_amd as tb  # noqa: E402
from custom_lib import GOLDEN, compile_ref_shim, decorate, rays_for, sphere_set  # noqa: E402
from test_custom_host import anim_scene, tlas_rays  # noqa: E402


def main():
    os.makedirs(GOLDEN, exist_ok=True)
    ref = compile_ref_shim(tempfile.mkdtemp())
    assert ref is not None, "the reference checkout is needed"
    for name, n in (("bunny16", 1000), ("soup", 1000)):
        sph = sphere_set(name)
        h = ref.build_spheres(sph)
        rays = np.concatenate([decorate(rays_for(sph, n, 41 + i, k), 51 + i) for i, k in enumerate(("camera", "incoherent", "inside"))])
        hits = ref.intersect(h, rays)
        occ = ref.occluded(h, rays)
        np.savez_compressed(os.path.join(GOLDEN, f"blas_{name}.npz"), nodes=ref.blob(h, 0), prim_idx=ref.blob(h, 1), spheres=sph,
                            rays=rays.view(np.uint8), hits=hits.view(np.uint8), occluded=occ)
        ref.free(h)
    sph, tris, inst = anim_scene(spheres="bunny16", n_tris=1200)
    hs, ht = ref.build_spheres(sph), ref.build_tris(tris)
    th = ref.tlas_build(inst, [hs, ht])
    rays = tlas_rays(800, 61)
    np.savez_compressed(os.path.join(GOLDEN, "tlas_anim.npz"), tlas_nodes=ref.tlas_blob(th, 2), tlas_nodes64=ref.tlas_blob(th, 0),
                        tlas_idx=ref.tlas_blob(th, 1), instances=inst.view(np.uint8), sph_nodes=ref.blob(hs, 0), sph_idx=ref.blob(hs, 1),
                        spheres=sph, tri_nodes=ref.blob(ht, 0), tri_nodes64=ref.blob(ht, 2), tri_idx=ref.blob(ht, 1), tri_verts=tris,
                        sph_set=np.array("bunny16"), n_tris=np.array(1200),
                        rays=rays.view(np.uint8), hits=ref.tlas_intersect(th, rays).view(np.uint8), occluded=ref.tlas_occluded(th, rays))
    ref.tlas_free(th); ref.free(hs); ref.free(ht)
    for f in sorted(os.listdir(GOLDEN)):
        print(f, os.path.getsize(os.path.join(GOLDEN, f)), "bytes")


if __name__ == "__main__":
    main()
