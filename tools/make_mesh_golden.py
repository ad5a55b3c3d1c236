"""Writes tests/golden/mesh/*.npz from the REAL reference (tests/mesh_ref_shim.cpp, compiled from $TBVH_REFERENCE/tiny_bvh.h): an indexed mesh
(every 24th triangle of the committed bunny, vertices compacted), the BVH_GPU the reference builds over it with BVH_GPU::Build( slice, indices, n )
(bvhNode, primIdx, the Wald nodes it came from), 3 000 rays with BVH::Intersect records and IsOccluded flags, 3 000 spheres with IntersectSphere
flags, and all of it again after the shared vertices moved and BVH::Refit + BVH_GPU::ConvertFrom ran.  The mesh is below the reference's
threshold for threaded builds, so the blobs are reproducible.  Spheres on which the reference's walk does not terminate (DESIGN.md par. 11,
defect 1) are found with the verbatim restatement first, never handed to the reference, and stored as 255; `agree` marks those on which its walk
took no leaf off the stack, where the library's answer must be the reference's.
Run: python tools/make_mesh_golden.py  (needs the reference checkout and a C compiler; no GPU)."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_lib as ml  # noqa: E402
import sphere_lib as sl  # noqa: E402


def make(ref, orc):
    """the arrays of the golden file, made now (tests/test_mesh_host.py compares the committed file with this)"""
    pos, idx = ml.bunny(ml.GOLDEN_STEP)
    flat = ml.flatten(pos, idx)
    rays, sp = ml.golden_rays(flat), ml.golden_spheres(flat)
    h = ref.build(pos, idx)
    out = {"positions": pos, "indices": idx, "rays": rays.view(np.uint8), "spheres": sp}
    for tag, p in (("", pos), ("_refit", ml.moved(pos))):
        if tag:
            ref.refit(h, p)
            out["positions_refit"] = p
        f = ml.flatten(p, idx)
        n32, pi = ref.blob(h, 2), ref.blob(h, 1)
        verb = orc.wald(n32, pi, f, sp, mode=0)
        ok = verb != 2
        ans = np.full(sp.shape[0], 255, np.uint8)
        ans[ok] = ref.spheres(h, sp[ok])
        out.update({"bvhgpu_nodes" + tag: ref.blob(h, 0), "prim_idx" + tag: pi, "wald_nodes" + tag: n32,
                    "hits" + tag: ref.intersect(h, rays).view(np.uint8), "occluded" + tag: ref.occluded(h, rays),
                    "sphere_answers" + tag: ans, "sphere_agree" + tag: ok & ((verb & 4) == 0)})
    ref.free(h)
    return out


def main():
    d = tempfile.mkdtemp()
    ref, orc = ml.compile_ref_shim(d), sl.compile_oracle(d)
    assert ref is not None, "the reference checkout (TBVH_REFERENCE) is absent"
    os.makedirs(ml.GOLDEN, exist_ok=True)
    g = make(ref, orc)
    path = os.path.join(ml.GOLDEN, "bunny_indexed.npz")
    np.savez_compressed(path, **g)
    hits = g["hits"].view(np.float32).reshape(-1, 16)[:, 12]
    print(path, os.path.getsize(path), "bytes;", int((hits < 1e30).sum()), "hits,", int((g["sphere_answers"] == 1).sum()), "spheres touch,",
          int((g["sphere_answers"] == 255).sum()), "not terminating,", int(g["sphere_agree"].sum()), "agree")


if __name__ == "__main__":
    main()
