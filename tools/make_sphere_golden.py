"""Writes tests/golden/spheres/*.npz from the REAL reference (tests/sphere_ref_shim.cpp, compiled from $TBVH_REFERENCE/tiny_bvh.h): per case a
small mesh, the reference-built blobs of the three GPU layouts (BVH_GPU from the Wald BVH, BVH4_GPU and BVH8_CWBVH by their own Build), the
sphere sets of tests/sphere_lib.py and BVH::IntersectSphere's answers.  The reference's walk does not terminate for every sphere (DESIGN.md
par. 11, defect 1): those spheres are found with the restatement's verbatim walk first, never handed to the reference, and stored with answer
255; `agree` marks the spheres on which the reference's walk took no leaf off the stack, where the library's answer must be the reference's.
Run: python tools/make_sphere_golden.py  (needs the reference checkout and a C compiler; no GPU)."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sphere_lib as sl  # noqa: E402
from tinybvh_amd import scenes  # noqa: E402

CASES = {
    "soup": lambda: sl.with_degenerate(scenes.soup(1500, seed=23)),
    "tri2": lambda: sl.mesh("tri2"),
}


def main():
    d = tempfile.mkdtemp()
    orc, ref = sl.compile_oracle(d), sl.compile_ref_shim(d)
    assert ref is not None, "the reference checkout (TBVH_REFERENCE) is absent"
    os.makedirs(sl.GOLDEN, exist_ok=True)
    for name, make in CASES.items():
        verts = make()
        h = ref.build(verts, False)
        n32, pi = ref.blob(h, 0), ref.blob(h, 1)
        sp = np.concatenate(list(sl.sphere_sets(verts, n32, seed=500 + len(name), n=800).values()))
        verb = orc.wald(n32, pi, verts, sp, mode=0)
        ok = verb != 2
        ans = np.full(sp.shape[0], 255, np.uint8)
        ans[ok] = ref.intersect(h, sp[ok])
        out = os.path.join(sl.GOLDEN, f"{name}.npz")
        np.savez_compressed(out, verts=verts, spheres=sp, answers=ans, agree=ok & ((verb & 4) == 0), wald_nodes=n32, prim_idx=pi,
                            bvh_gpu=ref.blob(h, 2), bvh4_gpu=ref.blob(h, 3), cwbvh_nodes=ref.blob(h, 4), cwbvh_tris=ref.blob(h, 5))
        print(out, os.path.getsize(out), "bytes,", sp.shape[0], "spheres,", int((~ok).sum()), "not terminating")
        ref.free(h)


if __name__ == "__main__":
    main()
