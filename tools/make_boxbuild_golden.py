"""Records the real reference's builds over boxes (threadedBuild = false, through tests/boxbuild_ref_shim.cpp) into tests/golden/boxbuild/*.npz:
BVH::BuildAABB and BVH::Build( customGetAABB, n ) over the sets of boxbuild_lib.SETS, BVH_GPU::Build( BLASInstance*, .. ) over boxbuild_lib.TLAS_SIZES
updated instance records.  Each file holds the node bytes (of the larger trees their count and SHA-256 only) and primIdx with every leaf's range
sorted.  Results only; tests/test_boxbuild_host.py regenerates the same arrays where the reference is present.

    python tools/make_boxbuild_golden.py
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import boxbuild_lib as bl  # noqa: E402


def main():
    os.makedirs(bl.GOLDEN, exist_ok=True)
    with tempfile.TemporaryDirectory() as d:
        ref = bl.compile_ref_shim(d)
        assert ref is not None, "the reference checkout (TBVH_REFERENCE) is absent"
        for name in bl.golden_names():
            out = bl.make_golden(ref, name)
            np.savez_compressed(bl.golden_path(name), **out)
            print(name, int(out["n_nodes"]), "nodes", os.path.getsize(bl.golden_path(name)), "bytes")


if __name__ == "__main__":
    main()
