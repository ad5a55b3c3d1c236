"""Records the real reference's BVH::Build (threadedBuild = false, through tests/sahbuild_ref_shim.cpp) for the scenes of sahbuild_lib.GOLDEN_SCENES
into tests/golden/sahbuild/*.npz: the Wald nodes (or, where they would exceed the size the fixtures keep to, their count and SHA-256 only) and
primIdx with every leaf's range sorted.  Results only; tests/test_sahbuild_host.py regenerates the same bytes where the reference is present.

    python tools/make_sahbuild_golden.py
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sahbuild_lib as sl  # noqa: E402

MAX_NODE_BYTES = 256 << 10


def main():
    os.makedirs(sl.GOLDEN, exist_ok=True)
    with tempfile.TemporaryDirectory() as d:
        ref = sl.compile_ref_shim(d)
        assert ref is not None, "the reference checkout (TBVH_REFERENCE) is absent"
        for name in sl.GOLDEN_SCENES:
            nodes, idx = ref.build(sl.scene(name))
            out = {"sha256": np.array(sl.node_digest(nodes)), "n_nodes": np.array(nodes.shape[0], np.uint32), "prim_idx": sl.leaf_sets(nodes, idx)}
            if nodes.nbytes <= MAX_NODE_BYTES:
                out["nodes"] = nodes
            np.savez_compressed(sl.golden_path(name), **out)
            print(name, nodes.shape[0], "nodes", os.path.getsize(sl.golden_path(name)), "bytes")


if __name__ == "__main__":
    main()
