"""Records the real reference's BVH::BuildHQ (threadedBuild = false, through oracle/_ref) for the scenes of sbvhbuild_lib.GOLDEN_SCENES into
tests/golden/sbvhbuild/*.npz: the Wald nodes (GOLDEN_FULL) or their count and SHA-256 only (GOLDEN_HASHED), and the used prefix of primIdx.
Results only; tests/test_sbvhbuild_host.py regenerates the same bytes where the reference is present.

    python tools/make_sbvhbuild_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sahbuild_lib as sl  # noqa: E402
import sbvhbuild_lib as ql  # noqa: E402
from oracle_lib import Reference, have_reference  # noqa: E402


def main():
    assert have_reference(), "oracle/_ref/libtinybvh_ref.so is not built (it needs the reference checkout at build time)"
    ref = Reference()
    os.makedirs(ql.GOLDEN, exist_ok=True)
    for name in ql.GOLDEN_SCENES:
        nodes, idx = ql.ref_flat(ref, ql.scene(name))
        out = {"sha256": np.array(sl.node_digest(nodes)), "n_nodes": np.array(nodes.shape[0], np.uint32), "prim_idx": idx}
        if name in ql.GOLDEN_FULL:
            out["nodes"] = nodes
        np.savez_compressed(ql.golden_path(name), **out)
        print(name, nodes.shape[0], "nodes", idx.size, "references", os.path.getsize(ql.golden_path(name)), "bytes")


if __name__ == "__main__":
    main()
