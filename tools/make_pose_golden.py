"""Regenerate tests/golden/pose/*.npz from the REAL reference's Mesh::SetPose (tests/pose_lib.py: make_golden; needs the reference checkout,
TBVH_REFERENCE).  The inputs are pose_lib's deterministic generators; tests/test_pose_host.py holds the files to them and to the restatement."""
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import pose_lib as P  # noqa: E402

if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as d:
        ref = P.compile_ref_shim(d)
        if ref is None:
            sys.exit("the reference checkout (TBVH_REFERENCE) is absent")
        P.make_golden(ref)
    for f in sorted(os.listdir(P.GOLDEN)):
        print(f, os.path.getsize(os.path.join(P.GOLDEN, f)), "bytes")
