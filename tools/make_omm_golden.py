"""Regenerate tests/golden/omm/*.npz from the REAL reference's CreateOpacityMicroMap (tests/omm_lib.py: make_golden; needs the reference checkout,
TBVH_REFERENCE).  The inputs are omm_lib's deterministic generators; make_golden itself checks that the reference's words are not vacuous (between 20 and
80 % of the bits set, at least half of the textured triangles mixed, one fully clear, one fully set), and tests/test_omm_host.py holds the files to the
generators and to the restatement."""
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import omm_lib as O  # noqa: E402

if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as d:
        ref = O.compile_ref_shim(d)
        if ref is None:
            sys.exit("the reference checkout (TBVH_REFERENCE) is absent")
        O.make_golden(ref)
    for N in O.GOLDEN_N:
        g = O.golden(N)
        print(f"mixed_n{N}.npz", os.path.getsize(os.path.join(O.GOLDEN, f"mixed_n{N}.npz")), "bytes; set share, mixed share, clear, full:",
              O.map_stats(g["words"], g["tri_texture"], N))
