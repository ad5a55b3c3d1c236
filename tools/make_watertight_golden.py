"""Regenerates tests/golden/watertight/*.npz from the real reference (TBVH_REFERENCE) through tests/watertight_ref_shim.cpp: data only, see
tests/watertight_lib.py: make_golden.  Prints the four miss counts of every fixture."""
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
sys.path.insert(0, os.path.dirname(HERE))   # (the two-level fixture's instances are made by the library's host TLAS builder)

import watertight_lib as W   # noqa: E402

if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as d:
        refs = W.compile_ref_shims(d)
        if refs is None:
            sys.exit("the reference checkout (TBVH_REFERENCE) is absent")
        if "--tlas-only" not in sys.argv:
            W.make_golden(refs)
        W.make_tlas_golden(refs)
    for name in sorted(os.listdir(W.GOLDEN)):
        g = W.golden(name[:-4])
        if "counts" not in g.files:
            print(name, "aimed", int(g["n_aimed"]), "of", g["wt"].shape[0], "rays; Moeller-Trumbore brute force misses", int(g["mt_misses"]), "watertight 0;",
                  os.path.getsize(os.path.join(W.GOLDEN, name)), "bytes")
            continue
        print(name, "aimed", int(g["n_aimed"]), "misses MT bvh / MT brute / WT bvh / WT brute", [int(x) for x in g["counts"]], "WT brute with contraction", int(g["fma_misses"]),
              os.path.getsize(os.path.join(W.GOLDEN, name)), "bytes")
