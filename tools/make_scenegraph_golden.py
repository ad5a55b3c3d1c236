#!/usr/bin/env python
"""Writes tests/golden/graph/*.npz through the real reference (tests/scenegraph_ref_shim.cpp, compiled from $TBVH_REFERENCE) and derives the tolerance of slerp's
trigonometric branch (tests/oracle_scenegraph.c).  usage: python tools/make_scenegraph_golden.py"""
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import scenegraph_lib as L  # noqa: E402

with tempfile.TemporaryDirectory() as d:
    ref = L.compile_ref_shim(d)
    assert ref is not None, "the reference checkout is needed (TBVH_REFERENCE)"
    for name, out in zip(("synthetic", "drone"), L.make_golden(ref, L.compile_oracle(d))):
        u, D, bound = out["trig_bound"]
        print(f"{name}: {out['t'].shape[0]} frames, exact {out['exact_frames'].tolist()}, trigonometric {out['trig_frames'].tolist()}; "
              f"u = {u:g} ulp, D = {D:.3e} over {int(out['trig_intervals'])} intervals of both fixtures, bound = {bound:.3e}")
