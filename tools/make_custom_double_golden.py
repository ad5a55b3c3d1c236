#!/usr/bin/env python
"""Writes tests/golden/custom_double/<set>.npz from the real reference (tests/custom_double_ref_shim.cpp over $TBVH_REFERENCE/tiny_bvh.h): per sphere set
the tree BVH_Double::Build( customGetAABB, n ) makes (bvhNode, primIdx) and, for the camera and bounce batches of tests/custom_double_lib.py, the rays and
the records BVH_Double::Intersect leaves.  Data only: the spheres themselves are made by the tests.  usage: tools/make_custom_double_golden.py"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import custom_double_lib as L  # noqa: E402

with tempfile.TemporaryDirectory() as d:
    ref = L.compile_ref_shim(d)
    assert ref is not None, "the reference checkout (TBVH_REFERENCE) is absent"
    ocd = L.compile_oracle(d)
    os.makedirs(L.GOLDEN, exist_ok=True)
    for name in L.GOLDEN_SETS:
        sph = L.sphere_set(name)
        h = ref.build_spheres(sph)
        nodes, idx = ref.blob(h)
        out = {"nodes": nodes, "prim_idx": idx}
        for kind, rays in L.golden_rays(name, ocd).items():
            out[kind + "_rays"] = rays
            traced = ref.intersect(h, rays)
            out[kind + "_t"], out[kind + "_prim"], out[kind + "_inst"] = traced["t"], traced["prim"], traced["inst"]
            assert all(np.array_equal(traced[f], rays[f]) for f in ("O", "D", "u", "v", "instIdx", "mask"))   # (what a sphere hit leaves alone)
        ref.free(h)
        path = os.path.join(L.GOLDEN, name + ".npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), "bytes;", len(nodes), "nodes")
