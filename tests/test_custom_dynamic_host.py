"""Sphere BLASes that move, without a GPU (DESIGN.md par. 12): the numpy restatement of the refit rule the GPU tests share reproduces the
host builder's boxes, and the new calls are declared and bound."""
import os
import re

import numpy as np
import pytest

import tinybvh_amd as tb
from tinybvh_amd import _capi
from custom_dynamic_lib import check_boxes, check_structure, node_boxes, wald_refit
from custom_lib import caterpillar, sphere_set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_CALLS = ["tbvh_build_device_custom_spheres", "tbvh_rebuild_custom_spheres_device", "tbvh_refit_custom_spheres", "tbvh_custom_spheres_download"]


@pytest.mark.parametrize("name", ["one", "dups", "soup", "bunny16", "bunny"])
def test_restatement_reproduces_the_host_builder(name):
    """leaf box = min of pos - r / max of pos + r over its range, interior box = min / max of the children: exactly the host builder's boxes"""
    sph = sphere_set(name)
    nodes, pi = tb.host_build_custom_spheres(sph)
    reached = check_boxes(nodes, pi, sph)
    assert reached[0] and reached.sum() >= 1
    check_structure(nodes, pi, sph.shape[0], max_leaf=pi.size, node1_unused=False)


def test_restatement_on_a_tree_out_of_builder_order():
    """the caterpillar's hand-made boxes are not the refit's (they are looser on y, z by nothing and exact on x): moved spheres give moved boxes"""
    nodes, pi, sph = caterpillar(100)
    want, reached = wald_refit(nodes, pi, sph)
    assert reached.sum() == 201 and not reached[1]
    assert np.array_equal(want[reached], node_boxes(nodes)[reached])
    moved = sph.copy(); moved[:, 1] += np.float32(0.25)
    box, _ = wald_refit(nodes, pi, moved)
    assert np.array_equal(box[0], [2.0, -0.75, -1.0, 304.0, 1.25, 1.0])


def test_new_calls_are_declared_and_bound():
    src = open(os.path.join(ROOT, "include", "tinybvh_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW_CALLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), f"{name} is not declared in include/tinybvh_amd.h"
        assert name in _capi.SYMBOLS, f"{name} is not bound in _capi.py"
    for method in ("BuildOnDevice", "RebuildOnDevice", "Refit", "Download"):
        assert callable(getattr(tb.SphereBVH, method, None)), method
