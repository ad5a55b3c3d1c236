"""tbvh_host_build_bvh2_sah — the CPU twin of the device SAH builder over csrc/sah_split.h — against the real reference's BVH::Build
(threadedBuild = false; tests/sahbuild_ref_shim.cpp): node for node and byte for byte, every leaf's primitive set the reference's (DESIGN.md par. 18).
No GPU.  The recorded fixtures (tests/golden/sahbuild, tools/make_sahbuild_golden.py) are regenerated here, which pins them to the reference."""
import numpy as np
import pytest

import tinybvh_amd as tb
import mesh_lib
import sahbuild_lib as sl
from sahbuild_lib import sah_ref  # noqa: F401  (fixture)

SMALL = ["SOUP1", "SOUP2", "SOUP3", "SOUP5", "SOUP9", "SOUP64", "SOUP65", "S", "FAR", "FLAT", "POINT", "TWO", "QUADS", "LATTICE"]
MEDIUM = ["ATRIUM30K", "STREET45K", "BLOB20K"]
LARGE = ["ATRIUM262K"]   # (one of the three large scenes: the file stays within some 20 s)


@pytest.mark.parametrize("name", SMALL + MEDIUM + LARGE)
def test_host_twin_is_the_reference_tree(sah_ref, name):
    v = sl.scene(name)
    ref_nodes, ref_idx = sah_ref.build(v)
    nodes, idx = tb.host_build_bvh2_sah(v)
    sl.assert_same_tree(nodes, idx, ref_nodes, ref_idx, name)


def walk_bvh2(nodes, idx, verts, max_leaf):
    """every primitive in exactly one leaf, leaves of at most max_leaf, every leaf's box is the bounds of its triangles (the halves of a split leaf
    included), every child box lies in its parent's"""
    f = nodes.view(np.float32)
    tri = verts[:, :3].reshape(-1, 3, 3)
    seen = np.zeros(tri.shape[0], np.int32)
    stack, visited = [0], 0
    while stack:
        i = stack.pop()
        visited += 1
        first, count = int(nodes[i, 3]), int(nodes[i, 7])
        if count:
            assert max_leaf == 0 or count <= max_leaf, f"leaf {i} holds {count}"
            p = idx[first:first + count]
            assert np.array_equal(p, np.sort(p)), f"leaf {i} is not ascending"
            seen[p] += 1
            assert (tri[p].min(axis=(0, 1)) == f[i, 0:3]).all() and (tri[p].max(axis=(0, 1)) == f[i, 4:7]).all(), f"leaf {i}: the box is not the bounds of its triangles"
        else:
            for c in (first, first + 1):
                assert 1 < c < nodes.shape[0]
                assert (f[c, 0:3] >= f[i, 0:3]).all() and (f[c, 4:7] <= f[i, 4:7]).all(), f"child {c} leaves node {i}"
                stack.append(c)
    assert (seen == 1).all(), "a primitive is in no leaf or in two"
    assert visited == nodes.shape[0] - 1, "unreachable nodes"


@pytest.mark.parametrize("k", [3, 4])
@pytest.mark.parametrize("name", ["S", "FLAT", "POINT", "STREET45K"])
def test_split_leafs(sah_ref, name, k):
    v = sl.scene(name)
    ref_nodes, ref_idx = sah_ref.build(v)
    nodes, idx = tb.host_build_bvh2_sah(v, max_leaf_tris=k)
    n = ref_nodes.shape[0]
    became_interior = (ref_nodes[:, 7] > k)
    same = ~became_interior
    assert np.array_equal(nodes[:n][same], ref_nodes[same]), "a node the split did not touch differs from the reference's"
    assert np.array_equal(nodes[:n][became_interior][:, [0, 1, 2, 4, 5, 6]], ref_nodes[became_interior][:, [0, 1, 2, 4, 5, 6]]), "a split leaf's box changed"
    assert (nodes[:n][became_interior][:, 7] == 0).all() and (nodes[:n][became_interior][:, 3] >= n).all()
    # the reference's own SplitLeafs makes as many nodes
    split_nodes, _ = sah_ref.build(v, split_leafs=k)
    assert nodes.shape[0] == split_nodes.shape[0]
    assert np.array_equal(idx, sl.leaf_sets(ref_nodes, ref_idx)), "SplitLeafs moved primitives"
    walk_bvh2(nodes, idx, v, k)


def test_indexed_form_equals_flat():
    pos, ind = mesh_lib.bunny()
    flat = mesh_lib.flatten(pos, ind)
    a = tb.host_build_bvh2_sah(flat)
    b = tb.host_build_bvh2_sah(pos, indices=ind)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_indexed_form_is_the_reference_s(sah_ref):
    pos, ind = mesh_lib.bunny()
    ref_nodes, ref_idx = sah_ref.build(pos, indices=ind)
    nodes, idx = tb.host_build_bvh2_sah(pos, indices=ind)
    sl.assert_same_tree(nodes, idx, ref_nodes, ref_idx, "bunny, indexed")


@pytest.mark.parametrize("name", sl.GOLDEN_SCENES)
def test_fixtures_are_the_reference_s(sah_ref, name):
    v = sl.scene(name)
    ref_nodes, ref_idx = sah_ref.build(v)
    sl.assert_matches_golden(name, ref_nodes, sl.leaf_sets(ref_nodes, ref_idx), "reference")


@pytest.mark.parametrize("name", sl.GOLDEN_SCENES)
def test_host_twin_matches_the_fixtures(name):
    nodes, idx = tb.host_build_bvh2_sah(sl.scene(name))
    sl.assert_matches_golden(name, nodes, idx, "host twin")


def test_errors():
    import ctypes as C
    v = sl.scene("SOUP9")
    m, keep = tb._mesh(v)
    n = C.c_uint64(0)
    lib = tb.lib
    assert lib.tbvh_host_build_bvh2_sah(None, 0, None, 0, None, 0, C.byref(n)) == -1
    assert lib.tbvh_host_build_bvh2_sah(C.byref(m), 0, None, 0, None, 0, None) == -1
    assert lib.tbvh_host_build_bvh2_sah(C.byref(m), 0, None, 0, None, 0, C.byref(n)) == 0 and n.value == tb.host_build_bvh2_sah(v)[0].shape[0]
    nodes = np.zeros((2, 8), np.uint32); idx = np.zeros(9, np.uint32)
    need = n.value
    n.value = 0
    assert lib.tbvh_host_build_bvh2_sah(C.byref(m), 0, nodes.ctypes.data, 2, idx.ctypes.data, 9, C.byref(n)) == -1 and n.value == need
    assert not nodes.any()
    bad = np.array([0, 1, 99], np.uint32)
    mb, keep2 = tb._mesh(v, bad)
    assert lib.tbvh_host_build_bvh2_sah(C.byref(mb), 0, None, 0, None, 0, C.byref(n)) == -5   # TBVH_E_FORMAT: host indices are checked first
