"""The CPU twins of the SAH builder over boxes — tbvh_host_build_bvh2_sah_aabbs, tbvh_host_build_bvh2_sah_spheres, tbvh_host_build_tlas_sah, all over
csrc/sah_split.h — against the real reference's BVH::BuildAABB, BVH::Build( customGetAABB, n ), BVH::Build( BLASInstance*, .. ) and
BVH_GPU::Build( BLASInstance*, .. ), node for node and byte for byte, and the fixtures of tests/golden/boxbuild against both (DESIGN.md par. 20)."""
import ctypes as C

import numpy as np
import pytest

import tinybvh_amd as tb
import boxbuild_lib as bl
from boxbuild_lib import box_ref  # noqa: F401  (fixture)

lib = tb.lib


@pytest.mark.parametrize("name", bl.SETS)
def test_box_twin_is_the_reference_s_BuildAABB(box_ref, name):
    nodes, idx = tb.host_build_bvh2_sah_boxes(bl.boxes(name))
    ref_nodes, ref_idx = box_ref.build(bl.RefBox.AABBS, bl.boxes(name))
    bl.assert_same_tree(nodes, idx, ref_nodes, ref_idx, name)


def test_the_sets_reach_what_they_are_for(box_ref):
    n, i = box_ref.build(bl.RefBox.AABBS, bl.boxes("LATTICE1000"))
    assert n.shape[0] == 2000 and set(n[n[:, 7] > 0, 7]) == {1}, "LATTICE1000: 2000 nodes, every leaf one box"
    n, i = box_ref.build(bl.RefBox.AABBS, bl.boxes("IDENT700"))
    assert n.shape[0] == 2 and n[0, 7] == 700, "IDENT700: one leaf of 700"
    n, i = box_ref.build(bl.RefBox.AABBS, bl.boxes("GEO256"))
    assert n.shape[0] == 4 and 247 in n[:, 7], "GEO256: two leaves, one of 247 boxes (the rootExtent * 1e-20f gate)"
    n, i = box_ref.build(bl.RefBox.AABBS, bl.boxes("MIXED1000"))
    assert n[:, 7].max() > 1, "MIXED1000: some leaf holds more than one box"


@pytest.mark.parametrize("name", bl.SETS)
def test_sphere_twin_is_the_reference_s_custom_build(box_ref, name):
    nodes, idx = tb.host_build_bvh2_sah_spheres(bl.spheres(name))
    ref_nodes, ref_idx = box_ref.build(bl.RefBox.SPHERES, bl.spheres(name))
    bl.assert_same_tree(nodes, idx, ref_nodes, ref_idx, name + " as spheres")


@pytest.mark.parametrize("n", bl.TLAS_SIZES)
def test_tlas_twin_is_the_reference_s(box_ref, n):
    inst = bl.instances(n)
    # the Wald tree: the instance source of the seam is the box-pair source at float4 8 and 9 of a record
    pairs = np.zeros((n, 8), np.float32)
    pairs[:, 0:3] = inst["aabbMin"]; pairs[:, 4:7] = inst["aabbMax"]
    ref_nodes, ref_idx = box_ref.build(bl.RefBox.TLAS_WALD, inst)
    nodes, idx = tb.host_build_bvh2_sah_boxes(pairs)
    bl.assert_same_tree(nodes, idx, ref_nodes, ref_idx, f"TLAS over {n} instances, Wald")
    # the Aila-Laine bytes: encode_bvh_gpu of the twin's tree against BVH_GPU::Build (BVH_GPU::ConvertFrom)
    al, al_idx = tb.host_build_tlas_sah(inst)
    ref_al, ref_al_idx = box_ref.build(bl.RefBox.TLAS_GPU, inst)
    assert al.shape[0] == ref_al.shape[0] == max(ref_nodes.shape[0] - 1, 1), "usedNodes - 1 Aila-Laine nodes (the pad node is not emitted)"
    assert np.array_equal(al, ref_al[:al.shape[0]]), f"TLAS over {n} instances: Aila-Laine nodes differ"
    assert np.array_equal(al_idx, bl.al_leaf_sets(ref_al, ref_al_idx))


def test_fixtures_are_what_the_reference_builds(box_ref):
    for name in bl.golden_names():
        want, have = bl.make_golden(box_ref, name), bl.load_golden(name)
        assert sorted(want) == sorted(have), name
        for k in want:
            assert np.array_equal(want[k], have[k]), f"{name}: {k} differs from the committed fixture"


@pytest.mark.parametrize("name", bl.SETS)
def test_twins_match_the_fixtures(name):
    """without the reference: the twins against what it built"""
    bl.assert_matches_golden(f"boxes_{name}", *tb.host_build_bvh2_sah_boxes(bl.boxes(name)), "twin")
    bl.assert_matches_golden(f"spheres_{name}", *tb.host_build_bvh2_sah_spheres(bl.spheres(name)), "twin")


@pytest.mark.parametrize("n", bl.TLAS_SIZES)
def test_tlas_twin_matches_the_fixture(n):
    bl.assert_matches_golden(f"tlas_{n}", *tb.host_build_tlas_sah(bl.instances(n)), "twin")


def check_structure(nodes, idx, n):
    """every node reached once from the root, children behind their parents' pair, the leaves' ranges a partition of [0, n), primIdx a permutation"""
    assert np.array_equal(np.sort(idx), np.arange(n, dtype=np.uint32)), "primIdx is not a permutation"
    assert not nodes[1].any(), "node 1 is not zero"
    seen, covered, todo = np.zeros(nodes.shape[0], bool), np.zeros(n, np.uint32), [0]
    while todo:
        i = todo.pop()
        assert not seen[i]
        seen[i] = True
        first, count = int(nodes[i, 3]), int(nodes[i, 7])
        if count:
            assert first + count <= n
            covered[first:first + count] += 1
            assert np.all(np.diff(idx[first:first + count].astype(np.int64)) > 0), "a leaf's primitives are not ascending"
        else:
            assert 2 <= first and first + 1 < nodes.shape[0]
            todo += [first, first + 1]
    assert np.all(covered == 1) and seen[0] and np.all(seen[2:]) and not seen[1]


@pytest.mark.parametrize("case", ["nan_box", "inverted_box", "r_zero", "r_negative", "all_nan"])
def test_twin_terminates_on_input_the_reference_leaves_undefined(case):
    """the device builder shares the header: this is where termination with a structurally valid tree is shown for such input (no GPU test feeds NaNs)"""
    b = np.array(bl.boxes("MIXED65")); s = np.array(bl.spheres("MIXED65"))
    if case == "nan_box":
        b[17, 0:3] = np.nan
    elif case == "all_nan":
        b[:, 0:3] = np.nan; b[:, 4:7] = np.nan
    elif case == "inverted_box":
        b[17, 0:3], b[17, 4:7] = b[17, 4:7].copy(), b[17, 0:3].copy()
    elif case == "r_zero":
        s[::3, 3] = 0
    else:
        s[::3, 3] = -1.5
    nodes, idx = tb.host_build_bvh2_sah_spheres(s) if case.startswith("r_") else tb.host_build_bvh2_sah_boxes(b)
    check_structure(nodes, idx, 65)
    nodes, idx = tb.host_build_bvh2_sah_spheres(s, max_leaf=2) if case.startswith("r_") else tb.host_build_bvh2_sah_boxes(b, max_leaf=2)
    check_structure(nodes, idx, 65)
    assert nodes[:, 7].max() <= 2


def test_split_leafs_over_boxes():
    nodes, idx = tb.host_build_bvh2_sah_boxes(bl.boxes("IDENT700"), max_leaf=4)
    check_structure(nodes, idx, 700)
    assert nodes[:, 7].max() == 4 and nodes.shape[0] == 2 + 2 * (700 // 4 - 1)


def test_refusals():
    b = bl.boxes("MIXED3")
    n = C.c_uint64(0)
    for fn in (lib.tbvh_host_build_bvh2_sah_aabbs, lib.tbvh_host_build_bvh2_sah_spheres):
        assert fn(None, 3, 0, None, 0, None, 0, C.byref(n)) == -1 and fn.__name__.encode() in lib.tbvh_last_error()
        assert fn(b.ctypes.data, 0, 0, None, 0, None, 0, C.byref(n)) == -1
        assert fn(b.ctypes.data, 1 << 31, 0, None, 0, None, 0, C.byref(n)) == -1
        assert fn(b.ctypes.data, 3, 0, None, 0, None, 0, None) == -1
        assert fn(b.ctypes.data, 3, 0, None, 0, None, 0, C.byref(n)) == 0 and n.value >= 2   # the count alone
        nodes = np.zeros((1, 8), np.uint32); idx = np.zeros(3, np.uint32)
        assert fn(b.ctypes.data, 3, 0, nodes.ctypes.data, 1, idx.ctypes.data, 3, C.byref(n)) == -1 and not nodes.any()
    inst = bl.instances(3)
    assert lib.tbvh_host_build_tlas_sah(None, 3, None, 0, None, 0, C.byref(n)) == -1 and b"tbvh_host_build_tlas_sah" in lib.tbvh_last_error()
    assert lib.tbvh_host_build_tlas_sah(inst.ctypes.data, 0, None, 0, None, 0, C.byref(n)) == -1
    assert lib.tbvh_host_build_tlas_sah(inst.ctypes.data, 1 << 31, None, 0, None, 0, C.byref(n)) == -1
    assert lib.tbvh_host_build_tlas_sah(inst.ctypes.data, 3, None, 0, None, 0, C.byref(n)) == 0 and n.value >= 1
