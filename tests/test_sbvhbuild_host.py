"""tbvh_host_build_bvh2_sbvh — the CPU twin of the device SBVH builder over csrc/sbvh_split.h — against the real reference's BVH::BuildHQ
(threadedBuild = false; oracle/_ref for flat arrays, tests/sbvhbuild_ref_shim.cpp for the indexed form): node for node and byte for byte, and the
used prefix of primIdx element for element (DESIGN.md par. 19).  No GPU.  The recorded fixtures (tests/golden/sbvhbuild,
tools/make_sbvhbuild_golden.py) are regenerated here, which pins them to the reference."""
import ctypes as C

import numpy as np
import pytest

import tinybvh_amd as tb
import mesh_lib
import sbvhbuild_lib as ql
from sbvhbuild_lib import sbvh_ref_indexed  # noqa: F401  (fixture)

SCENES = ["SOUP500", "S", "FAR", "FLAT", "TWO", "QUADS", "LATTICE", "POINT", "LONG300", "LONG2000", "LONGFLAT", "BLOB20K", "ATRIUMROT30K", "STREET45K",
          "STREETROT262K"]
COVERAGE = ["LONG2000", "LONGFLAT", "ATRIUMROT30K"]
_twin = {}


def twin(name):
    """(nodes, primIdx, statistics) of the host twin, built once per scene"""
    if name not in _twin:
        _twin[name] = tb.host_build_bvh2_sbvh(ql.scene(name), stats=True)
    return _twin[name]


@pytest.mark.parametrize("name", SCENES + ql.SOUPS)
def test_host_twin_is_the_reference_tree(reference, name):
    nodes, idx, st = twin(name)
    ql.assert_same_tree((nodes, idx), ql.ref_flat(reference, ql.scene(name)), name)
    assert st["n_refs"] == idx.size and st["n_failed_partitions"] == 0


def test_the_threaded_reference_build_gives_the_same_bytes(reference):
    nodes, idx, _ = twin("STREETROT262K")
    ql.assert_same_tree((nodes, idx), ql.ref_flat(reference, ql.scene("STREETROT262K"), threaded=True), "STREETROT262K, threaded reference")


@pytest.mark.parametrize("name", sorted(ql.REFERENCE_SIZES))
def test_sizes_are_the_ones_measured_on_the_reference(name):
    nodes, idx, st = twin(name)
    assert (nodes.shape[0], idx.size) == ql.REFERENCE_SIZES[name]
    assert ql.used_refs(nodes) == idx.size == st["n_refs"]
    assert st["n_failed_partitions"] == 0, "byte equality with the reference is not promised for this tree"


def test_every_path_of_the_builder_is_taken():
    """coverage is a condition: over the three scenes every counter but the two rare ones is above zero; the one-sided cut happens on STREETROT262K"""
    total = {k: sum(twin(n)[2][k] for n in COVERAGE) for k in tb.SBVH_STATS}
    for k in tb.SBVH_STATS:
        if k not in ("n_one_sided_splits", "n_failed_partitions"):
            assert total[k] > 0, (k, total)
    assert total["n_failed_partitions"] == 0
    assert twin("STREETROT262K")[2]["n_one_sided_splits"] >= 1
    # the counts an instrumented build of the reference gave for LONG2000
    st = twin("LONG2000")[2]
    assert (st["n_spatial_splits"], st["n_unsplit_left"], st["n_unsplit_right"], st["n_fragment_splits"], st["n_budget_refusals"], st["n_clipped_reclips"]) == \
        (33, 37, 21, 459, 258, 46)
    # a triangle that was cut is named by more than one leaf
    assert np.bincount(twin("LONG2000")[1]).max() > 1


def test_a_failed_partition_is_counted_and_leaves_a_valid_tree():
    """the one path on which the reference cannot be followed (it reads stale index entries there): the node becomes a leaf, the count says so"""
    nodes, idx, st = twin("HUGE300")
    assert st["n_failed_partitions"] >= 1
    assert np.array_equal(np.sort(idx), np.arange(300, dtype=np.uint32)) and ql.used_refs(nodes) == idx.size


def test_indexed_and_strided_forms_give_the_flat_form_s_bytes():
    pos, ind = mesh_lib.bunny()
    flat = mesh_lib.flatten(pos, ind)
    a = tb.host_build_bvh2_sbvh(flat)
    ql.assert_same_tree(tb.host_build_bvh2_sbvh(pos, indices=ind), a, "bunny, indexed")
    wide = np.zeros((pos.shape[0], 7), np.float32)   # a 28-byte stride: x y z and four floats of something else
    wide[:, :3] = pos[:, :3]; wide[:, 3:] = 7.0
    ql.assert_same_tree(tb.host_build_bvh2_sbvh(wide[:, :3], indices=ind), a, "bunny, 28-byte stride")
    v = ql.scene("LONG300")
    packed = np.ascontiguousarray(v[:, :3])   # 12-byte stride, no indices
    ql.assert_same_tree(tb.host_build_bvh2_sbvh(packed), twin("LONG300")[:2], "LONG300, 12-byte stride")


def test_indexed_form_is_the_reference_s(sbvh_ref_indexed):
    pos, ind = mesh_lib.bunny()
    ql.assert_same_tree(tb.host_build_bvh2_sbvh(pos, indices=ind), sbvh_ref_indexed.build(pos, ind), "bunny, indexed")
    # long thin triangles through an index buffer (shared vertices would not straddle much): LONG300 indexed in reverse vertex order per triangle
    v = ql.scene("LONG300")
    ind2 = np.arange(v.shape[0], dtype=np.uint32).reshape(-1, 3)[:, ::-1].copy()
    ql.assert_same_tree(tb.host_build_bvh2_sbvh(v, indices=ind2), sbvh_ref_indexed.build(v, ind2), "LONG300, indexed")


def leaves(nodes):
    """the leaves reachable from the root"""
    out, stack = [], [0]
    while stack:
        i = stack.pop()
        if nodes[i, 7]:
            out.append(i)
        else:
            stack += [int(nodes[i, 3]), int(nodes[i, 3]) + 1]
    return out


@pytest.mark.parametrize("k", [1, 3, 4])
@pytest.mark.parametrize("name", ["S", "POINT", "LONG2000", "ATRIUMROT30K"])
def test_max_leaf_tris(name, k):
    n0, i0, _ = twin(name)
    nodes, idx = tb.host_build_bvh2_sbvh(ql.scene(name), max_leaf_tris=k)
    f = nodes.view(np.float32)
    n = n0.shape[0]
    assert np.array_equal(idx, i0), "the leaf splitting moved references"
    grew = n0[:, 7] > k
    assert np.array_equal(nodes[:n][~grew], n0[~grew]), "a node the splitting did not touch changed"
    assert np.array_equal(nodes[:n][grew][:, [0, 1, 2, 4, 5, 6]], n0[grew][:, [0, 1, 2, 4, 5, 6]]), "a split leaf's box changed"
    assert (nodes[:n][grew][:, 7] == 0).all() and (nodes[:n][grew][:, 3] >= n).all()
    assert nodes[:, 7].max() <= k, "a leaf above k"
    # every new leaf lies in one old leaf's range and box; together the new leaves of an old leaf are that leaf
    covered = np.zeros(idx.size, np.int32)
    for i in leaves(nodes):
        covered[int(nodes[i, 3]):int(nodes[i, 3]) + int(nodes[i, 7])] += 1
    assert (covered == 1).all(), "the leaves do not tile primIdx"
    for i in np.nonzero(grew)[0]:
        lo, hi = int(n0[i, 3]), int(n0[i, 3]) + int(n0[i, 7])
        box_mn, box_mx = n0.view(np.float32)[i, 0:3], n0.view(np.float32)[i, 4:7]
        stack, at = [int(nodes[i, 3]), int(nodes[i, 3]) + 1], lo
        while stack:
            c = stack.pop()
            assert c >= n, "a chain leaves the new nodes"
            assert (f[c, 0:3] >= box_mn).all() and (f[c, 4:7] <= box_mx).all(), f"new node {c} grows out of leaf {i}'s box"
            if nodes[c, 7]:
                assert lo <= nodes[c, 3] and nodes[c, 3] + nodes[c, 7] <= hi
            else:
                stack += [int(nodes[c, 3]), int(nodes[c, 3]) + 1]


@pytest.mark.parametrize("name", ql.GOLDEN_SCENES)
def test_fixtures_are_the_reference_s(reference, name):
    nodes, idx = ql.ref_flat(reference, ql.scene(name))
    ql.assert_matches_golden(name, nodes, idx, "reference")


@pytest.mark.parametrize("name", ql.GOLDEN_SCENES)
def test_host_twin_matches_the_fixtures(name):
    nodes, idx, _ = twin(name)
    ql.assert_matches_golden(name, nodes, idx, "host twin")
    g_nodes = ql.load_golden(name)[0]
    assert (g_nodes is not None) == (name in ql.GOLDEN_FULL)


def test_errors():
    v = ql.scene("SOUP9")
    m, keep = tb._mesh(v)
    n, k = C.c_uint64(0), C.c_uint64(0)
    lib = tb.lib
    assert lib.tbvh_host_build_bvh2_sbvh(None, 0, None, 0, None, 0, C.byref(n), C.byref(k), None) == -1
    assert lib.tbvh_host_build_bvh2_sbvh(C.byref(m), 0, None, 0, None, 0, None, C.byref(k), None) == -1
    assert lib.tbvh_host_build_bvh2_sbvh(C.byref(m), 0, None, 0, None, 0, C.byref(n), None, None) == -1
    assert lib.tbvh_host_build_bvh2_sbvh(C.byref(m), 0, None, 0, None, 0, C.byref(n), C.byref(k), None) == 0
    want = tb.host_build_bvh2_sbvh(v)
    assert (n.value, k.value) == (want[0].shape[0], want[1].size)
    nodes = np.zeros((2, 8), np.uint32); idx = np.zeros(9, np.uint32)
    need = n.value
    n.value = 0
    assert lib.tbvh_host_build_bvh2_sbvh(C.byref(m), 0, nodes.ctypes.data, 2, idx.ctypes.data, 9, C.byref(n), C.byref(k), None) == -1 and n.value == need
    assert not nodes.any()
    bad = np.array([0, 1, 99], np.uint32)
    mb, keep2 = tb._mesh(v, bad)
    assert lib.tbvh_host_build_bvh2_sbvh(C.byref(mb), 0, None, 0, None, 0, C.byref(n), C.byref(k), None) == -5   # TBVH_E_FORMAT: host indices are checked first
