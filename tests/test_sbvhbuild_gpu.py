"""The device SBVH builder (tbvh_build_bvh2_sbvh_device, tbvh_build_device_sbvh, tbvh_build_device_sbvh_mesh; csrc/kernels_sbvhbuild.hip) against its
sequential CPU twin over the same csrc/sbvh_split.h and against the recorded reference trees of tests/golden/sbvhbuild: byte for byte, statistics
included.  The twin itself is held to the real reference's BVH::BuildHQ in tests/test_sbvhbuild_host.py (DESIGN.md par. 19).
(The builder has no small-subtree path, so there is no second path to force.)"""
import ctypes as C

import numpy as np
import pytest

import tinybvh_amd as tb
import mesh_lib
import sahbuild_lib as sl
import sbvhbuild_lib as ql
import tree_check as tc
from test_sahbuild_gpu import camera_rays, check_hits

pytestmark = pytest.mark.gpu
lib = tb.lib
CW, B4 = tb.LAYOUT_CWBVH, tb.LAYOUT_BVH4_GPU
BIG = ["S", "FAR", "FLAT", "POINT", "TWO", "QUADS", "LATTICE", "LONG300", "LONG2000", "LONGFLAT", "ATRIUMROT30K", "STREET45K"]
_twin = {}


def twin(name, k=0):
    """the host twin's tree and statistics of a scene, built once"""
    if (name, k) not in _twin:
        _twin[(name, k)] = tb.host_build_bvh2_sbvh(ql.scene(name), max_leaf_tris=k, stats=True)
    return _twin[(name, k)]


@pytest.mark.parametrize("name", ql.SOUPS + BIG)
def test_device_tree_is_the_host_twin_s(ctx, name):
    nodes, idx, st = tb.build_bvh2_sbvh(ctx, ql.scene(name), stats=True)
    want = twin(name)
    ql.assert_same_tree((nodes, idx), want, name)
    assert st == want[2], f"{name}: the device counts {st}, the twin {want[2]}"
    assert st["n_failed_partitions"] == 0
    assert ctx.time_last_ms() > 0


def test_a_failed_partition_is_the_host_twin_s_too(ctx):
    """HUGE300 takes the path the reference cannot be followed on (no byte equality with the reference is promised there): the device still equals the twin"""
    nodes, idx, st = tb.build_bvh2_sbvh(ctx, ql.scene("HUGE300"), stats=True)
    want = twin("HUGE300")
    ql.assert_same_tree((nodes, idx), want, "HUGE300")
    assert st == want[2] and st["n_failed_partitions"] >= 1


@pytest.mark.parametrize("k", [1, 3, 4])
@pytest.mark.parametrize("name", ["SOUP9", "S", "POINT", "LONG2000", "ATRIUMROT30K"])
def test_max_leaf_tris_is_the_host_twin_s(ctx, name, k):
    ql.assert_same_tree(tb.build_bvh2_sbvh(ctx, ql.scene(name), max_leaf_tris=k), twin(name, k), f"{name}, max_leaf_tris = {k}")


@pytest.mark.parametrize("name", ql.GOLDEN_SCENES)
def test_device_tree_is_the_recorded_reference_tree(ctx, name):
    nodes, idx = tb.build_bvh2_sbvh(ctx, ql.scene(name))
    ql.assert_matches_golden(name, nodes, idx, "device")


@pytest.mark.parametrize("name", ["LONG2000", "ATRIUMROT30K"])
def test_two_builds_give_identical_trees(ctx, name):
    """fragment indices are handed out by an atomic counter: they must not reach the output"""
    verts = ql.scene(name)
    one, two = tb.build_bvh2_sbvh(ctx, verts, stats=True), tb.build_bvh2_sbvh(ctx, verts, stats=True)
    ql.assert_same_tree(one, two, name + ", second build")
    assert one[2] == two[2] and one[2]["n_fragment_splits"] > 0


def assert_sbvh_blob(layout, nodes, tris, verts, refs, label):
    """tree_check.assert_tree's conditions, except the three that hold a box to be NO SMALLER than the bounds of the whole triangles beneath it,
    which the clipped leaves of an SBVH are on purpose (tests/test_tree_check_host.py: test_golden_reference_blobs_walk only counts them for the
    reference's own BuildHQ blobs): `containment` (a plane inside a triangle's bounds), `inexact` (a stored origin or box that is not exactly those
    bounds) and `short_reach` (255 steps end before the far face of those bounds).  Everything that holds a box to be no LARGER stays: slack,
    exponent and step.  The references reached are exactly the twin's, and every triangle record is its triangle."""
    F = tc.check_tree(layout, nodes, tris, verts)
    assert not F["bad_index"] and not F["multi_reached"], (label, F["bad_index"][:2], F["multi_reached"][:4])
    assert np.array_equal(np.sort(F["prims"]), np.sort(refs)), f"{label}: the references reached are not the twin's"
    assert np.array_equal(np.unique(F["prims"]), np.arange(verts.shape[0] // 3, dtype=np.uint32)), f"{label}: a triangle is in no leaf"
    assert not F["record_mismatch"], (label, F["record_mismatch"][:2])
    assert not F["exponent_over"] and not F["step_over"] and not F["slack_over"], (label, F["exponent_over"][:2], F["step_over"][:2], F["slack_over"][:2])


@pytest.mark.parametrize("layout", [CW, B4])
@pytest.mark.parametrize("name", ["S", "LONG2000", "POINT", "ATRIUMROT30K"])
def test_wide_layouts(ctx, oracle, layout, name):
    verts = ql.scene(name)
    cls = tb.LAYOUT_CLASSES[layout]
    k = 3 if layout == CW else 4
    sc = cls(ctx).BuildOnDevice(verts, builder="sbvh", max_leaf_tris=k)
    nodes, tris = sc.download_blobs()
    n2, pi, _ = twin(name, k)
    assert_sbvh_blob(layout, nodes, None if layout == B4 else tris, verts, pi, f"{name} built by the device SBVH builder")
    # the blob is the conversion of the host twin's tree (sahbuild_lib.assert_same_blobs: the same bytes, or the same nodes in another order)
    ref = cls(ctx).ConvertFromBVH2(n2, pi, verts); ref2 = cls(ctx).ConvertFromBVH2(n2, pi, verts)
    sl.assert_same_blobs(layout == CW, ref.download_blobs(), ref2.download_blobs(), (nodes, tris), name)
    # max_leaf_tris = 0 means the most the layout's leaves hold
    dflt = cls(ctx).BuildOnDevice(verts, builder="sbvh", max_leaf_tris=0)
    sl.assert_same_blobs(layout == CW, ref.download_blobs(), ref2.download_blobs(), dflt.download_blobs(), name + ", max_leaf_tris = 0")
    rays = camera_rays(verts)
    t0, i0, _ = twin(name, 0)
    want = oracle.bvh2_intersect(t0, i0, verts, rays)
    c = check_hits(sc.Intersect(rays.copy()), want)
    assert c["hits"] > 500, c
    for s in (sc, ref, ref2, dflt):
        s.free()


@pytest.mark.parametrize("layout", [CW, B4])
def test_indexed_form_equals_flat(ctx, layout):
    pos, idx = mesh_lib.bunny()
    flat = mesh_lib.flatten(pos, idx)
    cls = tb.LAYOUT_CLASSES[layout]
    a = cls(ctx).BuildOnDevice(flat, builder="sbvh"); a2 = cls(ctx).BuildOnDevice(flat, builder="sbvh")
    b = cls(ctx).BuildOnDevice(pos, builder="sbvh", indices=idx)
    sl.assert_same_blobs(layout == CW, a.download_blobs(), a2.download_blobs(), b.download_blobs(), "bunny, indexed")
    assert b.device_bytes == a.device_bytes + 12 * idx.shape[0], "the scene keeps its index buffer (and nothing else)"
    ql.assert_same_tree(tb.build_bvh2_sbvh(ctx, pos, indices=idx), tb.host_build_bvh2_sbvh(flat), "bunny, indexed")
    # long thin triangles through an index buffer, and through a 12-byte stride
    v = ql.scene("LONG300")
    ind2 = np.arange(v.shape[0], dtype=np.uint32).reshape(-1, 3)
    ql.assert_same_tree(tb.build_bvh2_sbvh(ctx, v, indices=ind2), twin("LONG300"), "LONG300, indexed")
    ql.assert_same_tree(tb.build_bvh2_sbvh(ctx, np.ascontiguousarray(v[:, :3])), twin("LONG300"), "LONG300, 12-byte stride")
    a.free(); a2.free(); b.free()


def test_everything_on_the_device(ctx):
    """vertices given as a device pointer, the BVH2 left on the device and handed to tbvh_convert_bvh2_device( on_device = 1 )"""
    verts = ql.scene("LONG2000")
    n = verts.shape[0] // 3
    cap_n, cap_i = 3 * n, n + n // 2
    d_v = ctx.malloc(verts.nbytes); ctx.to_device(d_v, verts)
    d_n = ctx.malloc(cap_n * 32); d_i = ctx.malloc(cap_i * 4)
    m = tb.device_mesh(d_v, verts.shape[0], n)
    nn, ni = C.c_uint64(0), C.c_uint64(0)
    tb.check(lib.tbvh_build_bvh2_sbvh_device(ctx._h, C.byref(m), 3, C.c_void_p(d_n), cap_n, C.c_void_p(d_i), cap_i, 1, C.byref(nn), C.byref(ni), None),
             "tbvh_build_bvh2_sbvh_device")
    want = twin("LONG2000", 3)
    assert (nn.value, ni.value) == (want[0].shape[0], want[1].size)
    nodes = np.zeros((nn.value, 8), np.uint32); idx = np.zeros(ni.value, np.uint32)
    ctx.from_device(nodes, d_n); ctx.from_device(idx, d_i)
    ql.assert_same_tree((nodes, idx), want, "LONG2000, device in and out")
    sc = tb.BVH8_CWBVH(ctx)
    tb.check(lib.tbvh_convert_bvh2_device(ctx._h, C.c_void_p(d_n), nn.value, C.c_void_p(d_i), ni.value, C.c_void_p(d_v), n, 1, CW, C.byref(sc._h)), "tbvh_convert_bvh2_device")
    ref = tb.BVH8_CWBVH(ctx).ConvertFromBVH2(want[0], want[1], verts); ref2 = tb.BVH8_CWBVH(ctx).ConvertFromBVH2(want[0], want[1], verts)
    dev = tb.BVH8_CWBVH(ctx)
    tb.check(lib.tbvh_build_device_sbvh(ctx._h, C.c_void_p(d_v), n, 1, CW, 3, C.byref(dev._h)), "tbvh_build_device_sbvh")
    for x in (sc, dev):
        sl.assert_same_blobs(True, ref.download_blobs(), ref2.download_blobs(), x.download_blobs(), "LONG2000, everything on the device")
    for s in (sc, ref, ref2, dev):
        s.free()
    for d in (d_v, d_n, d_i):
        ctx.free(d)


def test_errors_leave_the_context_usable(ctx):
    verts = ql.scene("SOUP65")
    n = verts.shape[0] // 3
    m, keep = tb._mesh(verts)
    nn, ni = C.c_uint64(0), C.c_uint64(0)
    out = C.c_void_p()
    INVALID, FORMAT = -1, -5
    empty = tb.Mesh(C.c_void_p(verts.ctypes.data), verts.shape[0], 16, 0, None, 0)
    assert lib.tbvh_build_bvh2_sbvh_device(ctx._h, C.byref(empty), 0, None, 0, None, 0, 0, C.byref(nn), C.byref(ni), None) == INVALID
    assert lib.tbvh_build_bvh2_sbvh_device(ctx._h, None, 0, None, 0, None, 0, 0, C.byref(nn), C.byref(ni), None) == INVALID
    assert lib.tbvh_build_bvh2_sbvh_device(ctx._h, C.byref(m), 0, None, 0, None, 0, 0, None, C.byref(ni), None) == INVALID
    assert lib.tbvh_build_bvh2_sbvh_device(ctx._h, C.byref(m), 0, None, 0, None, 0, 0, C.byref(nn), None, None) == INVALID
    assert lib.tbvh_build_device_sbvh(ctx._h, C.c_void_p(verts.ctypes.data), 0, 0, CW, 0, C.byref(out)) == INVALID
    assert lib.tbvh_build_device_sbvh(ctx._h, C.c_void_p(verts.ctypes.data), n, 0, tb.LAYOUT_BVH_GPU, 0, C.byref(out)) == INVALID
    assert lib.tbvh_build_device_sbvh(ctx._h, C.c_void_p(verts.ctypes.data), n, 0, CW, 4, C.byref(out)) == INVALID
    assert lib.tbvh_build_device_sbvh(ctx._h, C.c_void_p(verts.ctypes.data), n, 0, B4, 5, C.byref(out)) == INVALID
    assert lib.tbvh_build_device_sbvh_mesh(ctx._h, C.byref(m), CW, 4, C.byref(out)) == INVALID
    assert lib.tbvh_build_device_sbvh_mesh(ctx._h, None, CW, 0, C.byref(out)) == INVALID
    assert lib.tbvh_build_device_mesh(ctx._h, C.byref(m), CW, 0, 3, 0, C.byref(out)) == INVALID   # (builder 3 stays invalid: the SBVH has entry points of its own)
    # the counts alone, then a capacity that is too small: the needs are reported, nothing is written
    assert lib.tbvh_build_bvh2_sbvh_device(ctx._h, C.byref(m), 0, None, 0, None, 0, 0, C.byref(nn), C.byref(ni), None) == 0
    need, need_i = nn.value, ni.value
    assert (need, need_i) == (twin("SOUP65")[0].shape[0], twin("SOUP65")[1].size)
    nodes = np.zeros((need - 1, 8), np.uint32); idx = np.zeros(n + n // 2, np.uint32)
    nn.value = 0
    assert lib.tbvh_build_bvh2_sbvh_device(ctx._h, C.byref(m), 0, nodes.ctypes.data, need - 1, idx.ctypes.data, idx.size, 0, C.byref(nn), C.byref(ni), None) == INVALID
    assert nn.value == need and not nodes.any()
    nodes = np.zeros((need, 8), np.uint32)
    assert lib.tbvh_build_bvh2_sbvh_device(ctx._h, C.byref(m), 0, nodes.ctypes.data, need, idx.ctypes.data, need_i - 1, 0, C.byref(nn), C.byref(ni), None) == INVALID
    assert ni.value == need_i and not nodes.any() and not idx.any()
    # a device-resident index beyond n_verts (but inside the allocation): reported, never dereferenced (as tests/test_mesh_gpu.py)
    pos, ind = mesh_lib.bunny()
    padded = np.concatenate([pos, np.zeros((64, 4), np.float32)])
    bad = ind.copy(); bad[123, 1] = pos.shape[0] + 5
    d_v = ctx.malloc(padded.nbytes); ctx.to_device(d_v, padded)
    d_i = ctx.malloc(bad.nbytes); ctx.to_device(d_i, bad)
    dm = tb.device_mesh(d_v, pos.shape[0], ind.shape[0], d_i)
    assert lib.tbvh_build_bvh2_sbvh_device(ctx._h, C.byref(dm), 0, None, 0, None, 0, 0, C.byref(nn), C.byref(ni), None) == FORMAT
    assert lib.tbvh_build_device_sbvh_mesh(ctx._h, C.byref(dm), CW, 0, C.byref(out)) == FORMAT
    with pytest.raises(tb.TbvhError, match="triangle 123"):
        tb.build_bvh2_sbvh(ctx, pos, indices=bad)
    ctx.free(d_v); ctx.free(d_i)
    # the context works on
    ql.assert_same_tree(tb.build_bvh2_sbvh(ctx, verts), twin("SOUP65"), "after the errors")
