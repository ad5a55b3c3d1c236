"""Sphere-overlap queries on the CPU: the restatement (tests/oracle_sphere.c) pinned to the real BVH::IntersectSphere, and the restatements of
the three GPU layouts checked against the Wald walk (DESIGN.md par. 11).  The GPU side is tests/test_sphere_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import tinybvh_amd as tb
from tinybvh_amd import _capi
from sphere_lib import MESHES, box_faces, in_rounding_class, mesh, sph_oracle, sph_ref, sphere_sets, zero_area_yes  # noqa: F401 (fixtures)


def test_sphere_symbols_are_exported_and_bound():
    raw = C.CDLL(_capi.LIB_PATH)
    for s in ("tbvh_intersect_spheres", "tbvh_intersect_spheres_device"):
        assert hasattr(raw, s), f"{s} not exported"
        assert s in _capi.SYMBOLS
    for cls in (tb.BVH_GPU, tb.BVH4_GPU, tb.BVH8_CWBVH):
        for m in ("intersect_spheres", "intersect_spheres_device", "intersect_sphere"):
            assert callable(getattr(cls, m, None)), f"{cls.__name__}.{m}"


def test_refusals_need_no_device():
    lib = _capi.lib
    s = np.zeros((1, 4), np.float32)
    v = np.zeros((3, 4), np.float32)
    hit = np.zeros(1, np.uint8)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    assert lib.tbvh_intersect_spheres(None, p(s), 1, p(v), 1, p(hit)) == -1
    assert b"null scene" in lib.tbvh_last_error()
    assert lib.tbvh_intersect_spheres_device(None, p(s), 1, p(v), 1, p(hit)) == -1


def geometric(sp):
    """spheres whose answer is a property of the geometry: r >= 0 and components whose squares and products stay finite in float"""
    return (np.abs(sp) < 1e15).all(1) & (sp[:, 3] >= 0)


def _reference_case(sph_oracle, sph_ref, name, hq):
    verts = mesh(name)
    h = sph_ref.build(verts, hq)
    n32, pi = sph_ref.blob(h, 0), sph_ref.blob(h, 1)
    sets = sphere_sets(verts, n32, seed=100 + 7 * MESHES.index(name) + hq)
    return verts, h, n32, pi, sets


@pytest.mark.parametrize("name", MESHES)
@pytest.mark.parametrize("hq", [False, True])
def test_restatement_equals_the_reference(sph_oracle, sph_ref, name, hq):
    """(a): the restated arithmetic equals the real reference on every sphere (its root made one leaf), and the restated walk verbatim equals
    BVH::IntersectSphere on every sphere whose reference walk stays defined; the library's walk equals it wherever that walk took no leaf
    off the stack (defect 1)"""
    verts, h, n32, pi, sets = _reference_case(sph_oracle, sph_ref, name, hq)
    try:
        f = np.ascontiguousarray(n32).view(np.float32)
        root = np.concatenate([f[0, 0:3], f[0, 4:7]])
        tot = {"spheres": 0, "undefined": 0, "popped_leaf": 0, "differ": 0}
        for kind, sp in sets.items():
            np.testing.assert_array_equal(sph_oracle.flat(root, pi, verts, sp), sph_ref.intersect_flat(h, sp), err_msg=f"{kind}: triangle test")
            verb = sph_oracle.wald(n32, pi, verts, sp, mode=0)
            ok = verb != 2
            ref = sph_ref.intersect(h, sp[ok])
            np.testing.assert_array_equal(verb[ok] & 1, ref, err_msg=f"{kind}: verbatim walk")
            lib = sph_oracle.wald(n32, pi, verts, sp, mode=1)
            same = ok & ((verb & 4) == 0)
            np.testing.assert_array_equal(lib[same], (verb & 1)[same], err_msg=f"{kind}: library walk where no leaf was popped")
            assert (lib[ok & ~same] >= (verb & 1)[ok & ~same]).all(), "the library's walk only ADDS the leaves the reference skips"
            tot["spheres"] += sp.shape[0]; tot["undefined"] += int((~ok).sum()); tot["popped_leaf"] += int((~same & ok).sum())
            tot["differ"] += int((lib[ok] != (verb & 1)[ok]).sum())
        print(f"{name} hq={hq}: {tot}")
    finally:
        sph_ref.free(h)


@pytest.mark.parametrize("name", MESHES)
@pytest.mark.parametrize("hq", [False, True])
def test_layout_restatements_against_the_wald_walk(sph_oracle, sph_ref, name, hq):
    """(b) BVH_GPU equals (a) on every sphere; (c) BVH4_GPU and (d) BVH8_CWBVH differ from (a) only in the rounding class (r >= 0), or
    where the reference's own test answers yes for a zero-area triangle that one tree's leaf boxes reach and the other's do not"""
    verts, h, n32, pi, sets = _reference_case(sph_oracle, sph_ref, name, hq)
    try:
        wald_faces = box_faces(1, [n32])
        blobs = {8: [sph_ref.blob(h, 3)], 10: [sph_ref.blob(h, 4), sph_ref.blob(h, 5)]}
        faces = {k: box_faces(k, b) for k, b in blobs.items()}
        counts = {8: [0, 0], 10: [0, 0]}
        for kind, sp in sets.items():
            a = sph_oracle.wald(n32, pi, verts, sp, mode=1)
            np.testing.assert_array_equal(sph_oracle.bvhgpu(sph_ref.blob(h, 2), pi, verts, sp), a, err_msg=f"{kind}: BVH_GPU")
            for lay in (8, 10):
                got = sph_oracle.layout(lay, blobs[lay], verts, sp)
                # r < 0 inverts the sphere's box, a non-finite component fails every box test, huge ones overflow: the answer then depends on the trees'
                # node sizes and on whether the root is a leaf (never box-tested), not on the geometry; the device matches each layout's
                # restatement on those too (test_sphere_gpu.py)
                diff = np.flatnonzero((got != a) & geometric(sp))
                cls = in_rounding_class(sp[diff], verts, [wald_faces, faces[lay]])
                deg = zero_area_yes(sph_oracle, sp[diff], verts) & ~cls
                assert (cls | deg).all(), f"{kind} layout {lay}: spheres outside the rounding class differ: {sp[diff][~(cls | deg)][:5]}"
                counts[lay][0] += int(cls.sum()); counts[lay][1] += int(deg.sum())
        print(f"{name} hq={hq}: differences from the Wald walk (rounding class, zero-area triangle) BVH4_GPU {counts[8]}, BVH8_CWBVH {counts[10]}")
    finally:
        sph_ref.free(h)


@pytest.mark.parametrize("layout", [tb.LAYOUT_BVH_GPU, tb.LAYOUT_BVH4_GPU, tb.LAYOUT_CWBVH])
def test_host_built_layouts_against_their_wald_tree(sph_oracle, layout):
    """the library's own host builds: each layout's restatement against the Wald walk over the BVH2 it was encoded from"""
    verts = mesh("atrium")
    hb = tb.HostBVH(verts, layout)
    n32, pi = hb.bvh2_nodes(), hb.bvh2_prim_idx()
    sets = sphere_sets(verts, n32, seed=31)
    if layout == tb.LAYOUT_BVH_GPU:
        blobs = [hb.blob(0, np.uint32, 16), hb.blob(1, np.uint32, 1).reshape(-1)]
    elif layout == tb.LAYOUT_BVH4_GPU:
        blobs = [hb.blob(0, np.uint32, 4)]
    else:
        blobs = [hb.blob(0, np.uint32, 4), hb.blob(1, np.uint32, 4)]
    faces = [box_faces(1, [n32]), box_faces(layout, blobs)]
    for kind, sp in sets.items():
        a = sph_oracle.wald(n32, pi, verts, sp, mode=1)
        got = sph_oracle.layout(layout, blobs, verts, sp)
        if layout == tb.LAYOUT_BVH_GPU:
            np.testing.assert_array_equal(got, a, err_msg=kind)
        else:
            diff = np.flatnonzero((got != a) & geometric(sp))
            assert (in_rounding_class(sp[diff], verts, faces) | zero_area_yes(sph_oracle, sp[diff], verts)).all(), kind
