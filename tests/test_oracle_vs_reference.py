"""Pins the C restatement (oracle/tbvh_oracle.c) against the REAL reference
(oracle/_ref/libtinybvh_ref.so, built from tiny_bvh.h where the checkout exists): on the
reference's own trees and blobs the restated traversals reproduce BVH::Intersect /
IsOccluded and the three layout mirrors bit for bit."""
import os

import numpy as np
import pytest

import tinybvh_amd as tb
from tinybvh_amd import rays as R
from tinybvh_amd import scenes
from oracle_lib import compare_hits


def batches(verts):
    lo, hi = verts[:, :3].min(0), verts[:, :3].max(0)
    c = (lo + hi) / 2; ext = float((hi - lo).max())
    cam = R.camera(c + np.array([0.1 * ext, 0.2 * ext, 1.4 * ext], np.float32), (-0.05, -0.12, -1.0), 96, 96, 1, 1)
    prim = R.primary(cam)
    rnd = R.random_rays(12_000, lo - 0.1 * ext, hi + 0.1 * ext, seed=5)
    return prim, rnd


def exact(got, want):
    for f in ("t", "u", "v", "prim", "inst"):
        assert np.array_equal(got[f].view(np.uint32), want[f].view(np.uint32)), f


SCENES = ["soup", "atrium", "bunny"]


def get_scene(name):
    if name == "soup":
        return scenes.soup(8192, seed=7)
    if name == "atrium":
        return scenes.atrium(25_000, seed=1)
    # the reference's testdata/bunny.bin, stored bit for bit as its distinct vertices, three indices per triangle and the common w
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "meshes", "bunny.npz"))
    verts = np.empty((g["indices"].size, 4), np.float32)
    verts[:, :3] = g["positions"][g["indices"].ravel()]
    verts[:, 3] = g["w_bits"].view(np.float32)[0]
    return verts


@pytest.mark.parametrize("scene", SCENES)
@pytest.mark.parametrize("hq", [False, True])
def test_restated_traversals_equal_the_reference(oracle_ref, reference, scene, hq):
    verts = get_scene(scene)
    rs = reference.build(verts, hq=hq)
    n2, pi = rs.blob(1, 0, np.uint32, 8), rs.blob(1, 1, np.uint32, 1)
    for rays in batches(verts):
        want = rs.intersect(1, rays)
        assert (want["t"] < 1e30).sum() > 100
        exact(oracle_ref.bvh2_intersect(n2, pi, verts, rays), want)                       # BVH::Intersect
        exact(oracle_ref.bvhgpu_intersect(rs.blob(5, 0, np.uint32, 16), rs.blob(5, 1, np.uint32, 1), verts, rays), rs.intersect(5, rays))
        exact(oracle_ref.bvh4_intersect(rs.blob(8, 0, np.uint32, 4), rays), rs.intersect(8, rays))
        # the CWBVH mirror zeroes u,v,prim of missed finite-tmax rays (tiny_bvh.h:7148); tmax is
        # 1e30 here so records are comparable field by field
        got = oracle_ref.cwbvh_intersect(rs.blob(10, 0, np.uint32, 4), rs.blob(10, 1, np.uint32, 4), rays)
        ref9 = rs.intersect(10, rays)
        for f in ("t", "u", "v", "prim"):
            assert np.array_equal(got[f].view(np.uint32), ref9[f].view(np.uint32)), f
        # shadow rays
        sh = R.shadow(want, verts[:, :3].max(0) * 1.1, 1e-4)
        assert np.array_equal(oracle_ref.bvh2_occluded(n2, pi, verts, sh), rs.occluded(1, sh))


def test_own_builder_gives_the_reference_hits(oracle_ref, reference):
    """Hit records are builder independent (up to ties): the library's own BVH and the
    reference's BVH::Build agree ray by ray."""
    verts = scenes.atrium(25_000, seed=1)
    rs = reference.build(verts)
    h = tb.HostBVH(verts, tb.LAYOUT_BVH2_WALD)
    for rays in batches(verts):
        got = oracle_ref.bvh2_intersect(h.bvh2_nodes(), h.bvh2_prim_idx(), verts, rays)
        c = compare_hits(got, rs.intersect(1, rays))
        assert c["hitmiss"] == 0 and c["prim_real"] == 0 and c["t_bad"] == 0 and c["tie"] <= 2, c
        assert c["bit_identical"] == c["same_prim"], c


def test_reference_counts_match_oracle_counts(oracle_ref, reference):
    verts = scenes.atrium(25_000, seed=1)
    rs = reference.build(verts)
    rays = batches(verts)[0]
    for layout, fn in ((1, lambda: oracle_ref.bvh2_intersect(rs.blob(1, 0, np.uint32, 8), rs.blob(1, 1, np.uint32, 1), verts, rays, counts=True)),
                       (5, lambda: oracle_ref.bvhgpu_intersect(rs.blob(5, 0, np.uint32, 16), rs.blob(5, 1, np.uint32, 1), verts, rays, counts=True)),
                       (8, lambda: oracle_ref.bvh4_intersect(rs.blob(8, 0, np.uint32, 4), rays, counts=True))):
        s, t = rs.counts(layout, rays)
        _, c = fn()
        assert (int(c[0]), int(c[1])) == (s, t), layout


def _random_instances(n, seed, projective_every=0):
    rng = np.random.default_rng(seed)
    T = np.zeros((n, 4, 4), np.float32)
    for i in range(n):
        a, b, c = rng.random(3) * 6.28
        ca, sa, cb, sb, cc, sc = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(c), np.sin(c)
        Rm = np.array([[cb * cc, -cb * sc, sb], [sa * sb * cc + ca * sc, -sa * sb * sc + ca * cc, -sa * cb], [-ca * sb * cc + sa * sc, ca * sb * sc + sa * cc, ca * cb]])
        T[i, :3, :3] = Rm @ np.diag(0.3 + rng.random(3)); T[i, :3, 3] = rng.normal(0, 4, 3); T[i, 3, 3] = 1
        if projective_every and i % projective_every == 0:
            T[i, 3, :3] = rng.normal(0, 0.02, 3); T[i, 3, 3] = 1 + rng.normal(0, 0.05)
    return tb.make_instances(T, (np.arange(n) % 2).astype(np.uint32))


def test_instance_update_is_bit_identical_to_the_reference(reference):
    """BLASInstance::Update (inverse + world box) restated in host_builder.cpp (and run unchanged on the device by
    tbvh_rebuild_tlas_device) against the real thing, affine and projective transforms."""
    import ctypes as C
    v0, v1 = scenes.blob(1500, seed=3), scenes.soup(800, seed=2)
    r0, r1 = reference.build(v0, hq=False, threaded=False), reference.build(v1, hq=False, threaded=False)
    inst = _random_instances(600, seed=11, projective_every=5)
    mine, theirs = inst.copy(), inst.copy()
    bounds = np.stack([np.concatenate([v[:, :3].min(0), v[:, :3].max(0)]) for v in (v0, v1)]).astype(np.float32)
    h = C.c_void_p()
    tb.check(tb.lib.tbvh_host_build_tlas(C.c_void_p(mine.ctypes.data), mine.shape[0], C.c_void_p(bounds.ctypes.data), 2, C.byref(h)), "tbvh_host_build_tlas")
    tb.lib.tbvh_host_free(h)
    arr = (C.c_void_p * 2)(r0.h, r1.h)
    t = reference.lib.ref_tlas_build(C.c_void_p(theirs.ctypes.data), theirs.shape[0], arr, 2)
    reference.lib.ref_tlas_free(t)
    for f in ("invTransform", "aabbMin", "aabbMax"):
        assert np.array_equal(mine[f].view(np.uint32), theirs[f].view(np.uint32)), f


def test_restated_tlas_traversal_equals_the_reference(oracle_ref, reference):
    """BVH::IntersectTLAS restated (orc_tlas_intersect) on the reference's own TLAS and instance records."""
    import ctypes as C
    from oracle_lib import tlas_intersect
    v0, v1 = scenes.blob(3000, seed=3), scenes.soup(1500, seed=2, extent=1.6, size=0.25)
    r0, r1 = reference.build(v0, hq=False, threaded=False), reference.build(v1, hq=False, threaded=False)
    inst = _random_instances(64, seed=4)
    inst["transform"].reshape(-1, 4, 4)[:, :3, 3] *= 0.6
    arr = (C.c_void_p * 2)(r0.h, r1.h)
    t = reference.lib.ref_tlas_build(C.c_void_p(inst.ctypes.data), inst.shape[0], arr, 2)
    rays = R.random_rays(20_000, (-8, -8, -8), (8, 8, 8), seed=9)
    rays["inst"] = 0
    want = np.ascontiguousarray(rays).copy()
    reference.lib.ref_tlas_intersect(t, C.c_void_p(want.ctypes.data), want.shape[0], want.strides[0])
    p = C.c_void_p()
    nn = reference.lib.ref_tlas_blob(t, 2, C.byref(p)); nodes = np.frombuffer((C.c_char * (nn * 32)).from_address(p.value), np.uint32).reshape(-1, 8).copy()
    ni = reference.lib.ref_tlas_blob(t, 1, C.byref(p)); idx = np.frombuffer((C.c_char * (ni * 4)).from_address(p.value), np.uint32).copy()
    bl = [(r.blob(1, 0, np.uint32, 8), r.blob(1, 1, np.uint32, 1).reshape(-1), v) for r, v in ((r0, v0), (r1, v1))]
    got = tlas_intersect(oracle_ref, nodes, idx, inst, bl, rays)
    reference.lib.ref_tlas_free(t)
    assert int((want["t"] < 1e30).sum()) > 1000
    c = compare_hits(got, want)
    assert c["hitmiss"] == 0 and c["prim_real"] == 0 and c["t_bad"] == 0 and c["uv_bad"] == 0, c
    same = (want["t"] < 1e30) & (got["prim"] == want["prim"]) & (got["t"] == want["t"])
    print("TLAS hits", c["hits"], "bit-identical", c["bit_identical"], "same prim", c["same_prim"], "ties", c["tie"])
    assert np.array_equal(got["inst"][same], want["inst"][same])


def test_restated_tlas_traversal_equals_the_reference_on_hostile_instances(oracle_ref, reference):
    """orc_tlas_intersect against the real BVH::IntersectTLAS on the instance families and ray groups of tests/tlas_edges_lib.py (mirrored, exactly
    axis-aligned, strongly anisotropic, sheared and PROJECTIVE transforms: the oracle's w != 1 branch; duplicated and masked instances), with
    tmax = 1e30, a finite tmax and carried-in records.  This is what entitles tests/test_tlas_edges_gpu.py to take the oracle for the reference there."""
    import ctypes as C
    from oracle_lib import tlas_intersect
    import tlas_edges_lib as E
    vs = E.meshes()
    rs = [reference.build(v, hq=False, threaded=False) for v in vs]
    inst, names = E.families(len(vs))
    arr = (C.c_void_p * len(rs))(*[r.h for r in rs])
    t = reference.lib.ref_tlas_build(C.c_void_p(inst.ctypes.data), inst.shape[0], arr, len(rs))     # (BLASInstance::Update fills inst)
    mine = E.fill_instances(E.families(len(vs))[0], E.mesh_bounds(vs))
    for f in ("invTransform", "aabbMin", "aabbMax"):
        assert np.array_equal(mine[f].view(np.uint32), inst[f].view(np.uint32)), f
    p = C.c_void_p()
    nn = reference.lib.ref_tlas_blob(t, 2, C.byref(p)); nodes = np.frombuffer((C.c_char * (nn * 32)).from_address(p.value), np.uint32).reshape(-1, 8).copy()
    ni = reference.lib.ref_tlas_blob(t, 1, C.byref(p)); idx = np.frombuffer((C.c_char * (ni * 4)).from_address(p.value), np.uint32).copy()
    bl = [(r.blob(1, 0, np.uint32, 8), r.blob(1, 1, np.uint32, 1).reshape(-1), v) for r, v in zip(rs, vs)]
    rays, groups = E.ray_groups(inst, dict(enumerate(vs)))
    tmax = np.float32(0.3 * E.scene_diagonal(inst))
    finite = rays.copy(); finite["t"] = tmax
    try:
        first = None
        for label, batch in (("far", rays), ("finite", finite), ("carried", E.carried(rays, tmax)), ("retrace", None)):
            if batch is None:       # the first result's hit distance as tmax, the rest of the record junk
                batch = first.copy(); batch["u"] = 7.0; batch["v"] = -3.0; batch["prim"] = 12345; batch["inst"] = 0xDEAD
            want = np.ascontiguousarray(batch).copy()
            reference.lib.ref_tlas_intersect(t, C.c_void_p(want.ctypes.data), want.shape[0], want.strides[0])
            got = tlas_intersect(oracle_ref, nodes, idx, inst, bl, batch)
            if first is None:
                first = want
            # compare_hits takes t < 1e30 for a hit: the records that changed are the hits here
            hit_w, hit_g = E.differing(want, batch), E.differing(got, batch)
            assert np.array_equal(hit_w, hit_g), (label, hit_w.size, hit_g.size)
            c = compare_hits(got[hit_w], want[hit_w])
            print(label, "hits", hit_w.size, "bit-identical", c["bit_identical"], "same prim", c["same_prim"], "ties", c["tie"])
            assert c["hitmiss"] == 0 and c["prim_real"] == 0 and c["t_bad"] == 0 and c["uv_bad"] == 0, (label, c)
            same = (got["prim"] == want["prim"]) & (got["t"] == want["t"])
            assert np.array_equal(got["inst"][same], want["inst"][same]), label
            miss = np.setdiff1d(np.arange(batch.shape[0]), hit_w)
            assert np.array_equal(E.bytes_of(got[miss]), E.bytes_of(batch[miss])) and np.array_equal(E.bytes_of(want[miss]), E.bytes_of(batch[miss])), label
            if label != "retrace":
                assert hit_w.size > 300 and miss.size > 300, (label, hit_w.size, miss.size)
            if label == "far":      # every family but the masked-out one is hit, the projective one included
                hit_inst = set(want["inst"][hit_w].tolist())
                assert hit_inst >= set(range(inst.shape[0])) - {names.index("mask_none"), names.index("dup0"), names.index("dup1")}, sorted(hit_inst)
                assert names.index("mask_none") not in hit_inst and hit_inst & {names.index("dup0"), names.index("dup1")}
                assert hit_w[groups["mask0"].start <= hit_w].size == 0      # (the mask-0 group is last)
    finally:
        reference.lib.ref_tlas_free(t)


def random_opmap(n_tris, N, seed, density=0.6):
    rng = np.random.default_rng(seed)
    wpt = (N * N + 31) // 32
    m = np.zeros((n_tris, wpt), np.uint32)
    bits = rng.random((n_tris, N * N)) < density
    for b in range(N * N):
        m[:, b >> 5] |= (bits[:, b].astype(np.uint32) << np.uint32(b & 31))
    return m


@pytest.mark.parametrize("N", [4, 8, 32])
def test_opacity_micromaps_equal_the_reference(oracle_ref, reference, N):
    """IntersectTri / TriOccludes with opacity micromaps (tiny_bvh.h:8514-8522, 8562-8570): restated index arithmetic
    against the real BVH::Intersect / IsOccluded with SetOpacityMicroMaps."""
    import ctypes as C
    verts = scenes.blob(4000, seed=3)
    rs = reference.build(verts, hq=False, threaded=False)
    om = random_opmap(verts.shape[0] // 3, N, seed=N)
    prim, rnd = batches(verts)
    rays = np.concatenate([prim, rnd])
    plain = rs.intersect(1, rays)
    reference.lib.ref_set_opmap(rs.h, C.c_void_p(om.ctypes.data), N)
    want = rs.intersect(1, rays)
    sh = R.shadow(plain, verts[:, :3].max(0) * 1.5, 1e-5)
    want_occ = rs.occluded(1, sh)
    reference.lib.ref_set_opmap(rs.h, None, 0)
    assert int((want["prim"] != plain["prim"]).sum()) > 500          # the maps really cut holes
    oracle_ref.set_opmap(om, N)
    try:
        got = oracle_ref.bvh2_intersect(rs.blob(1, 0, np.uint32, 8), rs.blob(1, 1, np.uint32, 1).reshape(-1), verts, rays)
        got_occ = oracle_ref.bvh2_occluded(rs.blob(1, 0, np.uint32, 8), rs.blob(1, 1, np.uint32, 1).reshape(-1), verts, sh)
    finally:
        oracle_ref.set_opmap(None, 0)
    exact(got, want)
    assert np.array_equal(got_occ, want_occ)
