"""fp64 custom geometry (sphere BLASes of BVH_Double) without a GPU: the restatement's three walks against each other, the host builder, the
upload's validation (all of it before any device call), the numpy restatement of the device builder over sphere boxes, the ABI tables."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import tinybvh_amd as tb
from custom_double_lib import (GOLDEN, GOLDEN_SETS, N_RAYS, bounce_rays, camera_rays, cd_ref, chain_spheres, check_tree, decorate, golden_rays,  # noqa: F401
                               karras_spheres, mismatches, ocd, sphere_boxes, sphere_set, tlas_rays, tlas_scene)   # (ocd, cd_ref: fixtures)
from double_anim_lib import check_tlas_tree
from native_build import ROOT, syntax_check
from tinybvh_amd import _capi, lib

NEW_SYMBOLS = ("tbvh_upload_custom_spheres_double", "tbvh_host_build_custom_spheres_double", "tbvh_build_device_custom_spheres_double",
               "tbvh_rebuild_custom_spheres_double_device", "tbvh_custom_spheres_double_download")


def test_header_and_binding_declare_the_same_symbols():
    with open(os.path.join(ROOT, "include", "tinybvh_amd.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint " + name + r"\(", header), f"{name} is not declared in tinybvh_amd.h"
        assert name in _capi.SYMBOLS, f"{name} is not bound in _capi.py"
        assert hasattr(lib, name)
    assert lib.tbvh_abi_version() == 5


def test_null_handles_are_refused_by_name():
    s = np.zeros((1, 4)); h = C.c_void_p()
    calls = {
        "tbvh_upload_custom_spheres_double": lambda: lib.tbvh_upload_custom_spheres_double(None, None, 0, None, 0, None, 0, C.byref(h)),
        "tbvh_host_build_custom_spheres_double": lambda: lib.tbvh_host_build_custom_spheres_double(None, 1, C.byref(h)),
        "tbvh_build_device_custom_spheres_double": lambda: lib.tbvh_build_device_custom_spheres_double(None, s.ctypes.data, 1, 0, C.byref(h)),
        "tbvh_rebuild_custom_spheres_double_device": lambda: lib.tbvh_rebuild_custom_spheres_double_device(None, s.ctypes.data, 1, 0),
        "tbvh_custom_spheres_double_download": lambda: lib.tbvh_custom_spheres_double_download(None, None, 0, None, 0, None, 0, None, None),
    }
    for name, call in calls.items():
        assert call() == -1 and name in lib.tbvh_last_error().decode(), (name, lib.tbvh_last_error())


@pytest.mark.parametrize("name", ["bunny", "soup", "small", "dups", "one"])
def test_host_builder_makes_a_valid_tree(name):
    sph = sphere_set(name)
    h = tb.host_build_custom_spheres_double(sph)
    nodes, idx = h.nodes(), h.prim_idx()
    assert np.array_equal(np.sort(idx), np.arange(sph.shape[0], dtype=np.uint64))
    check_tree(nodes, idx, sph)
    lo, hi = sphere_boxes(sph)
    assert np.array_equal(nodes[0]["aabbMin"], lo.min(0)) and np.array_equal(nodes[0]["aabbMax"], hi.max(0))
    if name == "one":
        assert nodes[0]["triCount"] == 1 and nodes[0]["leftFirst"] == 0


def _upload_rc(nodes, n_nodes, idx, sph, n_sph):
    """the checks run before the context is touched: a context that is no context shows that no device call is made"""
    fake_ctx = C.c_void_p(8)
    h = C.c_void_p()
    rc = lib.tbvh_upload_custom_spheres_double(fake_ctx, nodes.ctypes.data, n_nodes, idx.ctypes.data, idx.size, sph.ctypes.data, n_sph, C.byref(h))
    return rc, lib.tbvh_last_error().decode()


def test_validation_names_the_first_bad_entry():
    sph = sphere_set("soup")[:200].copy()
    host = tb.host_build_custom_spheres_double(sph)
    nodes, idx = host.nodes().copy(), host.prim_idx().copy()
    interior = int(np.nonzero(nodes["triCount"] == 0)[0][0]); leaf = int(np.nonzero(nodes["triCount"] > 0)[0][0])
    cases = []
    n = nodes.copy(); n[interior]["leftFirst"] = len(nodes) - 1; cases.append(("child", n, idx, sph, f"node {interior}: child index"))
    n = nodes.copy(); n[leaf]["leftFirst"] = idx.size - 1; n[leaf]["triCount"] = 2; cases.append(("leaf range", n, idx, sph, f"node {leaf}: leaf range"))
    i = idx.copy(); i[17] = 200; cases.append(("primIdx", nodes, i, sph, "primIdx[17] = 200 >= n_spheres"))
    n = nodes.copy(); n[int(n[interior]["leftFirst"])]["leftFirst"] = n[interior]["leftFirst"]; n[int(n[interior]["leftFirst"])]["triCount"] = 0
    cases.append(("cycle", n, idx, sph, "reachable along two paths"))
    s = sph.copy(); s[5, 3] = np.nan; cases.append(("r = NaN", nodes, idx, s, "sphere 5: r = nan"))
    s = sph.copy(); s[9, 3] = -0.5; cases.append(("r < 0", nodes, idx, s, "sphere 9: r = -0.5"))
    s = sph.copy(); s[3, 3] = np.inf; cases.append(("r = inf", nodes, idx, s, "sphere 3: r = inf"))
    for what, n, i, s, msg in cases:
        rc, err = _upload_rc(n, len(n), i, s, 200)
        assert rc == -5 and msg in err and "tbvh_upload_custom_spheres_double" in err, (what, rc, err)


@pytest.mark.parametrize("n", [1, 2, 3, 64, 1000])
def test_numpy_builder_over_sphere_boxes(n):
    sph = sphere_set("soup")[:n]
    nodes, idx = karras_spheres(sph)
    boxes = np.zeros(n, [("aabbMin", "<f8", 3), ("aabbMax", "<f8", 3)])
    boxes["aabbMin"], boxes["aabbMax"] = sphere_boxes(sph)
    check_tlas_tree(nodes, idx, boxes)
    check_tree(nodes, idx, sph)
    assert len(nodes) == 2 * n - 1 and (n > 1 or (nodes[0]["triCount"] == 1 and nodes[0]["leftFirst"] == 0))


# ---- the three walks ------------------------------------------------------------------------------------------------------------------------
def _fixture_rays(ocd, sph, nodes, idx):
    cam = decorate(camera_rays(sph), 3)
    traced = ocd.intersect(nodes, idx, sph, camera_rays(sph), rule=1)
    return {"camera": cam, "bounce": decorate(bounce_rays(sph, traced), 4)}


@pytest.mark.parametrize("name", ["bunny", "soup"])
def test_rule0_rule1_and_brute_force_agree(ocd, name):
    """The fixtures the GPU tests assert on: the reference's rule, the library's rule and the brute force give the same records, on the host
    builder's tree and on the device builder's tree alike (counts: DESIGN.md par. 9)."""
    sph = sphere_set(name)
    h = tb.host_build_custom_spheres_double(sph)
    kn, ki = karras_spheres(sph)
    for kind, rays in _fixture_rays(ocd, sph, h.nodes(), h.prim_idx()).items():
        brute = ocd.brute(sph, rays, rule=1)
        hits = int((brute["t"] != rays["t"]).sum())
        assert hits > N_RAYS // (10 if kind == "camera" else 50), (name, kind, hits)   # (most bounce rays leave the set)
        counts = {}
        for tree, (nodes, idx) in {"host": (h.nodes(), h.prim_idx()), "lbvh": (kn, ki)}.items():
            r0 = ocd.intersect(nodes, idx, sph, rays, rule=0); r1 = ocd.intersect(nodes, idx, sph, rays, rule=1)
            counts[tree] = (mismatches(r0, r1), mismatches(r1, brute), mismatches(r0, ocd.brute(sph, rays, rule=0)))
            occ = ocd.occluded(nodes, idx, sph, rays, rule=1)
            assert np.array_equal(occ.astype(bool), brute["t"] != rays["t"]) and np.array_equal(occ, ocd.occluded(nodes, idx, sph, rays, rule=0))
            hit = brute["t"] != rays["t"]
            assert np.array_equal(r1["u"], rays["u"]) and np.array_equal(r1["v"], rays["v"]) and np.array_equal(r1["inst"][hit], rays["instIdx"][hit])
            assert r1[~hit].tobytes() == rays[~hit].tobytes()
        print(f"{name} {kind}: {hits} hits; (rule 0 / rule 1, rule 1 / brute, rule 0 / brute 0) differ: {counts}")
        assert all(c == (0, 0, 0) for c in counts.values()), (name, kind, counts)


def test_exact_duplicates_name_the_smaller_prim(ocd):
    sph = sphere_set("dups")
    h = tb.host_build_custom_spheres_double(sph)
    rays = camera_rays(sph, 512)
    for nodes, idx in ((h.nodes(), h.prim_idx()), karras_spheres(sph)):
        r1 = ocd.intersect(nodes, idx, sph, rays, rule=1)
        hit = r1["t"] < 1e299
        assert hit.sum() > 50 and (r1["prim"][hit] == 0).all()
        assert mismatches(r1, ocd.brute(sph, rays, rule=1)) == 0
        r0 = ocd.intersect(nodes, idx, sph, rays, rule=0)
        assert np.array_equal(r0["t"], r1["t"])   # the reference's rule names whichever duplicate it met first
        print("rule 0 names a prim other than 0 on", int((r0["prim"][hit] != 0).sum()), "of", int(hit.sum()), "hits")


def test_far_from_the_origin_keeps_the_prims(ocd):
    """The small soup moved by (1e7, -1e7, 1e7), rays moved alike: the library's rule names the same sphere as at the origin wherever the brute
    force over the moved set does (the moved positions round: 1e7 + x is not exact)."""
    from custom_double_lib import FAR, translated
    sph = sphere_set("small")
    far = sph.copy(); far[:, :3] += FAR
    rays = camera_rays(sph)
    h0, h1 = tb.host_build_custom_spheres_double(sph), tb.host_build_custom_spheres_double(far)
    near = ocd.intersect(h0.nodes(), h0.prim_idx(), sph, rays, rule=1)
    moved = ocd.intersect(h1.nodes(), h1.prim_idx(), far, translated(rays, FAR), rule=1)
    assert mismatches(moved, ocd.brute(far, translated(rays, FAR), rule=1)) == 0
    hit = near["t"] < 1e299
    same = (moved["t"] < 1e299) == hit
    same &= ~hit | (moved["prim"] == near["prim"])
    print("far from the origin:", int(hit.sum()), "hits,", int((~same).sum()), "rays name another sphere than at the origin")
    assert hit.sum() > N_RAYS // 10 and (~same).sum() <= 2   # (grazing rays, where a position's rounding by 2e-9 decides)
    assert np.abs(moved["t"][hit & same] - near["t"][hit & same]).max() < 1e-7


def test_chain_needs_the_spill_area(ocd):
    nodes, idx, sph = chain_spheres(220)
    n = 256
    rng = np.random.default_rng(4)
    O = np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n), np.full(n, 3.0 * 220 + 40.0)], 1)
    rays = tb.make_rays_ex(O, np.tile([0.0, 0.0, -1.0], (n, 1)) + np.concatenate([rng.normal(0, 1e-5, (n, 2)), np.zeros((n, 1))], 1))
    r1, depth = ocd.intersect(nodes, idx, sph, rays, rule=1, depth=True)
    assert (r1["prim"] == 220).all() and depth > 200   # (the LDS top holds 16 entries)


def test_two_level_rules_agree(ocd):
    """six instances over a sphere BLAS and a triangle BLAS: rule 0 and rule 1 part only where a ray starts inside the box of a triangle
    instance, hits a triangle and then a nearer sphere: the reference leaves the triangle's u, v, the library writes the record's own"""
    sph, verts, inst = tlas_scene()
    hs, ht = tb.host_build_custom_spheres_double(sph), tb.host_build_double(verts)
    lo, hi = sphere_boxes(sph)
    bounds = np.stack([np.concatenate([lo.min(0), hi.max(0)]), np.concatenate([verts.min(0), verts.max(0)])])
    th = tb.host_build_tlas_double(inst, bounds)
    rays = decorate(tlas_rays(inst), 6)
    blas = [("sph", hs.nodes(), hs.prim_idx(), sph), ("tri", ht.nodes(), ht.prim_idx(), verts)]
    r0 = ocd.tlas_intersect(th.nodes(), th.prim_idx(), inst, blas, rays, rule=0)
    r1 = ocd.tlas_intersect(th.nodes(), th.prim_idx(), inst, blas, rays, rule=1)
    hit = r1["t"] != rays["t"]
    assert hit.sum() > N_RAYS // 10 and np.unique(r1["inst"][hit]).size == 5 and not (r1["inst"][hit] == 5).any()
    on_sphere = hit & np.isin(r1["inst"], [0, 1, 3])
    assert np.array_equal(r1["u"][on_sphere], rays["u"][on_sphere]) and np.array_equal(r1["v"][on_sphere], rays["v"][on_sphere])
    for f in ("t", "prim", "inst"):
        assert np.array_equal(r0[f], r1[f]), f
    stale = (r0["u"] != r1["u"]) | (r0["v"] != r1["v"])
    print("two-level:", int(hit.sum()), "hits;", int(stale.sum()), "records where the reference keeps a triangle's u, v under a sphere hit")
    assert not stale[~on_sphere].any()
    o0 = ocd.tlas_occluded(th.nodes(), th.prim_idx(), inst, blas, rays, rule=0); o1 = ocd.tlas_occluded(th.nodes(), th.prim_idx(), inst, blas, rays, rule=1)
    assert np.array_equal(o0, o1) and np.array_equal(o1.astype(bool), hit)


# ---- the restatement against the real reference, and against what it recorded ----------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDEN_SETS)
def test_restatement_equals_reference_blas(ocd, cd_ref, name):
    """rule 0 on the tree BVH_Double::Build( customGetAABB, n ) made equals BVH_Double::Intersect through the callbacks, record for record in all
    bytes; the tree is a valid one over the sphere boxes, and the committed golden holds exactly it"""
    sph = sphere_set(name)
    h = cd_ref.build_spheres(sph)
    try:
        nodes, idx = cd_ref.blob(h)
        check_tree(nodes, idx, sph)
        for kind, rays in golden_rays(name, ocd).items():
            assert mismatches(ocd.intersect(nodes, idx, sph, rays, rule=0), cd_ref.intersect(h, rays)) == 0, (name, kind)
        g = np.load(os.path.join(GOLDEN, name + ".npz"))
        assert g["nodes"].tobytes() == nodes.tobytes() and np.array_equal(g["prim_idx"], idx)
    finally:
        cd_ref.free(h)


def test_restatement_equals_reference_tlas(ocd, cd_ref):
    sph, verts, inst = tlas_scene()
    hs, ht = cd_ref.build_spheres(sph), cd_ref.build_tris(verts)
    try:
        ours = inst.copy()
        lo, hi = sphere_boxes(sph)
        th = tb.host_build_tlas_double(ours, np.stack([np.concatenate([lo.min(0), hi.max(0)]), np.concatenate([verts.min(0), verts.max(0)])]))
        t = cd_ref.tlas_build(inst, [hs, ht])
        try:
            assert inst.tobytes() == ours.tobytes()   # BLASInstanceEx::Update, as the library's host builder restates it
            (sn, si), (tn, ti), (ln, li) = cd_ref.blob(hs), cd_ref.blob(ht), cd_ref.blob(t, tlas=True)
            rays = decorate(tlas_rays(inst), 6)
            want = cd_ref.intersect(t, rays, tlas=True)
            got = ocd.tlas_intersect(ln, li, inst, [("sph", sn, si, sph), ("tri", tn, ti, verts)], rays, rule=0)
            assert mismatches(got, want) == 0
            assert (want["t"] != rays["t"]).sum() > N_RAYS // 10
        finally:
            cd_ref.tlas_free(t)
    finally:
        cd_ref.free(hs); cd_ref.free(ht)


@pytest.mark.parametrize("name", GOLDEN_SETS)
def test_goldens_restated(ocd, name):
    """without the reference: its recorded tree is valid, and rule 0 and rule 1 on it give the records it recorded"""
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    sph = sphere_set(name)
    check_tree(g["nodes"], g["prim_idx"], sph)
    for kind, rays in golden_rays(name, ocd).items():
        assert rays.tobytes() == g[kind + "_rays"].tobytes(), "the batch the golden was recorded for is not the one the tests make"
        for rule in (0, 1):
            got = ocd.intersect(g["nodes"], g["prim_idx"], sph, rays, rule=rule)
            assert np.array_equal(got["t"], g[kind + "_t"]) and np.array_equal(got["prim"], g[kind + "_prim"]) and np.array_equal(got["inst"], g[kind + "_inst"]), (kind, rule)
            assert np.array_equal(got["u"], rays["u"]) and np.array_equal(got["v"], rays["v"])


def test_tiny_hip_sphere_double_binding_compiles(tmp_path):
    syntax_check(tmp_path, '#include "tiny_bvh.h"\n#include "tiny_hip.h"\n'
                 "struct Sphere { tinybvh::bvhdbl3 pos; double r; };\n"
                 "void f(tinybvh::BVH_Double& b, tinybvh::BVH_Double& tri, tinybvh::BVH_Double& tlas, const Sphere* s, tinybvh::RayEx* r, uint8_t* o) {\n"
                 "    tinyhip::SphereBVH_Double sb(b, s, 100); tinyhip::Scene st(tri); tinyhip::SphereBVH_Double sd(s, 100); std::vector<tinyhip::Scene*> v{&sb, &st, &sd}; tinyhip::Scene t(tlas, v);\n"
                 "    sb.Intersect(r, 4); sb.IsOccluded(r, 4, o); sb.RebuildOnDevice(s, 100); t.Intersect(r, 4); t.IsOccluded(r, 4, o); t.RebuildOnDevice();\n}\n")
