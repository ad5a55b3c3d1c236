"""Custom-geometry sphere BLASes on the host (DESIGN.md par. 12): the restatement (tests/oracle_custom.c) against the real reference
(tests/custom_ref_shim.cpp: BVH::Build( customGetAABB, n ) and the anim demo's sphere callback), against a brute-force minimum, the library's
host builder, and the counted deviation classes.  No GPU."""
import os

import numpy as np
import pytest

import tinybvh_amd as tb
from custom_lib import GOLDEN, caterpillar, cu_oracle, cu_ref, decorate, mismatches, rays_for, shadow_rays, sphere_set  # noqa: F401

SETS = ["bunny", "soup", "dups"]


def _rays(spheres, seed):
    return np.concatenate([decorate(rays_for(spheres, 3000, seed, k), seed + i) for i, k in enumerate(("camera", "incoherent", "inside"))])


def _wald_tree_ok(nodes, prim_idx, spheres):
    """every sphere once; leaf boxes = the union of pos -/+ r of their spheres, interior boxes = the union of the children's"""
    f = nodes.view(np.float32)
    seen = np.zeros(spheres.shape[0], np.int64)
    stack = [0]
    while stack:
        k = stack.pop()
        lf, tc = int(nodes[k, 3]), int(nodes[k, 7])
        if tc:
            s = spheres[prim_idx[lf:lf + tc]]
            seen[prim_idx[lf:lf + tc]] += 1
            lo, hi = (s[:, :3] - s[:, 3:4]).min(0), (s[:, :3] + s[:, 3:4]).max(0)
        else:
            stack += [lf, lf + 1]
            lo = np.minimum(f[lf, 0:3], f[lf + 1, 0:3]); hi = np.maximum(f[lf, 4:7], f[lf + 1, 4:7])
        assert np.array_equal(f[k, 0:3], lo) and np.array_equal(f[k, 4:7], hi), k
    assert (seen == 1).all()


@pytest.mark.parametrize("name", SETS + ["one"])
def test_host_builder_makes_a_valid_tree(name):
    sph = sphere_set(name)
    nodes, pi = tb.host_build_custom_spheres(sph)
    assert nodes.shape[1] == 8 and pi.size == sph.shape[0]
    _wald_tree_ok(nodes, pi, sph)


@pytest.mark.parametrize("name", SETS)
def test_restatement_equals_reference_blas(cu_oracle, cu_ref, name):
    """rule 0 restates BVH::Intersect / IsOccluded with the callback bit for bit, on the reference's own tree"""
    sph = sphere_set(name)
    h = cu_ref.build_spheres(sph)
    try:
        nodes, pi = cu_ref.blob(h, 0), cu_ref.blob(h, 1)
        rays = _rays(sph, 3)
        want = cu_ref.intersect(h, rays)
        got, _ = cu_oracle.intersect(nodes, pi, sph, rays, rule=0)
        assert mismatches(got, want) == 0
        sh = shadow_rays(want, sph[:, :3].mean(0) + np.float32(30))
        assert np.array_equal(cu_oracle.occluded(nodes, pi, sph, sh, rule=0), cu_ref.occluded(h, sh))
        assert np.array_equal(cu_oracle.occluded(nodes, pi, sph, rays, rule=0), cu_ref.occluded(h, rays))
    finally:
        cu_ref.free(h)


@pytest.mark.parametrize("name", SETS + ["one"])
def test_library_rule_equals_brute_force(cu_oracle, name):
    """rule 1 over the tree = the minimum over every sphere (smallest recorded distance, then the smaller prim)"""
    sph = sphere_set(name)
    nodes, pi = tb.host_build_custom_spheres(sph)
    rays = _rays(sph, 5)
    got, _ = cu_oracle.intersect(nodes, pi, sph, rays, rule=1)
    want = cu_oracle.brute(sph, rays, rule=1)
    assert mismatches(got, want) == 0


def test_near_tie_class_is_counted(cu_oracle):
    """the reference's first-accepted rule against the library's: they differ only where the recorded distances tie (or nearly: within the
    rounding of t * reciMag * mag); on exact duplicates the library names the smaller prim"""
    counts = {}
    for name in SETS:
        sph = sphere_set(name)
        nodes, pi = tb.host_build_custom_spheres(sph)
        rays = _rays(sph, 9)
        r0, _ = cu_oracle.intersect(nodes, pi, sph, rays, rule=0)
        r1, _ = cu_oracle.intersect(nodes, pi, sph, rays, rule=1)
        d = (r0["prim"] != r1["prim"]) | (r0["t"] != r1["t"])
        # every difference is a near-tie: the two distances within a few ulps
        rel = np.abs(r0["t"][d].astype(np.float64) - r1["t"][d]) / np.maximum(np.abs(r1["t"][d]), 1e-30)
        assert (rel <= 4e-7).all(), name
        assert (r1["t"][d] <= r0["t"][d]).all() or name == "dups"
        counts[name] = int(d.sum())
    print("near-tie differences (rule 0 vs rule 1):", counts)
    assert counts["dups"] > 0 and counts["bunny"] + counts["soup"] <= 20


def test_callback_forms_counted(cu_oracle):
    """the anim demo's callback against tiny_bvh_custom.cpp's unit-direction form, for constructor-made (normalised) rays: |D| rounds to 1
    only within an ulp, so the recorded distances often differ in their last bits; the sphere named differs only at near-ties"""
    total = prim = n = 0
    for name in SETS:
        sph = sphere_set(name)
        rays = _rays(sph, 13)
        a = cu_oracle.brute(sph, rays, rule=0)
        b = cu_oracle.brute_unit(sph, rays)
        total += mismatches(a, b); n += rays.shape[0]
        prim += int((a["prim"] != b["prim"]).sum())
    print(f"callback forms: {total} of {n} records differ, {prim} of them in the sphere named (or hit / miss)")
    assert prim <= 0.02 * n


def test_caterpillar_depth(cu_oracle):
    nodes, pi, sph = caterpillar(100)
    r = tb.make_rays(np.array([[-10.0, 0.0, 0.0]], np.float32), np.array([[1.0, 0.0, 0.0]], np.float32))
    got, depth = cu_oracle.intersect(nodes, pi, sph, r, rule=1)
    assert depth == 100 and got["prim"][0] == 100 and got["t"][0] == np.float32(12.0)


# ---- TLAS ------------------------------------------------------------------------------------------------------------------------------
def anim_scene(n_side=3, seed=3, spheres="bunny", n_tris=4000):
    """tiny_bvh_anim.cpp's kind of scene: scaled (and here also rotated) instances of the bunny spheres on a grid, plus one triangle BLAS;
    some instances masked"""
    rng = np.random.default_rng(seed)
    sph = sphere_set(spheres)
    tris = tb.scenes.atrium(n_tris, seed=2)
    xf = []
    for x in range(n_side):
        for y in range(n_side):
            for z in range(n_side):
                a = rng.uniform(0, np.pi)
                c, s = np.cos(a), np.sin(a)
                m = np.eye(4, dtype=np.float32)
                m[:3, :3] = np.float32(0.6) * np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float32) if (x + y + z) % 2 else np.float32(0.6) * np.eye(3, dtype=np.float32)
                m[:3, 3] = [x * 5 - n_side * 2.5, y * 5 - n_side * 2.5 + 7, z * 5 - n_side * 2.5 + 1]
                xf.append(m)
    xf.append(np.eye(4, dtype=np.float32))
    inst = tb.make_instances(np.array(xf), [0] * (len(xf) - 1) + [1])
    inst["mask"][::5] = 0x2
    return sph, tris, inst


def tlas_rays(n, seed):
    rng = np.random.default_rng(seed)
    eye = np.array([-15.24, 21.5, 2.54], np.float32)
    r = tb.make_rays(np.broadcast_to(eye, (n, 3)), rng.uniform(-1, 1, (n, 3)) + np.array([0.826, -0.438, -0.356]))
    r2 = tb.make_rays(rng.uniform(-8, 12, (n, 3)), rng.normal(size=(n, 3)))
    r = np.concatenate([r, r2])
    r["mask"][::3] = 0x1
    return decorate(r, seed)


def test_restatement_equals_reference_tlas(cu_oracle, cu_ref):
    """IntersectTLAS / IsOccludedTLAS over sphere instances and a triangle BLAS, rule 0 = the reference bit for bit; the stale u, v of
    rule 0 (a sphere hit keeps the u, v of a triangle met before) is the counted class of DESIGN.md par. 12"""
    sph, tris, inst = anim_scene()
    hs, ht = cu_ref.build_spheres(sph), cu_ref.build_tris(tris)
    th = cu_ref.tlas_build(inst, [hs, ht])
    try:
        blas = [("sph", cu_ref.blob(hs, 0), cu_ref.blob(hs, 1), sph), ("tri", cu_ref.blob(ht, 0), cu_ref.blob(ht, 1), tris)]
        tn, ti = cu_ref.tlas_blob(th, 2), cu_ref.tlas_blob(th, 1)
        rays = tlas_rays(4000, 21)
        want = cu_ref.tlas_intersect(th, rays)
        got = cu_oracle.tlas_intersect(tn, ti, inst, blas, rays, rule=0)
        assert mismatches(got, want) == 0
        assert np.array_equal(cu_oracle.tlas_occluded(tn, ti, inst, blas, rays, rule=0), cu_ref.tlas_occluded(th, rays))
        lib = cu_oracle.tlas_intersect(tn, ti, inst, blas, rays, rule=1)
        sphere_hit = (lib["t"] < np.float32(1e30)) & (lib["inst"] < inst.shape[0] - 1)
        same = (lib["prim"] == want["prim"]) & (lib["inst"] == want["inst"]) & (lib["t"] == want["t"])
        stale = sphere_hit & same & ((lib["u"] != want["u"]) | (lib["v"] != want["v"]))
        print("TLAS: stale u, v under rule 0:", int(stale.sum()), "near-ties:", int((~same).sum()), "of", rays.shape[0])
        assert int((~same).sum()) <= 0.005 * rays.shape[0]
    finally:
        cu_ref.tlas_free(th)
        cu_ref.free(hs); cu_ref.free(ht)


@pytest.mark.parametrize("path", sorted(p for p in os.listdir(GOLDEN) if p.endswith(".npz")) if os.path.isdir(GOLDEN) else [])
def test_goldens_restated(cu_oracle, path):
    """the committed reference records (tools/make_custom_golden.py) equal the rule-0 restatement bit for bit"""
    g = np.load(os.path.join(GOLDEN, path))
    rays = g["rays"].view(tb.RAY_DTYPE).reshape(-1)
    if "tlas_nodes" in g:
        blas = [("sph", g["sph_nodes"], g["sph_idx"], g["spheres"]), ("tri", g["tri_nodes"], g["tri_idx"], g["tri_verts"])]
        got = cu_oracle.tlas_intersect(g["tlas_nodes"], g["tlas_idx"], g["instances"].view(tb.INSTANCE_DTYPE).reshape(-1), blas, rays, rule=0)
        occ = cu_oracle.tlas_occluded(g["tlas_nodes"], g["tlas_idx"], g["instances"].view(tb.INSTANCE_DTYPE).reshape(-1), blas, rays, rule=0)
    else:
        got, _ = cu_oracle.intersect(g["nodes"], g["prim_idx"], g["spheres"], rays, rule=0)
        occ = cu_oracle.occluded(g["nodes"], g["prim_idx"], g["spheres"], rays, rule=0)
    assert mismatches(got, g["hits"].view(tb.RAY_DTYPE).reshape(-1)) == 0
    assert np.array_equal(occ, g["occluded"])


def test_stale_uv_class(cu_oracle):
    """the second counted class: under a TLAS the reference keeps the u, v of a farther triangle it met first when a sphere then wins (the
    callback never writes them); the library writes the record's incoming u, v.  A triangle instance whose box holds the ray origins is
    entered first, the sphere instance lies in front of its far wall."""
    sph = np.array([[0.0, 0.0, 5.0, 1.0]], np.float32)
    tris = np.array([[-50, -50, 10, 0], [50, -50, 10, 0], [0, 50, 10, 0], [-50, -50, -1, 0], [0, 50, -1, 0], [50, -50, -1, 0]], np.float32)
    s_nodes, s_pi = tb.host_build_custom_spheres(sph)
    tb_h = tb.HostBVH(tris, tb.LAYOUT_BVH_GPU)
    t_nodes, t_pi = np.array(tb_h.bvh2_nodes()), np.array(tb_h.bvh2_prim_idx())
    inst = tb.make_instances(np.eye(4, dtype=np.float32)[None].repeat(2, 0), [0, 1])
    inst["invTransform"] = np.eye(4, dtype=np.float32).reshape(16)
    # a two-leaf Wald TLAS: root, then the triangle instance (box z -1..10, holds the origins) and the sphere instance (box z 4..6)
    tn = np.zeros((4, 8), np.uint32); f = tn.view(np.float32)
    f[0, 0:3] = [-50, -50, -1]; f[0, 4:7] = [50, 50, 10]; tn[0, 3] = 2
    f[2, 0:3] = [-50, -50, -1]; f[2, 4:7] = [50, 50, 10]; tn[2, 3] = 0; tn[2, 7] = 1
    f[3, 0:3] = [-1, -1, 4]; f[3, 4:7] = [1, 1, 6]; tn[3, 3] = 1; tn[3, 7] = 1
    ti = np.array([1, 0], np.uint32)   # leaf 2 -> instance 1 (the triangles), leaf 3 -> instance 0 (the sphere)
    g = np.linspace(-0.5, 0.5, 8, dtype=np.float32)
    O = np.stack(np.meshgrid(g, g), -1).reshape(-1, 2)
    rays = decorate(tb.make_rays(np.concatenate([O, np.zeros((O.shape[0], 1), np.float32)], 1), np.tile([0.0, 0.0, 1.0], (O.shape[0], 1))), 3)
    rays["t"] = np.float32(1e30)
    blas = [("sph", s_nodes, s_pi, sph), ("tri", t_nodes, t_pi, tris)]
    r0 = cu_oracle.tlas_intersect(tn, ti, inst, blas, rays, rule=0)
    r1 = cu_oracle.tlas_intersect(tn, ti, inst, blas, rays, rule=1)
    assert (r1["prim"] == 0).all() and (r1["inst"] == 0).all() and np.array_equal(r0["t"], r1["t"])
    assert np.array_equal(r1["u"], rays["u"]) and np.array_equal(r1["v"], rays["v"])
    stale = (r0["u"] != r1["u"]) | (r0["v"] != r1["v"])
    print("stale u, v (constructed):", int(stale.sum()), "of", rays.shape[0])
    assert stale.all()


def test_tiny_hip_sphere_binding_compiles(tmp_path):
    """tinyhip::SphereBVH against the real tiny_bvh.h: Build, Upload, Intersect, IsOccluded, Handle (examples/sphere_bvh.cpp; the program
    build() makes of it runs on the GPU in tests/test_custom_gpu.py: test_tiny_hip_sphere_binding_runs)"""
    from native_build import ROOT, syntax_check
    syntax_check(tmp_path, '#include "%s"\n' % os.path.join(ROOT, "examples", "sphere_bvh.cpp"))




def test_brute_force_limit_counted(cu_oracle):
    """where the tree and the brute-force minimum part: rays passing small spheres (r 0.001-0.05) 3000 units from the origin.  There
    c = |oc|^2 - r^2 carries an absolute rounding error near 1, far above r^2, so the sphere test can answer d > 0 for a ray the slab test
    sees miss the sphere's box.  The tree then reports a farther sphere (or none), never a nearer one; the
    reference's walk has the same limit.  The count is quoted in DESIGN.md par. 12."""
    rng = np.random.default_rng(29)
    n = 2000
    dirs = rng.normal(size=(n, 3)); dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    sph = np.empty((n, 4), np.float32)
    sph[:, :3] = dirs * 3000 + rng.normal(0, 20, (n, 3))
    sph[:, 3] = rng.uniform(0.001, 0.05, n)
    k = rng.integers(0, n, 120_000)
    side = np.cross(sph[k, :3].astype(np.float64), rng.normal(size=(k.size, 3)))
    side /= np.linalg.norm(side, axis=1)[:, None]
    tgt = sph[k, :3] + side * rng.uniform(0.0, 1.0, (k.size, 1))   # passing up to one unit off the centre: |oc|^2 ~ 9e6 has an ulp of 1
    rays = tb.make_rays(np.zeros((k.size, 3), np.float32), tgt)
    nodes, pi = tb.host_build_custom_spheres(sph)
    tree, _ = cu_oracle.intersect(nodes, pi, sph, rays, rule=1)
    brute = cu_oracle.brute(sph, rays, rule=1)
    diff = (tree["prim"] != brute["prim"]) | (tree["t"] != brute["t"])
    print(f"tree vs brute force on grazing rays at far small spheres: {int(diff.sum())} of {rays.shape[0]}")
    tt, bt, tp, bp = tree["t"][diff], brute["t"][diff], tree["prim"][diff], brute["prim"][diff]
    assert ((tt > bt) | ((tt == bt) & (tp > bp))).all()   # the brute-force winner always ranks first: the tree only loses candidates
    assert diff.sum() > 0
