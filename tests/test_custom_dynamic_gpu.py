"""Sphere BLASes that move, on the GPU (DESIGN.md par. 12): tbvh_build_device_custom_spheres, tbvh_rebuild_custom_spheres_device,
tbvh_refit_custom_spheres and tbvh_custom_spheres_download.  Every tree is downloaded and checked in numpy (structure, boxes = the refit rule
restated in custom_dynamic_lib.wald_refit), every query equals the library-rule restatement (tests/oracle_custom.c) over the downloaded arrays
byte for byte, and the records are compared with a brute-force minimum over the spheres.

The brute-force comparison allows 1 differing record per set: the documented class, a sphere the sphere test reports hit while the slab test
misses its box.  A sphere with r < 0 is in that class by construction — its box pos - r .. pos + r is inverted, and no slab test passes an
inverted box, while the sphere test (which squares r) still reports hits — so records whose brute-force winner has r < 0 are counted apart and
not against the bound: on the soup with eight negated radii there are 4 of them among these 3000 rays on ANY tree (measured on the host
builder's tree without a GPU); every other difference still counts."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tinybvh_amd as tb
from custom_dynamic_lib import BUILD_SETS, build_set, check_boxes, check_structure
from custom_lib import caterpillar, cu_oracle, decorate, mismatches, rays_for, same_records, shadow_rays, sphere_set  # noqa: F401
from test_custom_host import anim_scene, tlas_rays

pytestmark = pytest.mark.gpu
lib = tb.lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BUILDERS = {"lbvh1": dict(builder="lbvh", max_leaf=1), "lbvh4": dict(builder="lbvh", max_leaf=4), "ploc8": dict(builder="ploc", radius=8),
            "ploc16": dict(builder="ploc", radius=16)}


@pytest.fixture(scope="module")
def ctx():
    c = tb.Context(0)
    yield c
    c.close()


def _rays(sph):
    return np.concatenate([decorate(rays_for(sph, 1000, 17, k), 17 + i) for i, k in enumerate(("camera", "incoherent", "inside"))])


def _check_queries(cu_oracle, sc, nodes, pi, sph, rays):
    """Intersect, IsOccluded and shadow rays from the hits = the restatement over the downloaded arrays, byte for byte"""
    want, _ = cu_oracle.intersect(nodes, pi, sph, rays, rule=1)
    got = sc.Intersect(rays.copy())
    assert mismatches(got, want) == 0
    assert np.array_equal(sc.IsOccluded(rays), cu_oracle.occluded(nodes, pi, sph, rays, rule=1))
    sh = shadow_rays(want, sph[:, :3].mean(0) + np.float32(25))
    assert np.array_equal(sc.IsOccluded(sh), cu_oracle.occluded(nodes, pi, sph, sh, rule=1))
    return got


def _check_brute(cu_oracle, sph, rays, got, what):
    """at most 1 record differs from the brute-force minimum (module docstring: winners with r < 0 are counted apart)"""
    want = cu_oracle.brute(sph, rays, rule=1)
    x, y = same_records(got, want)
    diff = np.nonzero((x != y).any(1))[0]
    hit = want["t"][diff] < np.float32(1e30)
    inverted = hit & (sph[np.where(hit, want["prim"][diff], 0), 3] < 0)
    if diff.size:
        print(f"{what}: {diff.size} records differ from brute force, {int(inverted.sum())} of them won by a sphere with r < 0:",
              [(int(i), float(got["t"][i]), int(got["prim"][i]), float(want["t"][i]), int(want["prim"][i])) for i in diff[:8]])
    assert diff.size - int(inverted.sum()) <= 1, what


def _check_scene(cu_oracle, sc, sph, rays, max_leaf, what, node1_unused=True):
    """download, structure, boxes, gathered spheres, queries, brute force; returns the downloaded (nodes, prim_idx)"""
    nodes, pi, gathered = sc.Download()
    check_structure(nodes, pi, sph.shape[0], max_leaf, node1_unused)
    check_boxes(nodes, pi, sph)
    assert np.array_equal(gathered.view(np.uint32), sph[pi].view(np.uint32))
    f = nodes.view(np.float32)
    assert np.array_equal(sc._bounds, np.concatenate([f[0, 0:3], f[0, 4:7]]))
    got = _check_queries(cu_oracle, sc, nodes, pi, sph, rays)
    _check_brute(cu_oracle, sph, rays, got, what)
    return nodes, pi


# ---- 1. build --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BUILD_SETS)
@pytest.mark.parametrize("how", list(BUILDERS))
def test_build(ctx, cu_oracle, how, name):
    sph = build_set(name)
    sc = tb.SphereBVH(ctx).BuildOnDevice(sph, **BUILDERS[how])
    assert lib.tbvh_scene_layout(sc._h) == tb.LAYOUT_BVH2_WALD
    assert ctx.time_last_ms() > 0
    _check_scene(cu_oracle, sc, sph, _rays(sph), BUILDERS[how].get("max_leaf", 1), f"{how} {name}")
    sc.free()


@pytest.mark.parametrize("how", list(BUILDERS))
def test_build_terminates_on_non_finite_spheres(ctx, how):
    """non-finite values are not refused: the build ends with a structurally valid tree"""
    sph = build_set("rand65")
    sph[3, 0] = np.nan; sph[17, 3] = np.inf; sph[40, 3] = np.nan; sph[41, 1] = -np.inf; sph[64] = np.nan
    sc = tb.SphereBVH(ctx).BuildOnDevice(sph, **BUILDERS[how])
    nodes, pi, gathered = sc.Download()
    check_structure(nodes, pi, 65, BUILDERS[how].get("max_leaf", 1))
    assert np.array_equal(gathered.view(np.uint32), sph[pi].view(np.uint32))
    sc.Refit(sph)
    nodes2, pi2, _ = sc.Download()
    assert np.array_equal(nodes2[:, 3], nodes[:, 3]) and np.array_equal(nodes2[:, 7], nodes[:, 7]) and np.array_equal(pi2, pi)
    sc.free()


def test_build_from_device_memory(ctx, cu_oracle):
    sph = build_set("rand257")
    d = ctx.malloc(sph.nbytes)
    try:
        ctx.to_device(d, sph)
        sc = tb.SphereBVH(ctx).BuildOnDevice((d, sph.shape[0]))
        _check_scene(cu_oracle, sc, sph, _rays(sph), 1, "device-resident spheres")
        sc.free()
    finally:
        ctx.free(d)


# ---- 2. refit --------------------------------------------------------------------------------------------------------------------------
def _moved(sph, rng):
    out = sph.copy()
    out[:, :3] += rng.normal(0, 0.3, (sph.shape[0], 3)).astype(np.float32)
    out[:, 3] *= rng.uniform(0.5, 1.5, sph.shape[0]).astype(np.float32)
    return out


@pytest.mark.parametrize("start", ["device_lbvh1", "device_lbvh4", "uploaded"])
def test_refit(ctx, cu_oracle, start):
    """three frames of motion in a row, then one from a device-resident array: topology and primIdx stay bit for bit, boxes = the restatement"""
    sph = sphere_set("soup")
    if start == "uploaded":   # the host builder's tree: not in the device builders' node order, node 1 in use
        sc = tb.SphereBVH(ctx).Build(sph)
        max_leaf = sph.shape[0]
    else:
        max_leaf = int(start[-1])
        sc = tb.SphereBVH(ctx).BuildOnDevice(sph, max_leaf=max_leaf)
    nodes0, pi0, _ = sc.Download()
    rng = np.random.default_rng(5)
    d = ctx.malloc(sph.nbytes)
    try:
        for frame in range(4):
            sph = _moved(sph, rng)
            if frame < 3:
                sc.Refit(sph)
            else:
                ctx.to_device(d, sph)
                sc.Refit((d, sph.shape[0]))
            assert ctx.time_last_ms() > 0
            nodes, pi = _check_scene(cu_oracle, sc, sph, _rays(sph), max_leaf, f"refit {start} frame {frame}", node1_unused=start != "uploaded")
            assert np.array_equal(nodes[:, 3], nodes0[:, 3]) and np.array_equal(nodes[:, 7], nodes0[:, 7]) and np.array_equal(pi, pi0)
    finally:
        ctx.free(d)
    sc.free()


def test_refit_deeper_than_one_batch(ctx, cu_oracle):
    """the caterpillar: height 100, more passes than one batch; its children are numbered after their parents only by accident of its maker"""
    nodes0, pi0, sph = caterpillar(100)
    sc = tb.SphereBVH(ctx).Upload(nodes0, pi0, sph)
    moved = sph.copy(); moved[:, 1] += np.float32(0.25)
    sc.Refit(moved)
    O = np.tile(np.array([[-10.0, 0.25, 0.0]], np.float32), (256, 1)); O[:, 1:] += np.linspace(-0.5, 0.5, 256, dtype=np.float32)[:, None]
    rays = np.concatenate([tb.make_rays(O, np.tile(np.array([[1.0, 0.0, 0.0]], np.float32), (256, 1))), _rays(moved)])
    nodes, pi = _check_scene(cu_oracle, sc, moved, rays, 1, "caterpillar", node1_unused=True)
    assert np.array_equal(nodes[:, 3], nodes0[:, 3]) and np.array_equal(nodes[:, 7], nodes0[:, 7]) and np.array_equal(pi, pi0)
    assert np.array_equal(sc._bounds, [2.0, -0.75, -1.0, 304.0, 1.25, 1.0])
    sc.free()


# ---- 3. rebuild and refit in place under a TLAS ------------------------------------------------------------------------------------------
def _al_to_wald(al):
    """BVH_GPU (Aila-Laine) TLAS nodes as Wald nodes: every AL interior node's two children become a sibling pair (as tests/test_custom_gpu.py)"""
    al = np.ascontiguousarray(al, np.uint32).reshape(-1, 16)
    out = [np.zeros(8, np.uint32), np.zeros(8, np.uint32)]
    stack = [(0, 0)]
    while stack:
        a, w = stack.pop()
        if al[a, 11]:   # leaf: triCount, firstTri
            out[w][3] = al[a, 15]; out[w][7] = al[a, 11]
            continue
        first = len(out)
        out[w][3] = first
        for k, (lo, hi, child) in enumerate(((0, 4, al[a, 3]), (8, 12, al[a, 7]))):
            n = np.zeros(8, np.uint32)
            n[0:3] = al[a, lo:lo + 3]; n[4:7] = al[a, hi:hi + 3]
            out.append(n)
            stack.append((int(child), first + k))
    return np.array(out, np.uint32)   # (the root's box is never tested)


def _check_tlas_arrays(cu_oracle, tl, tn, ti, inst, blas_desc, rays, exact):
    want = cu_oracle.tlas_intersect(tn, ti, inst, blas_desc, rays, rule=1)
    got = tl.Intersect(rays.copy())
    n_sph_inst = int((inst["blasIdx"] == 0).sum())
    sphere_hit = (want["t"] < np.float32(1e30)) & (want["inst"] < n_sph_inst)
    if exact:
        assert mismatches(got, want) == 0
    else:   # triangle hits as the TLAS tests compare them (DESIGN.md par. 4); sphere hits byte for byte
        assert mismatches(got[sphere_hit], want[sphere_hit]) == 0
        from oracle_lib import compare_hits
        c = compare_hits(got, want)
        assert c["hitmiss"] <= 2 and c["prim_real"] == 0 and c["t_bad"] == 0, c
    occ_want = cu_oracle.tlas_occluded(tn, ti, inst, blas_desc, rays, rule=1)
    occ = tl.IsOccluded(rays)
    assert (occ != occ_want).sum() <= (0 if exact else 2)
    assert int(sphere_hit.sum()) > 0
    return want


@pytest.mark.parametrize("start", ["device", "uploaded"])
def test_rebuild_and_refit_under_a_tlas(ctx, cu_oracle, start):
    """tiny_bvh_anim.cpp's scene with the sphere BLAS moving: the TLAS is uploaded ONCE; after every rebuild / refit of the BLAS only
    tl.RebuildOnDevice() runs (the instance boxes follow the new root box), and the TLAS traces the new tree.  An uploaded scene's arrays are
    replaced by its first rebuild: the TLAS is re-pointed."""
    sph, tris, inst = anim_scene(spheres="bunny16")
    s = tb.SphereBVH(ctx).BuildOnDevice(sph) if start == "device" else tb.SphereBVH(ctx).Build(sph)
    t = tb.BVH8_CWBVH(ctx).Build(tris)
    tl = tb.TLAS(ctx).Build(inst, [s, t])
    rays = tlas_rays(1000, 41)
    h = t.host
    rng = np.random.default_rng(11)
    sizes = []
    for step in ("rebuild", "rebuild", "rebuild", "refit", "refit"):
        sph = _moved(sph, rng)
        if step == "rebuild":
            s.RebuildOnDevice(sph)
            sizes.append(s.device_bytes)
        else:
            s.Refit(sph)
        tl.RebuildOnDevice()
        nodes64, idx, inst3 = tl.Download()
        nodes, pi, _ = s.Download()
        check_structure(nodes, pi, sph.shape[0], 1)
        check_boxes(nodes, pi, sph)
        desc = [("sph", nodes, pi, sph), ("tri", h.bvh2_nodes(), h.bvh2_prim_idx(), tris)]
        _check_tlas_arrays(cu_oracle, tl, _al_to_wald(nodes64), idx, inst3, desc, rays, exact=False)
    assert sizes[2] == sizes[1], sizes   # no allocation per frame
    tl.free(); t.free(); s.free()


# ---- 4. refusals and accounting --------------------------------------------------------------------------------------------------------
def _live():
    out = (C.c_uint64 * 2)()
    tb.check(lib.tbvh_debug_device_allocations(out), "tbvh_debug_device_allocations")
    return int(out[0]), int(out[1])


def test_refusals_and_accounting(ctx):
    import gc
    sph = sphere_set("soup")[:64].copy()
    gc.collect()   # (scenes earlier tests dropped are freed by their finalizers: not in the middle of the count)
    before = _live()
    s = tb.SphereBVH(ctx).BuildOnDevice(sph)
    tri = tb.BVH_GPU(ctx).Build(tb.scenes.soup(64, seed=1))
    out, nn = C.c_void_p(), C.c_uint64(0)
    p = tb._ptr(sph)
    calls = {
        "tbvh_rebuild_custom_spheres_device (wrong n)": lambda: lib.tbvh_rebuild_custom_spheres_device(s._h, p, 63, 0),
        "tbvh_refit_custom_spheres (wrong n)": lambda: lib.tbvh_refit_custom_spheres(s._h, p, 65, 0),
        "tbvh_rebuild_custom_spheres_device (null spheres)": lambda: lib.tbvh_rebuild_custom_spheres_device(s._h, None, 64, 0),
        "tbvh_refit_custom_spheres (null spheres)": lambda: lib.tbvh_refit_custom_spheres(s._h, None, 64, 0),
        "tbvh_rebuild_custom_spheres_device (null scene)": lambda: lib.tbvh_rebuild_custom_spheres_device(None, p, 64, 0),
        "tbvh_refit_custom_spheres (null scene)": lambda: lib.tbvh_refit_custom_spheres(None, p, 64, 0),
        "tbvh_custom_spheres_download (null scene)": lambda: lib.tbvh_custom_spheres_download(None, None, 0, None, 0, None, 0, C.byref(nn), C.byref(nn)),
        "tbvh_build_device_custom_spheres (null spheres)": lambda: lib.tbvh_build_device_custom_spheres(ctx._h, None, 64, 0, 0, 0, 0, C.byref(out)),
        "tbvh_build_device_custom_spheres (null out)": lambda: lib.tbvh_build_device_custom_spheres(ctx._h, p, 64, 0, 0, 0, 0, None),
        "tbvh_build_device_custom_spheres (no spheres)": lambda: lib.tbvh_build_device_custom_spheres(ctx._h, p, 0, 0, 0, 0, 0, C.byref(out)),
        "tbvh_build_device_custom_spheres (max_leaf 5)": lambda: lib.tbvh_build_device_custom_spheres(ctx._h, p, 64, 0, 0, 5, 0, C.byref(out)),
        "tbvh_build_device_custom_spheres (builder 2)": lambda: lib.tbvh_build_device_custom_spheres(ctx._h, p, 64, 0, 2, 0, 0, C.byref(out)),
        "tbvh_build_device_custom_spheres (radius 33)": lambda: lib.tbvh_build_device_custom_spheres(ctx._h, p, 64, 0, 1, 0, 33, C.byref(out)),
        "tbvh_build_device_custom_spheres (2^31 spheres)": lambda: lib.tbvh_build_device_custom_spheres(ctx._h, p, 1 << 31, 0, 0, 0, 0, C.byref(out)),
        "tbvh_rebuild_custom_spheres_device (a triangle scene)": lambda: lib.tbvh_rebuild_custom_spheres_device(tri._h, p, 64, 0),
        "tbvh_refit_custom_spheres (a triangle scene)": lambda: lib.tbvh_refit_custom_spheres(tri._h, p, 64, 0),
        "tbvh_custom_spheres_download (a triangle scene)": lambda: lib.tbvh_custom_spheres_download(tri._h, None, 0, None, 0, None, 0, C.byref(nn), C.byref(nn)),
        "tbvh_custom_spheres_download (a node buffer too small)": lambda: lib.tbvh_custom_spheres_download(s._h, p, 1, None, 0, None, 0, None, None),
    }
    for name, f in calls.items():
        rc = f()
        msg = lib.tbvh_last_error().decode()
        assert rc == -1, (name, rc, msg)   # TBVH_E_INVALID
        assert name.split(" ")[0] in msg, (name, msg)
        assert not out.value
    # the refusals of the triangle calls stand for a device-built sphere scene as for an uploaded one
    v = np.ascontiguousarray(tb.scenes.soup(64, seed=1), np.float32)
    assert lib.tbvh_refit(s._h, tb._ptr(v), 64, 0) == -1 and "(custom geometry)" in lib.tbvh_last_error().decode()
    assert lib.tbvh_scene_download(s._h, 0, None, 0, None) == -1 and "(custom geometry)" in lib.tbvh_last_error().decode()
    # the scene still answers, and every refused call left it as it was
    nodes, pi, _ = s.Download()
    check_structure(nodes, pi, 64, 1); check_boxes(nodes, pi, sph)
    # accounting: the scene counts what it holds, the scratch of the later calls included, and gives all of it back
    size0 = s.device_bytes
    assert size0 >= nodes.nbytes + pi.size * 32
    s.Refit(sph)
    assert s.device_bytes > size0   # (the refit's pass words)
    assert _live()[1] - before[1] >= s.device_bytes
    tri.free(); s.free()
    assert _live() == before


# ---- 5. the C++ example ----------------------------------------------------------------------------------------------------------------
def test_example_runs():
    """examples/sphere_particles.cpp (built by __graft_entry__.build()): build, four refits and a rebuild from C++, each frame checked by the
    program against its own brute-force loop"""
    exe = os.path.join(ROOT, "examples", "_build", "sphere_particles")
    if not os.path.exists(exe):
        pytest.skip("examples/_build/sphere_particles not built (needs the reference header at build time)")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "sphere particles ok" in out.stdout
    assert len([l for l in out.stdout.split("\n") if l.startswith("frame ")]) == 6
