"""Sphere-overlap queries on the GPU (kernels_sphere.hip): every answer byte must equal the restatement (tests/oracle_sphere.c) over the same
blob, for host-built blobs and reference-built ones (tests/golden/spheres, tools/make_sphere_golden.py); BVH_GPU answers must also equal the
real reference's wherever its walk took no leaf off the stack (DESIGN.md par. 11)."""
import ctypes as C
import os

import numpy as np
import pytest

import tinybvh_amd as tb
from tinybvh_amd import lib, scenes
from sphere_lib import GOLDEN, mesh, sph_oracle, sphere_sets  # noqa: F401 (sph_oracle: fixture)
from test_deep_tree import chain_bvh2

pytestmark = pytest.mark.gpu

LAYOUTS = [tb.LAYOUT_BVH_GPU, tb.LAYOUT_BVH4_GPU, tb.LAYOUT_CWBVH]


@pytest.fixture(scope="module")
def ctx():
    c = tb.Context(0)
    yield c
    c.close()


def host_blobs(sc):
    """the restatement's view of a scene built on the host (Build keeps the HostBVH)"""
    hb = sc.host
    if sc.layout == tb.LAYOUT_BVH_GPU:
        return [hb.blob(0, np.uint32, 16), hb.blob(1, np.uint32, 1).reshape(-1)]
    if sc.layout == tb.LAYOUT_BVH4_GPU:
        return [hb.blob(0, np.uint32, 4)]
    return [hb.blob(0, np.uint32, 4), hb.blob(1, np.uint32, 4)]


def downloaded_blobs(sc):
    """the same, read back from the device (tbvh_scene_download): BVH_GPU's primIdx from its gathered records' v0.w"""
    nodes, tris = sc.download_blobs()
    if sc.layout == tb.LAYOUT_BVH_GPU:
        return [nodes.reshape(-1, 16), np.ascontiguousarray(tris.reshape(-1, 12)[:, 3])]
    if sc.layout == tb.LAYOUT_BVH4_GPU:
        return [nodes]
    return [nodes, tris]


def all_spheres(verts, n32, seed, n=1500):
    return np.concatenate(list(sphere_sets(verts, n32, seed, n).values()))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", ["bunny", "atrium", "soup"])
def test_device_equals_restatement_host_built(ctx, sph_oracle, layout, name):
    verts = mesh(name)
    sc = tb.LAYOUT_CLASSES[layout](ctx).Build(verts)
    for kind, sp in sphere_sets(verts, sc.host.bvh2_nodes(), seed=7).items():
        got = sc.intersect_spheres(sp, verts)
        want = sph_oracle.layout(layout, host_blobs(sc), verts, sp)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{name} {kind}: {bad.size} of {sp.shape[0]} answers differ, first spheres {sp[bad[:3]]}"
        if kind == "random":
            assert 0 < want.sum() < sp.shape[0]
    sc.free()


@pytest.mark.parametrize("case", ["soup", "tri2"])
def test_device_equals_restatement_and_reference_on_goldens(ctx, sph_oracle, case):
    g = np.load(os.path.join(GOLDEN, case + ".npz"))
    verts, sp = g["verts"], g["spheres"]
    scs = {
        tb.LAYOUT_BVH_GPU: (tb.BVH_GPU(ctx).Upload(g["bvh_gpu"], g["prim_idx"], verts), [g["bvh_gpu"], g["prim_idx"]]),
        tb.LAYOUT_BVH4_GPU: (tb.BVH4_GPU(ctx).Upload(g["bvh4_gpu"]), [g["bvh4_gpu"]]),
        tb.LAYOUT_CWBVH: (tb.BVH8_CWBVH(ctx).Upload(g["cwbvh_nodes"], g["cwbvh_tris"]), [g["cwbvh_nodes"], g["cwbvh_tris"]]),
    }
    for layout, (sc, blobs) in scs.items():
        got = sc.intersect_spheres(sp, verts)
        np.testing.assert_array_equal(got, sph_oracle.layout(layout, blobs, verts, sp), err_msg=f"{case} layout {layout}")
        if layout == tb.LAYOUT_BVH_GPU:
            agree = g["agree"]
            np.testing.assert_array_equal(got[agree], g["answers"][agree], err_msg=f"{case}: BVH_GPU against the reference")
            print(f"{case}: {int(agree.sum())} of {sp.shape[0]} spheres compared with the reference's answers")
        sc.free()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_host_and_device_entry_points_agree(ctx, layout):
    verts = mesh("soup")
    sc = tb.LAYOUT_CLASSES[layout](ctx).Build(verts)
    sp = all_spheres(verts, sc.host.bvh2_nodes(), seed=9)
    want = sc.intersect_spheres(sp, verts)
    d_sp, d_v, d_hit = ctx.malloc(sp.nbytes), ctx.malloc(verts.nbytes), ctx.malloc(sp.shape[0])
    try:
        ctx.to_device(d_sp, sp); ctx.to_device(d_v, verts)
        sc.intersect_spheres_device(d_sp, sp.shape[0], d_v, verts.shape[0] // 3, d_hit)
        got = np.zeros(sp.shape[0], np.uint8)
        ctx.synchronize()
        ctx.from_device(got, d_hit)
        np.testing.assert_array_equal(got, want)
        assert ctx.time_last_ms() >= 0.0
    finally:
        for p in (d_sp, d_v, d_hit):
            ctx.free(p)
    for i in np.flatnonzero(np.isfinite(sp).all(1))[:20]:
        assert sc.intersect_sphere(sp[i, :3], float(sp[i, 3]), verts) == bool(want[i])
    sc.free()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_tail_sizes(ctx, sph_oracle, layout):
    verts = mesh("soup")
    sc = tb.LAYOUT_CLASSES[layout](ctx).Build(verts)
    base = all_spheres(verts, sc.host.bvh2_nodes(), seed=13, n=3000)[:4096]
    base_want = sph_oracle.layout(layout, host_blobs(sc), verts, base)
    for n in (1, 63, 65, (1 << 20) + 3, 16_777_216):
        idx = np.arange(n) % base.shape[0]
        got = sc.intersect_spheres(base[idx], verts)
        bad = np.flatnonzero(got != base_want[idx])
        assert bad.size == 0, f"n = {n}: {bad.size} answers differ, first at {bad[:5]}"
    sc.free()


def test_tree_deeper_than_the_lds_stack(ctx, sph_oracle):
    """the caterpillar of test_deep_tree.py: a sphere whose box overlaps every node but which touches no triangle (its centre lies off the
    clumps' hypotenuse y + z = 2 by more than r) visits the whole tree with many children pending; small spheres near the clumps hit or miss
    by 0.05 - r"""
    depth = 80
    n2, pi, verts = chain_bvh2(depth)
    far = np.array([[depth / 2, 40.0, 40.0, depth / 2 + 2.0], [depth + 0.15, 1.0, 1.0, 0.02], [depth + 0.15, 1.0, 1.0, 0.06],
                    [0.05, 0.5, 0.5, 0.06], [depth / 2 + 0.05, -0.5, -0.5, 0.01]], np.float32)
    for cls in (tb.BVH4_GPU, tb.BVH8_CWBVH):
        sc = cls(ctx).ConvertFromBVH2(n2, pi, verts)
        got = sc.intersect_spheres(far, verts)
        want = sph_oracle.layout(sc.layout, downloaded_blobs(sc), verts, far[:1])
        assert sph_oracle.last_max_stack() > 16, "the walk must hold more entries than the LDS part of the stack"
        np.testing.assert_array_equal(got, np.concatenate([want, sph_oracle.layout(sc.layout, downloaded_blobs(sc), verts, far[1:])]))
        assert got.tolist() == [0, 0, 1, 1, 0]
        sc.free()


def test_stack_overflow_is_reported_and_the_context_stays_usable(sph_oracle):
    depth = 2100
    n2, pi, verts = chain_bvh2(depth)
    old = os.environ.get("TBVH_SPILL_ENTRIES")
    os.environ["TBVH_SPILL_ENTRIES"] = "2"
    try:
        c = tb.Context(0)
    finally:
        if old is None:
            os.environ.pop("TBVH_SPILL_ENTRIES", None)
        else:
            os.environ["TBVH_SPILL_ENTRIES"] = old
    try:
        sc = tb.BVH8_CWBVH(c).ConvertFromBVH2(n2, pi, verts)
        big = np.array([[depth / 2, 900.0, 900.0, depth / 2 + 2.0]], np.float32)   # (as above: every box overlapped, no triangle touched)
        with pytest.raises(tb.TbvhError) as e:
            sc.intersect_spheres(big, verts)
        assert e.value.code == -5 and b"stack overflow" in lib.tbvh_last_error()
        small = np.array([[depth + 0.15, 1.0, 1.0, 0.06]], np.float32)
        assert sc.intersect_spheres(small, verts).tolist() == [1]
        sc.free()
    finally:
        c.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_after_refit(ctx, sph_oracle, layout):
    verts = mesh("atrium")
    sc = tb.LAYOUT_CLASSES[layout](ctx).Build(verts)
    rng = np.random.default_rng(3)
    moved = verts.copy()
    moved[:, :3] += rng.normal(0, 0.05, (verts.shape[0], 3)).astype(np.float32)
    sc.Refit(moved)
    blobs = downloaded_blobs(sc)
    for kind, sp in sphere_sets(moved, sc.host.bvh2_nodes(), seed=21, n=1000).items():
        np.testing.assert_array_equal(sc.intersect_spheres(sp, moved), sph_oracle.layout(layout, blobs, moved, sp), err_msg=kind)
    sc.free()


def test_refusals_and_the_context_keeps_working(ctx):
    """the argument refusals return before any launch; a short vertex array is found by the kernel (the scene does not know its largest
    primitive index), which skips those records and reports TBVH_E_FORMAT at the synchronizing call"""
    verts = mesh("soup")
    blas = tb.BVH_GPU(ctx).Build(verts)
    sp = all_spheres(verts, blas.host.bvh2_nodes(), seed=4)[:500]
    want = blas.intersect_spheres(sp, verts)
    hit = np.zeros(sp.shape[0], np.uint8)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731

    def refused(scene_h, code, what, spheres=sp, v=verts, out=hit, n_tris=None):
        n_tris = (verts if v is None else v).shape[0] // 3 if n_tris is None else n_tris
        r = lib.tbvh_intersect_spheres(scene_h, None if spheres is None else p(spheres), sp.shape[0], None if v is None else p(v), n_tris,
                                       None if out is None else p(out))
        assert r == code, (what, r, lib.tbvh_last_error())
        assert lib.tbvh_last_error()

    tlas = tb.TLAS(ctx).Build(tb.make_instances(np.eye(4, dtype=np.float32)[None], [0]), [blas])
    refused(tlas._h, -1, "TLAS")
    dbl = tb.BVH_Double(ctx).Build(verts.astype(np.float64)[:, :3])
    refused(dbl._h, -1, "BVH_Double")
    dense = np.zeros((4, 4, 4), np.uint32); dense[1, 2, 3] = 7
    vox = tb.VoxelSet(ctx).Build(dense)
    refused(vox._h, -1, "VoxelSet")
    refused(blas._h, -1, "null spheres", spheres=None)
    refused(blas._h, -1, "null vertices", v=None)
    refused(blas._h, -1, "null result", out=None)
    refused(blas._h, -1, "empty vertex array", n_tris=0)
    assert lib.tbvh_intersect_spheres(blas._h, None, 0, None, 0, None) == 0   # n_spheres == 0: a no-op
    np.testing.assert_array_equal(blas.intersect_spheres(sp, verts), want)
    # a vertex array shorter than the blob's primitives: the records beyond it are skipped and reported at the synchronizing call
    refused(blas._h, -5, "short vertex array", v=np.ascontiguousarray(verts[: verts.shape[0] // 2]))
    assert b"beyond the vertex array" in lib.tbvh_last_error()
    np.testing.assert_array_equal(blas.intersect_spheres(sp, verts), want)
    for s in (tlas, dbl, vox, blas):
        s.free()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_ray_queries_unchanged_by_sphere_queries(ctx, layout):
    verts = scenes.atrium(20_000, seed=1)
    sc = tb.LAYOUT_CLASSES[layout](ctx).Build(verts)
    rng = np.random.default_rng(1)
    lo, hi = verts[:, :3].min(0), verts[:, :3].max(0)
    O = lo + rng.random((4096, 3)).astype(np.float32) * (hi - lo)
    D = rng.normal(size=(4096, 3)).astype(np.float32)
    rays = tb.make_rays(O, D)
    before, again, occ_before = sc.Intersect(rays.copy()), sc.Intersect(rays.copy()), sc.IsOccluded(rays)
    sc.intersect_spheres(np.concatenate([O, np.full((4096, 1), 0.5, np.float32)], 1), verts)
    after, occ_after = sc.Intersect(rays.copy()), sc.IsOccluded(rays)
    np.testing.assert_array_equal(after["t"].view(np.uint32), before["t"].view(np.uint32))
    same = (before.view(np.uint8).reshape(-1, 64) == again.view(np.uint8).reshape(-1, 64)).all(1)   # (records a ray query itself reproduces)
    assert (before.view(np.uint8).reshape(-1, 64)[same] == after.view(np.uint8).reshape(-1, 64)[same]).all()
    np.testing.assert_array_equal(occ_before, occ_after)
    sc.free()
