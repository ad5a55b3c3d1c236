"""Device-side BLAS refit (tbvh_refit): after the vertices move, queries through the
refitted blob must return the reference's hit records for the NEW geometry (BVH::Intersect on a BVH
built over the moved vertices: hit records do not depend on the tree), the refitted boxes must be
conservative, and refitting to unchanged vertices must reproduce the encoder's blob."""
import numpy as np
import pytest

import tinybvh_amd as tb
from tinybvh_amd import rays as R
from tinybvh_amd import scenes
from oracle_lib import compare_hits
from tree_check import assert_tree, check_tree, describe


def deform(verts, amount, seed):
    """Smooth, seeded displacement of every vertex (shared vertices move together: the mesh stays closed)."""
    v = verts.copy()
    p = v[:, :3]
    rng = np.random.default_rng(seed)
    k = rng.uniform(0.5, 2.0, (3, 3)).astype(np.float32); ph = rng.uniform(0, 6.28, 3).astype(np.float32)
    d = np.stack([np.sin(p @ k[0] + ph[0]), np.sin(p @ k[1] + ph[1]), np.sin(p @ k[2] + ph[2])], 1).astype(np.float32)
    v[:, :3] = p + np.float32(amount) * d
    return v


def oracle_hits(oracle, verts, rays):
    h = tb.HostBVH(verts, tb.LAYOUT_BVH_GPU)
    return oracle.bvh2_intersect(h.bvh2_nodes(), h.bvh2_prim_idx(), verts, rays)


def check(got, want):
    c = compare_hits(got, want)
    assert c["hitmiss"] == 0 and c["prim_real"] == 0 and c["t_bad"] == 0 and c["uv_bad"] == 0, c
    assert c["tie"] <= 4 and c["onsurf"] <= 4, c
    assert c["bit_identical"] == c["same_prim"], c
    return c


def blobs(sc):
    nodes, tris = sc.download_blobs()
    return nodes, (None if sc.layout == tb.LAYOUT_BVH4_GPU else tris)


def check_boxes(sc, verts, held, label):
    """the refitted boxes are conservative (and exact where the format is, tight where it quantises: tests/tree_check.py), the records are the moved
    triangles', and the tree still reaches the prim words `held` it reached before"""
    F = assert_tree(sc.layout, *blobs(sc), verts, prims=held, label=label)
    print(label, describe(F))
    return F


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [tb.LAYOUT_CWBVH, tb.LAYOUT_BVH_GPU, tb.LAYOUT_BVH4_GPU])
def test_refit_parity(ctx, oracle, layout):
    verts = scenes.blob(8000, seed=3)
    sc = tb.LAYOUT_CLASSES[layout](ctx).Build(verts)
    lo, hi = verts[:, :3].min(0) - 0.5, verts[:, :3].max(0) + 0.5
    rays = R.random_rays(40_000, lo, hi, seed=11)
    check(sc.Intersect(rays.copy()), oracle_hits(oracle, verts, rays))
    held = check_tree(layout, *blobs(sc), verts)["prims"]   # (the default BVH8_CWBVH build may hold a triangle in several leaves)
    for frame, amount in enumerate((0.05, 0.2, 0.0)):       # the last frame returns to the rest pose
        v2 = deform(verts, amount, seed=frame) if amount else verts
        sc.Refit(v2)
        check_boxes(sc, v2, held, f"frame {frame}")
        want = oracle_hits(oracle, v2, rays)
        c = check(sc.Intersect(rays.copy()), want)
        assert c["hits"] > 4000
        occ = sc.IsOccluded(rays.copy())
        assert int((occ.astype(bool) != (want["t"] < 1e30)).sum()) <= 2
    # vertices that already live on the device
    v3 = deform(verts, 0.1, seed=9)
    d_v = ctx.malloc(v3.nbytes); ctx.to_device(d_v, v3)
    sc.Refit((d_v, v3.shape[0] // 3), on_device=True)
    check_boxes(sc, v3, held, "device-resident vertices")
    check(sc.Intersect(rays.copy()), oracle_hits(oracle, v3, rays))
    ctx.free(d_v)


@pytest.mark.gpu
def test_refit_to_same_vertices_reproduces_the_encoder(ctx):
    """CWBVH: the device re-quantisation is the host encoder's arithmetic: same vertices -> same node bytes."""
    verts = scenes.soup(3000, seed=5)
    sc = tb.BVH8_CWBVH(ctx).Build(verts, split_budget=0.0)      # whole triangles: a leaf box is its triangles' box, which is what a refit computes
    before_n = sc.host.blob(0, np.uint32, 4).copy(); before_t = sc.host.blob(1, np.uint32, 4).copy()
    sc.Refit(verts)
    n, t = sc.download_blobs()
    assert np.array_equal(t, before_t)
    same = np.all(n.reshape(-1, 20) == before_n.reshape(-1, 20), axis=1)
    assert same.mean() > 0.999, f"{(~same).sum()} of {same.size} nodes differ"


@pytest.mark.gpu
def test_refit_of_a_split_tree_keeps_every_record(ctx, oracle):
    """The default BVH8_CWBVH tree holds PIECES of large triangles (TBVH_BUILD_SPLIT_TRIANGLES): a refit fits every leaf to its whole triangles again
    (looser boxes, same topology, the triangle records untouched) — the hit records must not change, before or after moving the vertices."""
    verts = scenes.rotate(scenes.rotate(scenes.atrium(30_000, seed=1), 0, 0.618), 1, 0.755)
    sc = tb.BVH8_CWBVH(ctx).Build(verts)
    assert sc.host.blob(1, np.uint32, 4).shape[0] // 3 > verts.shape[0] // 3                    # the tree does hold split triangles
    lo, hi = verts[:, :3].min(0), verts[:, :3].max(0)
    rays = R.random_rays(40_000, lo, hi, seed=11)
    want = oracle_hits(oracle, verts, rays)
    check(sc.Intersect(rays.copy()), want)
    before_t = sc.host.blob(1, np.uint32, 4).copy()
    sc.Refit(verts)
    n, t = sc.download_blobs()
    assert np.array_equal(t, before_t)
    held = before_t.reshape(-1, 3, 4)[:, 2, 3]
    check_boxes(sc, verts, held, "refitted to the same vertices")
    check(sc.Intersect(rays.copy()), want)
    v2 = deform(verts, 0.1, seed=4)
    sc.Refit(v2)
    check_boxes(sc, v2, held, "refitted to moved vertices")
    check(sc.Intersect(rays.copy()), oracle_hits(oracle, v2, rays))


@pytest.mark.gpu
def test_refit_on_reference_built_blob(ctx, oracle):
    """Blobs built by the real tiny_bvh.h (golden fixture) are refittable too."""
    import os
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "soup_2k.npz"))
    verts = g["verts"]
    rays = g["rays"].copy()
    v2 = deform(verts, 0.03, seed=2)
    want = oracle_hits(oracle, v2, rays)
    for k in (0, 1):                                     # BVH::Build and BuildHQ (SBVH: prims shared between leaves)
        sc = tb.BVH8_CWBVH(ctx).Upload(g[f"cwbvh_nodes_{k}"], g[f"cwbvh_tris_{k}"])
        sc.Refit(v2)
        check(sc.Intersect(rays.copy()), want)
        sg = tb.BVH_GPU(ctx).Upload(g[f"bvhgpu_nodes_{k}"], g[f"bvhgpu_idx_{k}"], verts)
        sg.Refit(v2)
        check(sg.Intersect(rays.copy()), want)
        s4 = tb.BVH4_GPU(ctx).Upload(g[f"bvh4_{k}"])
        s4.Refit(v2)
        check(s4.Intersect(rays.copy()), want)


@pytest.mark.gpu
def test_refit_errors(ctx):
    verts = scenes.soup(600, seed=1)
    tl = tb.TLAS(ctx).Build(tb.make_instances(np.eye(4, dtype=np.float32)[None], np.zeros(1, np.uint32)), [tb.BVH8_CWBVH(ctx).Build(verts)])
    with pytest.raises(tb.TbvhError):
        tb.check(tb.lib.tbvh_refit(tl._h, verts.ctypes.data_as(__import__("ctypes").c_void_p), verts.shape[0] // 3, 0), "refit of a TLAS")
    sc = tb.BVH8_CWBVH(ctx).Build(verts)
    sc.Refit(verts[: 3 * 100])                          # vertex array shorter than the blob's primitives
    r = R.random_rays(64, (-1, -1, -1), (1, 1, 1), seed=1)
    with pytest.raises(tb.TbvhError):
        sc.Intersect(r)                                  # reported by the next synchronising call
