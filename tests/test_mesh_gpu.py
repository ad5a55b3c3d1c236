"""Indexed and strided triangle meshes on the device (tbvh_mesh and the tbvh_*_mesh entry points; DESIGN.md par. 13).  The contract under test:
RESULTS DO NOT DEPEND ON THE FORM — for one set of triangles the indexed form, the strided form and the flat form give the same bytes: gathered
records, device-built and device-converted blobs, refitted nodes, sphere flags and hit records — and no flattened copy of the vertices is kept on
the device.  Every comparison is exact (array_equal on the bytes); where a builder numbers its nodes through atomics, two runs of the FLAT path
are compared first and, if they differ, the comparison is by hit records and by the sorted multiset of node boxes."""
import ctypes as C
import os

import numpy as np
import pytest

import tinybvh_amd as tb
from tinybvh_amd import _capi, scenes
from tinybvh_amd import rays as R
from oracle_lib import compare_hits, tlas_intersect
import mesh_lib as ml
from test_mesh_host import bunny, flatten, golden, hit_fields, interleave
from test_refit_device import check as check_hits, oracle_hits

pytestmark = pytest.mark.gpu
LAYOUTS = [tb.LAYOUT_BVH_GPU, tb.LAYOUT_BVH4_GPU, tb.LAYOUT_CWBVH]
lib = _capi.lib


def mixed_rays(flat, n, seed=3):
    """random rays through the box, rays from a camera outside it, and short rays (finite tmax): n in all"""
    lo, hi = flat[:, :3].min(0), flat[:, :3].max(0)
    ext = hi - lo
    a = R.random_rays(n // 2, lo - 0.2 * ext, hi + 0.2 * ext, seed=seed)
    rng = np.random.default_rng(seed + 1)
    m = n - n // 2
    eye = (lo + hi) * 0.5 + np.array([0.0, 0.1, 2.5], np.float32) * ext
    tgt = lo + rng.random((m, 3), dtype=np.float32) * ext
    b = tb.make_rays(np.broadcast_to(eye.astype(np.float32), (m, 3)).copy(), (tgt - eye).astype(np.float32))
    b["t"][::4] = np.float32(np.linalg.norm(ext) * 2.0)
    return np.concatenate([a, b])


def records(scene, rays):
    out = scene.Intersect(rays.copy())
    occ = scene.IsOccluded(rays.copy())
    return out.view(np.uint8).reshape(-1, 64), occ


def same_scene(a, b, rays, what):
    na, ta = a.download_blobs(); nb, tb_ = b.download_blobs()
    assert np.array_equal(na, nb), f"{what}: node blobs differ"
    assert np.array_equal(ta, tb_), f"{what}: triangle records differ"
    ra, oa = records(a, rays); rb, ob = records(b, rays)
    assert np.array_equal(ra, rb), f"{what}: {int((ra != rb).any(1).sum())} hit records differ"
    assert np.array_equal(oa, ob), f"{what}: IsOccluded differs"
    return ra


def three_forms(pos, idx):
    """(name, verts, indices) of one mesh: flat, indexed (bvhvec4 positions), indexed at a 32-byte stride with NaN behind every position,
    and that stride without indices.  pos has w = 0, so all four describe the same 16-byte vertices."""
    assert not pos[:, 3].any()
    flat = flatten(pos, idx)
    return flat, [("indexed", pos, idx), ("indexed+stride32", interleave(pos, 8), idx), ("stride32", interleave(flat, 8), None),
                  ("indexed+stride12", np.ascontiguousarray(pos[:, :3]), idx)]


# ---- uploads of host-built blobs ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", LAYOUTS)
def test_upload_does_not_depend_on_the_form(ctx, oracle, layout):
    pos, idx = bunny(2)                      # 34 815 triangles: a BVH_GPU / BVH4_GPU scene of this size owns a derived 8-wide copy
    flat, forms = three_forms(pos, idx)
    rays = mixed_rays(flat, 100_000)
    base = tb.LAYOUT_CLASSES[layout](ctx).Build(flat, threads=1)
    again = tb.LAYOUT_CLASSES[layout](ctx).Build(flat, threads=1)
    want = same_scene(base, again, rays, "two flat builds")          # the flat path is reproducible: the forms must be, too
    check_hits(base.Intersect(rays.copy()), oracle_hits(oracle, flat, rays))
    again.free()
    for name, v, i in forms:
        sc = tb.LAYOUT_CLASSES[layout](ctx).Build(v, indices=i, threads=1)
        got = same_scene(base, sc, rays, name)
        assert np.array_equal(got, want)
        # an indexed scene holds its index buffer and nothing else: no flattened vertices on the device
        assert sc.device_bytes == base.device_bytes + (12 * idx.shape[0] if i is not None else 0), name
        sc.free()
    base.free()


def test_upload_bvh_gpu_mesh_takes_a_blob_built_elsewhere(ctx):
    """tbvh_upload_bvh_gpu_mesh / tbvh_update_bvh_gpu_mesh with the blob's primIdx naming triangles of an indexed mesh, host and device resident"""
    pos, idx = bunny(8)
    flat = flatten(pos, idx)
    rays = mixed_rays(flat, 100_000)
    h = tb.HostBVH(flat, tb.LAYOUT_BVH_GPU, threads=1)
    nodes, prim = h.blob(0, np.uint32, 16), h.blob(1, np.uint32, 1)
    base = tb.BVH_GPU(ctx).Upload(nodes, prim, flat)
    a = tb.BVH_GPU(ctx).Upload(nodes, prim, pos, indices=idx)
    same_scene(base, a, rays, "host mesh")
    d_v = ctx.malloc(pos.nbytes); ctx.to_device(d_v, pos)
    d_i = ctx.malloc(idx.nbytes); ctx.to_device(d_i, idx)
    b = tb.BVH_GPU(ctx).Upload(nodes, prim, tb.device_mesh(d_v, pos.shape[0], idx.shape[0], d_i))
    same_scene(base, b, rays, "device mesh")
    for s in (base, a, b):
        s.free()
    ctx.free(d_v); ctx.free(d_i)


# ---- blobs the REAL reference built over an index buffer (tests/golden/mesh, tools/make_mesh_golden.py) ------------------------------------

def golden_budget(got, want, occ, want_occ, what):
    """the classes and budgets tests/test_golden.py applies to reference-built blobs of this size"""
    c = compare_hits(got, want)
    assert c["hitmiss"] + c["prim_real"] <= 1 and c["t_bad"] == 0 and c["uv_bad"] == 0 and c["tie"] <= 2 and c["onsurf"] <= 2, (what, c)
    assert c["bit_identical"] == c["same_prim"], (what, c)
    assert int((occ != want_occ).sum()) <= 1, what
    return c


def test_reference_built_indexed_blob_uploads_and_updates(ctx):
    """BVH_GPU::Build( slice, indices, n ) of the real reference through tbvh_upload_bvh_gpu_mesh, then its Refit() + ConvertFrom blob through
    tbvh_update_bvh_gpu_mesh (same topology, so the update always runs): the reference's own BVH::Intersect records and IsOccluded flags.  Host
    mesh, 32-byte-stride mesh and device-resident mesh; the flat upload of the flattened triangles beside them gives the same bytes."""
    g = golden()
    pos, idx, rays = g["positions"], g["indices"], hit_fields(g["rays"])
    flat = flatten(pos, idx)
    d_v = ctx.malloc(pos.nbytes); ctx.to_device(d_v, pos)
    d_i = ctx.malloc(idx.nbytes); ctx.to_device(d_i, idx)
    base = tb.BVH_GPU(ctx).Upload(g["bvhgpu_nodes"], g["prim_idx"], flat)
    forms = {"indexed": tb.BVH_GPU(ctx).Upload(g["bvhgpu_nodes"], g["prim_idx"], pos, indices=idx),
             "stride32": tb.BVH_GPU(ctx).Upload(g["bvhgpu_nodes"], g["prim_idx"], interleave(pos, 8), indices=idx),
             "device": tb.BVH_GPU(ctx).Upload(g["bvhgpu_nodes"], g["prim_idx"], tb.device_mesh(d_v, pos.shape[0], idx.shape[0], d_i))}
    for name, sc in forms.items():
        c = golden_budget(sc.Intersect(rays.copy()), hit_fields(g["hits"]), sc.IsOccluded(rays.copy()), g["occluded"], name)
        assert c["hits"] > 300
        same_scene(base, sc, rays, name)
    # the refitted blob: same node count by construction
    pos2 = g["positions_refit"]
    assert g["bvhgpu_nodes_refit"].shape == g["bvhgpu_nodes"].shape
    base.Update(g["bvhgpu_nodes_refit"], g["prim_idx_refit"], flatten(pos2, idx))
    ctx.to_device(d_v, pos2)
    for name, sc in forms.items():
        v = {"indexed": pos2, "stride32": interleave(pos2, 8), "device": tb.device_mesh(d_v, pos2.shape[0], idx.shape[0], d_i)}[name]
        sc.Update(g["bvhgpu_nodes_refit"], g["prim_idx_refit"], v, indices=None if name == "device" else idx)
        golden_budget(sc.Intersect(rays.copy()), hit_fields(g["hits_refit"]), sc.IsOccluded(rays.copy()), g["occluded_refit"], name + " updated")
        same_scene(base, sc, rays, name + " updated")
    # ... and the device refit of the first blob to the moved vertices answers like the reference's Refit()
    sc = tb.BVH_GPU(ctx).Upload(g["bvhgpu_nodes"], g["prim_idx"], pos, indices=idx)
    sc.Refit(pos2, mesh=True)
    golden_budget(sc.Intersect(rays.copy()), hit_fields(g["hits_refit"]), sc.IsOccluded(rays.copy()), g["occluded_refit"], "device refit")
    for x in list(forms.values()) + [base, sc]:
        x.free()
    ctx.free(d_v); ctx.free(d_i)


def test_sphere_flags_equal_the_golden(ctx):
    """tbvh_intersect_spheres_mesh on the reference-built blob: BVH::IntersectSphere's flags wherever the reference's walk is defined and took no leaf
    off the stack (DESIGN.md par. 11), and the flat call's flags everywhere; before and after the refit"""
    g = golden()
    pos, idx, sp = g["positions"], g["indices"], g["spheres"]
    sc = tb.BVH_GPU(ctx).Upload(g["bvhgpu_nodes"], g["prim_idx"], pos, indices=idx)
    for tag, p in (("", pos), ("_refit", g["positions_refit"])):
        if tag:
            sc.Update(g["bvhgpu_nodes_refit"], g["prim_idx_refit"], p, indices=idx)
        agree = g["sphere_agree" + tag]
        assert int(agree.sum()) > 2500
        flat_flags = sc.intersect_spheres(sp, flatten(p, idx))
        for name, v, i in (("indexed", p, idx), ("stride32", interleave(p, 8), idx)):
            got = sc.intersect_spheres(sp, v, indices=i)
            assert np.array_equal(got, flat_flags), name + tag
            assert np.array_equal(got[agree], g["sphere_answers" + tag][agree]), name + tag
        assert int(flat_flags.sum()) > 300
    sc.free()


# ---- device builders and the device conversion -----------------------------------------------------------------------------------------

def bvh4_nodes(blocks):
    """the node boxes of a BVH4_GPU stream (3 blocks per node: frame + quantised planes), found by walking it"""
    out, todo = [], [0]
    while todo:
        off = todo.pop()
        out.append(blocks[off:off + 3].reshape(-1))
        for w in blocks[off + 3]:
            if w and not (w >> 31):
                todo.append(int(w))
    return np.array(out)


def node_boxes(layout, nodes):
    if layout == tb.LAYOUT_CWBVH:   # n0 (origin, exponents, imask) and the quantised planes n2..n4; n1 holds child / triangle numbers
        n = nodes.reshape(-1, 20)
        rows = np.concatenate([n[:, :4], n[:, 8:]], 1)
    else:
        rows = bvh4_nodes(nodes)
    return rows[np.lexsort(rows.T[::-1])]


def same_built(layout, a, a2, b, rays, what):
    """a, a2: two runs of the flat path; b: the mesh form"""
    ra, oa = records(a, rays); ra2, _ = records(a2, rays); rb, ob = records(b, rays)
    assert np.array_equal(ra, ra2), "two flat runs give different hit records"
    assert np.array_equal(ra, rb), f"{what}: {int((ra != rb).any(1).sum())} hit records differ"
    assert np.array_equal(oa, ob), what
    na, ta = a.download_blobs(); na2, ta2 = a2.download_blobs(); nb, tb_ = b.download_blobs()
    assert na.shape == nb.shape and ta.shape == tb_.shape, what
    if np.array_equal(na, na2) and np.array_equal(ta, ta2):
        assert np.array_equal(na, nb) and np.array_equal(ta, tb_), f"{what}: the flat path is reproducible byte for byte, the mesh form differs"
    else:   # node numbering through atomics: the same boxes, in another order
        assert np.array_equal(node_boxes(layout, na), node_boxes(layout, na2)), "two flat runs give different node boxes"
        assert np.array_equal(node_boxes(layout, na), node_boxes(layout, nb)), f"{what}: node boxes differ"


@pytest.mark.parametrize("layout", [tb.LAYOUT_BVH4_GPU, tb.LAYOUT_CWBVH])
@pytest.mark.parametrize("builder", ["lbvh", "ploc"])
def test_device_build_does_not_depend_on_the_form(ctx, oracle, layout, builder):
    pos, idx = bunny(4)
    flat, forms = three_forms(pos, idx)
    rays = mixed_rays(flat, 100_000)
    cls = tb.LAYOUT_CLASSES[layout]
    a = cls(ctx).BuildOnDevice(flat, builder=builder); a2 = cls(ctx).BuildOnDevice(flat, builder=builder)
    check_hits(a.Intersect(rays.copy()), oracle_hits(oracle, flat, rays))
    for name, v, i in forms:
        b = cls(ctx).BuildOnDevice(v, builder=builder, indices=i)
        same_built(layout, a, a2, b, rays, f"{builder} {name}")
        assert b.device_bytes == a.device_bytes + (12 * idx.shape[0] if i is not None else 0), name
        b.free()
    a.free(); a2.free()


@pytest.mark.parametrize("layout", [tb.LAYOUT_BVH4_GPU, tb.LAYOUT_CWBVH])
def test_device_conversion_does_not_depend_on_the_form(ctx, layout):
    pos, idx = scenes.weld(scenes.atrium(20_000, seed=1))
    pos = pos.copy(); pos[:, 3] = 0
    flat, forms = three_forms(pos, idx)
    rays = mixed_rays(flat, 100_000)
    h = tb.HostBVH(pos, tb.LAYOUT_BVH2_WALD, threads=1, max_leaf_tris=3, indices=idx)
    n32, prim = h.bvh2_nodes(), h.bvh2_prim_idx()
    cls = tb.LAYOUT_CLASSES[layout]
    a = cls(ctx).ConvertFromBVH2(n32, prim, flat); a2 = cls(ctx).ConvertFromBVH2(n32, prim, flat)
    for name, v, i in forms:
        b = cls(ctx).ConvertFromBVH2(n32, prim, v, indices=i)
        same_built(layout, a, a2, b, rays, name)
        b.free()
    a.free(); a2.free()


# ---- refit -------------------------------------------------------------------------------------------------------------------------------

def deform_shared(pos, amount, seed):
    """a smooth displacement of the SHARED vertices: every triangle around a vertex moves with it"""
    v = pos.copy()
    p = v[:, :3]
    rng = np.random.default_rng(seed)
    k = rng.uniform(5.0, 20.0, (3, 3)).astype(np.float32); ph = rng.uniform(0, 6.28, 3).astype(np.float32)
    d = np.stack([np.sin(p @ k[0] + ph[0]), np.sin(p @ k[1] + ph[1]), np.sin(p @ k[2] + ph[2])], 1).astype(np.float32)
    v[:, :3] = p + np.float32(amount) * d
    return v


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("step", [1, 8], ids=["bunny", "bunny8"])
def test_refit_mesh_equals_refit_of_the_flattened_frame(ctx, oracle, layout, step):
    """three frames of moved shared vertices: host-staged with the scene's held indices (indices == NULL), host-staged at a 32-byte stride with
    indices passed again, device-resident.  step 1 = the whole bunny, 69 630 triangles: the BVH_GPU / BVH4_GPU scene owns an 8-wide copy, which
    the refit must carry along."""
    pos, idx = bunny(step)
    flat = flatten(pos, idx)
    n_rays = 120_000 if step == 1 else 100_000
    rays = mixed_rays(flat, n_rays)
    cls = tb.LAYOUT_CLASSES[layout]
    base = cls(ctx).Build(flat, threads=1)
    sc = cls(ctx).Build(pos, indices=idx, threads=1)
    same_scene(base, sc, rays, "before the first refit")       # (also the first large query: the derived copies exist from here on)
    bytes_before = (base.device_bytes, sc.device_bytes)
    assert bytes_before[1] == bytes_before[0] + 12 * idx.shape[0]
    d_v = ctx.malloc(pos.nbytes)
    ext = float(np.linalg.norm(flat[:, :3].max(0) - flat[:, :3].min(0)))
    for frame, amount in enumerate((0.01, 0.03, 0.0)):
        p2 = deform_shared(pos, amount * ext, seed=frame) if amount else pos
        f2 = flatten(p2, idx)
        base.Refit(f2)
        if frame == 0:
            sc.Refit(p2, mesh=True)                                     # the shared vertices and nothing else
        elif frame == 1:
            sc.Refit(interleave(p2, 8), indices=idx)                    # another stride, the indices replaced by themselves
        else:
            ctx.to_device(d_v, p2)
            sc.Refit(tb.device_mesh(d_v, p2.shape[0], idx.shape[0]))    # device-resident vertices, the held indices
        same_scene(base, sc, rays, f"frame {frame}")
        c = check_hits(sc.Intersect(rays.copy()), oracle_hits(oracle, f2, rays))
        assert c["hits"] > 10_000
        assert sc.device_bytes - base.device_bytes == 12 * idx.shape[0], "a hidden copy of the vertices?"
    # the flat call keeps working on a scene made from an indexed mesh
    p3 = deform_shared(pos, 0.02 * ext, seed=7); f3 = flatten(p3, idx)
    base.Refit(f3); sc.Refit(f3)
    same_scene(base, sc, rays, "tbvh_refit on the indexed scene")
    # held indices: the triangle count must be the scene's
    m = _capi.Mesh(C.c_void_p(p3.ctypes.data), p3.shape[0], 16, 0, None, idx.shape[0] - 1)
    assert lib.tbvh_refit_mesh(sc._h, C.byref(m)) == -1
    ctx.free(d_v); base.free(); sc.free()


# ---- sphere overlap, flatten, TLAS -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", LAYOUTS)
def test_sphere_flags_do_not_depend_on_the_form(ctx, layout):
    pos, idx = bunny(8)
    flat, forms = three_forms(pos, idx)
    lo, hi = flat[:, :3].min(0), flat[:, :3].max(0)
    rng = np.random.default_rng(5)
    sph = np.zeros((20_000, 4), np.float32)
    sph[:, :3] = lo + rng.random((sph.shape[0], 3), dtype=np.float32) * (hi - lo)
    sph[:, 3] = rng.random(sph.shape[0], dtype=np.float32) * np.float32(0.03 * np.linalg.norm(hi - lo))
    sc = tb.LAYOUT_CLASSES[layout](ctx).Build(pos, indices=idx, threads=1)
    want = sc.intersect_spheres(sph, flat)
    assert 500 < int(want.sum()) < sph.shape[0] - 500
    for name, v, i in forms:
        assert np.array_equal(sc.intersect_spheres(sph, v, indices=i), want), name
    d_v = ctx.malloc(pos.nbytes); ctx.to_device(d_v, pos)
    d_i = ctx.malloc(idx.nbytes); ctx.to_device(d_i, idx)
    d_s = ctx.malloc(sph.nbytes); ctx.to_device(d_s, sph)
    d_h = ctx.malloc(sph.shape[0])
    sc.intersect_spheres_mesh_device(d_s, sph.shape[0], tb.device_mesh(d_v, pos.shape[0], idx.shape[0], d_i), d_h)
    got = np.zeros(sph.shape[0], np.uint8); ctx.from_device(got, d_h)
    assert np.array_equal(got, want)
    for d in (d_v, d_i, d_s, d_h):
        ctx.free(d)
    sc.free()


def test_flatten_mesh_is_the_numpy_gather(ctx):
    pos, idx = bunny(8)
    pos = pos.copy(); pos[:, 3] = np.arange(pos.shape[0], dtype=np.float32)   # w travels at a 16-byte stride ...
    flat = flatten(pos, idx)
    out = np.zeros_like(flat)
    d = ctx.flatten_mesh(pos, idx); ctx.from_device(out, d)
    assert np.array_equal(out.view(np.uint32), flat.view(np.uint32))
    flat0 = flat.copy(); flat0[:, 3] = 0                                     # ... and is 0 at every other one
    for floats in (3, 5, 8):
        ctx.flatten_mesh(interleave(pos, floats), idx, d_out=d); ctx.from_device(out, d)
        assert np.array_equal(out.view(np.uint32), flat0.view(np.uint32)), floats
    ctx.flatten_mesh(flat, None, d_out=d); ctx.from_device(out, d)           # the flat form: a copy
    assert np.array_equal(out.view(np.uint32), flat.view(np.uint32))
    ctx.free(d)


def test_an_indexed_blas_under_a_tlas_next_to_a_flat_one(ctx):
    pos, idx = bunny(8)
    pos = pos.copy()
    lo, hi = pos[:, :3].min(0), pos[:, :3].max(0)
    pos[:, :3] = (pos[:, :3] - lo) / (hi - lo).max()                         # into the unit cube
    flat = flatten(pos, idx)
    other = scenes.soup(2000, seed=9, extent=1.0, size=0.2)
    xf = np.tile(np.eye(4, dtype=np.float32), (8, 1, 1))
    for k in range(8):
        xf[k, :3, 3] = [(k & 1) * 1.5, ((k >> 1) & 1) * 1.5, (k >> 2) * 1.5]
    rays = R.random_rays(100_000, (-0.5, -0.5, -0.5), (3.0, 3.0, 3.0), seed=6)
    got = []
    for indexed in (False, True):
        a = tb.BVH8_CWBVH(ctx).Build(pos, indices=idx, threads=1) if indexed else tb.BVH8_CWBVH(ctx).Build(flat, threads=1)
        b = tb.BVH8_CWBVH(ctx).Build(other, threads=1)
        inst = tb.make_instances(xf.reshape(8, 16), [0, 1, 0, 1, 1, 0, 1, 0])
        tlas = tb.TLAS(ctx).Build(inst, [a, b])
        got.append(tlas.Intersect(rays.copy()).view(np.uint8).reshape(-1, 64).copy())
        tlas.free(); a.free(); b.free()
    assert int((got[0].view(np.float32).reshape(-1, 16)[:, 12] < 1e30).sum()) > 5000
    assert np.array_equal(got[0], got[1])


# ---- a device-resident index buffer is checked by the kernels that read it ------------------------------------------------------------------

def test_an_out_of_range_device_index_is_reported_not_dereferenced(ctx):
    """An input check, and one that cannot fault even if it were missing: the vertex buffer is allocated LARGER than the n_verts the mesh declares,
    and the bad index lies beyond n_verts but inside the allocation."""
    pos, idx = bunny(8)
    extra = 64
    padded = np.concatenate([pos, np.zeros((extra, 4), np.float32)])
    bad = idx.copy()
    bad[1234, 2] = pos.shape[0] + 3                                          # >= n_verts (declared), < n_verts + extra (allocated)
    d_v = ctx.malloc(padded.nbytes); ctx.to_device(d_v, padded)
    d_i = ctx.malloc(bad.nbytes); ctx.to_device(d_i, bad)
    mesh = tb.device_mesh(d_v, pos.shape[0], idx.shape[0], d_i)
    # the host form of the same mesh is refused before anything is allocated, naming the triangle
    with pytest.raises(tb.TbvhError, match="triangle 1234"):
        tb.BVH8_CWBVH(ctx).BuildOnDevice(pos, indices=bad)
    # device form: the build reads the indices on the device and reports the bad one
    with pytest.raises(tb.TbvhError, match="vertex index"):
        tb.BVH8_CWBVH(ctx).BuildOnDevice(mesh)
    # an asynchronous call: the next synchronising call reports it
    good = tb.BVH8_CWBVH(ctx).Build(pos, indices=idx, threads=1)
    d_out = ctx.malloc(idx.shape[0] * 48)
    assert lib.tbvh_flatten_mesh_device(ctx._h, C.byref(mesh), C.c_void_p(d_out)) == 0
    rays = mixed_rays(flatten(pos, idx), 2048)
    with pytest.raises(tb.TbvhError, match="vertex index"):
        good.Intersect(rays.copy())
    want = good.Intersect(rays.copy())                                       # the status word is cleared: the context works on
    assert int((want["t"] < 1e30).sum()) > 100
    # refit through the bad buffer: reported, and the scene is usable again after a good refit
    with pytest.raises(tb.TbvhError, match="vertex index"):
        good.Refit(tb.device_mesh(d_v, pos.shape[0], idx.shape[0], d_i))
        good.Intersect(rays.copy())
    good.Refit(pos, mesh=True)                                               # the HELD indices: the bad buffer never replaced them
    assert np.array_equal(good.Intersect(rays.copy()).view(np.uint8), want.view(np.uint8))
    for d in (d_v, d_i, d_out):
        ctx.free(d)
    good.free()


def test_tiny_hip_indexed_binding_runs():
    """a tinybvh::BVH_GPU built over an index buffer (16- and 32-byte strides) uploaded as it is through tinyhip::Scene( gpu ), traced, refitted from
    the slice and sphere-queried from C++ (examples/indexed_mesh.cpp, built by __graft_entry__.build() where the reference header is found): the
    reference's own BVH::Intersect records before and after Refit(), within test_golden.py's tie budget; sphere flags equal to the flat call's"""
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "_build", "indexed_mesh")
    if not os.path.exists(exe):
        pytest.skip("examples/_build/indexed_mesh not built (needs the reference header at build time)")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, check=True).stdout.strip().split("\n")
    assert [l.split()[0] for l in out] == ["indexed", "stride32"], out
    for l in out:
        w = l.split()
        assert int(w[4]) == 4096 and int(w[2]) <= 2 and int(w[6]) <= 2, l        # rays differing before / after the refit
        assert int(w[8]) == 0 and int(w[10]) == 1024, l                            # sphere flags differing from the flat call
        assert int(w[12]) > 3500 and int(w[13]) > 3500 and 20 < int(w[15]) < 1000, l
