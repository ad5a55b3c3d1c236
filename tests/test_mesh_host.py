"""Indexed and strided triangle meshes on the host (tbvh_mesh; tbvh_host_build_mesh): the library's builder reads the triangles through
the index buffer and the vertex stride, and what it builds does not depend on the form — the blobs are the bytes tbvh_host_build gives
for the flattened triangles.  No GPU here; tests/test_mesh_gpu.py continues on the device."""
import ctypes as C
import os

import numpy as np
import pytest

import tinybvh_amd as tb
from tinybvh_amd import _capi, scenes
from tinybvh_amd import rays as R
import mesh_lib as ml
from mesh_lib import bunny, flatten, mesh_ref  # noqa: F401  (mesh_ref: the session fixture)
from native_build import syntax_check
from oracle_lib import compare_hits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = [tb.LAYOUT_BVH_GPU, tb.LAYOUT_BVH4_GPU, tb.LAYOUT_CWBVH]


def interleave(pos, stride_floats, junk=np.nan):
    """positions at the front of rows of stride_floats floats; whatever follows is junk that must never influence anything"""
    buf = np.full((pos.shape[0], stride_floats), junk, np.float32)
    buf[:, :3] = pos[:, :3]
    return buf[:, :3]   # a view: the row stride stays stride_floats * 4


MESHES = {
    "bunny8": lambda: bunny(8),
    "blob": lambda: scenes.weld(scenes.blob(4000, seed=3)),
    "atrium": lambda: scenes.weld(scenes.atrium(6000, seed=1)),
}


def all_blobs(h):
    return [h.blob(w, np.uint32, 1).copy() for w in range(4)]


def test_weld_is_the_inverse_of_flattening():
    v = scenes.blob(3000, seed=3)
    pos, idx = scenes.weld(v)
    assert pos.shape[0] < v.shape[0] // 2 and idx.shape == (v.shape[0] // 3, 3)
    assert np.array_equal(flatten(pos, idx).view(np.uint32), v.view(np.uint32))


@pytest.mark.parametrize("mesh", sorted(MESHES))
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("split", [0.0, 0.3], ids=["whole", "split"])
def test_indexed_build_is_byte_identical_to_the_flat_build(mesh, layout, split):
    pos, idx = MESHES[mesh]()
    flat = flatten(pos, idx)
    a = tb.HostBVH(flat, layout, threads=1, split_budget=split)
    b = tb.HostBVH(pos, layout, threads=1, split_budget=split, indices=idx)
    assert b.n_tris == idx.shape[0]
    for w, (x, y) in enumerate(zip(all_blobs(a), all_blobs(b))):
        assert x.size == y.size and np.array_equal(x, y), f"blob {w} differs"
    assert a.blob(0, np.uint32, 1).size > 0


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("stride_floats", [3, 5, 7, 8])
@pytest.mark.parametrize("split", [0.0, 0.3], ids=["whole", "split"])
def test_strided_build_is_byte_identical_to_the_flat_build(layout, stride_floats, split):
    """strides 12, 20, 28 and 32 bytes, with and without indices; NaN behind every position.  Only x, y, z are read at these strides, so the
    flat form it must equal has w = 0."""
    pos, idx = bunny(16)
    flat = flatten(pos, idx)
    assert not flat[:, 3].any()
    want = all_blobs(tb.HostBVH(flat, layout, threads=1, split_budget=split))
    got_indexed = all_blobs(tb.HostBVH(interleave(pos, stride_floats), layout, threads=1, split_budget=split, indices=idx))
    got_plain = all_blobs(tb.HostBVH(interleave(flat, stride_floats), layout, threads=1, split_budget=split))
    for w in range(4):
        assert np.array_equal(want[w], got_indexed[w]), f"indexed, blob {w}"
        assert np.array_equal(want[w], got_plain[w]), f"no indices, blob {w}"


def test_w_is_the_vertex_w_at_a_16_byte_stride():
    """bvhvec4 vertices: w travels into the records exactly as it does from the flat array (the wavefront tracer keeps materials there)"""
    pos, idx = bunny(32)
    pos = pos.copy()
    pos[:, 3] = np.arange(pos.shape[0], dtype=np.float32)
    for layout in (tb.LAYOUT_BVH4_GPU, tb.LAYOUT_CWBVH):
        a = tb.HostBVH(flatten(pos, idx), layout, threads=1, split_budget=0.0)
        b = tb.HostBVH(pos, layout, threads=1, split_budget=0.0, indices=idx)
        for x, y in zip(all_blobs(a), all_blobs(b)):
            assert np.array_equal(x, y)


# ---- validation: every error is a status code and a message, never an exit ----------------------------------------------------------

def _mesh(pos, idx, stride=16, n_verts=None, on_device=0, n_tris=None):
    return _capi.Mesh(C.c_void_p(pos.ctypes.data), pos.shape[0] if n_verts is None else n_verts, stride, on_device,
                      None if idx is None else C.c_void_p(idx.ctypes.data), (idx.shape[0] if idx is not None else pos.shape[0] // 3) if n_tris is None else n_tris)


def _build(mesh, layout=tb.LAYOUT_CWBVH):
    h = C.c_void_p()
    r = _capi.lib.tbvh_host_build_mesh(C.byref(mesh) if mesh is not None else None, layout, None, C.byref(h))
    msg = _capi.lib.tbvh_last_error() if r else b""
    if r == 0:
        _capi.lib.tbvh_host_free(h)
    return r, msg


def test_validation():
    pos, idx = bunny(64)
    assert _build(_mesh(pos, idx))[0] == 0
    assert _build(_mesh(pos, idx, stride=0))[0] == 0                      # 0 = 16
    r, msg = _build(None)
    assert r == -1 and b"mesh" in msg
    for bad in (4, 8, 10, 14, 18, 6):
        r, msg = _build(_mesh(pos, idx, stride=bad))
        assert r == -1 and b"stride" in msg, bad
    r, msg = _build(_mesh(pos, idx, on_device=1))
    assert r == -1 and b"host" in msg
    r, msg = _build(_mesh(pos, idx, n_verts=1 << 32))
    assert r == -1 and b"32-bit" in msg
    r, msg = _build(_mesh(pos, idx, n_tris=(1 << 32) // 3 + 1))
    assert r == -1 and b"32-bit" in msg
    r, msg = _build(_mesh(pos, idx, n_tris=0))
    assert r == -1
    r, msg = _build(_mesh(pos, None, n_tris=pos.shape[0] // 3 + 1))   # no indices: 3 n_tris vertices are needed
    assert r == -1 and b"without indices" in msg
    r, msg = _build(_mesh(pos, idx), layout=12345)
    assert r == -1 and b"layout" in msg
    bad = idx.copy()
    bad[7, 1] = pos.shape[0]                                              # the first index that is not a vertex
    bad[9, 0] = pos.shape[0] + 5
    r, msg = _build(_mesh(pos, bad))
    assert r == -5 and b"triangle 7" in msg and str(pos.shape[0]).encode() in msg
    # ... and the same index is fine once the mesh declares one more vertex
    pos2 = np.concatenate([pos, pos[:1]])
    bad[9, 0] = 0
    assert _build(_mesh(pos2, bad))[0] == 0
    h = C.c_void_p()
    assert _capi.lib.tbvh_host_build_mesh(C.byref(_mesh(pos, idx)), tb.LAYOUT_CWBVH, None, None) == -1


def test_python_keeps_the_flat_form_for_packed_arrays():
    """what was the flat form before still is: any packed array that reshapes to (3 n, 4) — only indices=, an (n, 3) array, a device_mesh() or a
    view whose rows are not packed select the mesh form"""
    v = scenes.blob(600, seed=3)
    a = tb.HostBVH(v, tb.LAYOUT_CWBVH, threads=1)
    for shaped in (v.reshape(-1, 12), v.reshape(-1), v.reshape(-1, 3, 4), v.reshape(-1, 8)):
        b = tb.HostBVH(shaped, tb.LAYOUT_CWBVH, threads=1)
        assert b.mesh is None and b.n_tris == a.n_tris
        assert np.array_equal(a.blob(0, np.uint32, 4), b.blob(0, np.uint32, 4))
    assert tb._is_mesh(v[:, :3]) and tb._is_mesh(np.ascontiguousarray(v[:, :3])) and tb._is_mesh(v, np.zeros(3, np.uint32)) and not tb._is_mesh(v)


def test_python_takes_the_stride_from_the_array():
    pos, idx = bunny(32)
    inter = np.full((pos.shape[0], 8), np.nan, np.float32)
    inter[:, :3] = pos[:, :3]
    view = inter[:, :3]
    m, keep = tb._mesh(view, idx)
    assert m.stride_bytes == 32 and keep[0].ctypes.data == inter.ctypes.data and m.n_verts == pos.shape[0] and m.n_tris == idx.shape[0]
    m, keep = tb._mesh(np.ascontiguousarray(pos[:, :3]), idx)
    assert m.stride_bytes == 12
    m, keep = tb._mesh(pos.astype(np.float64), idx)   # converted: a contiguous float32 copy
    assert m.stride_bytes == 16 and keep[0].dtype == np.float32


# ---- the real reference: its indexed path, and the committed goldens ---------------------------------------------------------------------

def golden():
    return np.load(os.path.join(ml.GOLDEN, "bunny_indexed.npz"))


def hit_fields(rec_bytes):
    return np.ascontiguousarray(rec_bytes).view(tb.RAY_DTYPE).reshape(-1)


def test_reference_results_do_not_depend_on_the_form(mesh_ref):
    """BVH::Build( verts, indices, n ), Build( slice( stride 32 ), indices, n ) and Build( flat, n ) of the real reference: identical nodes, identical
    Intersect / IsOccluded / IntersectSphere answers, and identical nodes and answers again after the shared vertices moved and Refit() ran."""
    g = golden()
    pos, idx, rays, sp = g["positions"], g["indices"], hit_fields(g["rays"]), g["spheres"]
    ok = g["sphere_answers"] != 255
    forms = {"indexed": (lambda p: p, idx), "stride32": (lambda p: ml.stride32(p), idx), "flat": (lambda p: flatten(p, idx), None)}
    got = {}
    for name, (layout, i) in forms.items():
        h = mesh_ref.build(layout(pos), i)
        r = [mesh_ref.blob(h, 0), mesh_ref.blob(h, 1), mesh_ref.blob(h, 2), mesh_ref.intersect(h, rays).view(np.uint8), mesh_ref.occluded(h, rays),
             mesh_ref.spheres(h, sp[ok])]
        mesh_ref.refit(h, layout(g["positions_refit"]))
        ok2 = g["sphere_answers_refit"] != 255
        r += [mesh_ref.blob(h, 0), mesh_ref.blob(h, 2), mesh_ref.intersect(h, rays).view(np.uint8), mesh_ref.occluded(h, rays), mesh_ref.spheres(h, sp[ok2])]
        mesh_ref.free(h)
        got[name] = r
    for name in ("stride32", "flat"):
        for k, (x, y) in enumerate(zip(got["indexed"], got[name])):
            assert np.array_equal(x, y), f"{name}: item {k} differs from the indexed build's"
    assert int((hit_fields(got["indexed"][3])["t"] < 1e30).sum()) > 300 and int(got["indexed"][5].sum()) > 300


def test_committed_goldens_are_what_the_reference_gives_today(mesh_ref, tmp_path):
    import sphere_lib as sl
    sys_path_tools = os.path.join(ROOT, "tools")
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_mesh_golden", os.path.join(sys_path_tools, "make_mesh_golden.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    now = mod.make(mesh_ref, sl.compile_oracle(tmp_path))
    g = golden()
    assert sorted(g.files) == sorted(now)
    for k in g.files:
        assert np.array_equal(np.asarray(now[k]).view(np.uint8), g[k].view(np.uint8)), k


@pytest.mark.parametrize("tag", ["", "_refit"])
def test_the_oracle_reproduces_the_goldens_bit_for_bit(oracle_ref, tag):
    """the restated BVH::Intersect / IsOccluded (reference tie rule) over the golden's Wald nodes and the FLATTENED triangles: 0 differing records of
    all rays — the chosen rays are clean inputs, checked on the CPU before any GPU time is spent"""
    g = golden()
    flat = flatten(g["positions_refit"] if tag else g["positions"], g["indices"])
    rays, want = hit_fields(g["rays"]), hit_fields(g["hits" + tag])
    got = oracle_ref.bvh2_intersect(g["wald_nodes" + tag], g["prim_idx" + tag], flat, rays)
    diff = int((got.view(np.uint8).reshape(-1, 64) != want.view(np.uint8).reshape(-1, 64)).any(1).sum())
    assert diff == 0, f"{diff} of {rays.shape[0]} records differ"
    assert np.array_equal(oracle_ref.bvh2_occluded(g["wald_nodes" + tag], g["prim_idx" + tag], flat, rays), g["occluded" + tag])


@pytest.mark.parametrize("tag", ["", "_refit"])
def test_the_library_builder_over_the_indexed_mesh_gives_the_golden_hits(oracle_ref, tag):
    """the library's own BVH2 built THROUGH the index buffer, traced by the restatement: the reference's records for its indexed build"""
    g = golden()
    pos = g["positions_refit"] if tag else g["positions"]
    h = tb.HostBVH(pos, tb.LAYOUT_BVH2_WALD, threads=1, indices=g["indices"])
    got = oracle_ref.bvh2_intersect(h.bvh2_nodes(), h.bvh2_prim_idx(), flatten(pos, g["indices"]), hit_fields(g["rays"]))
    c = compare_hits(got, hit_fields(g["hits" + tag]))
    assert c["hitmiss"] == 0 and c["prim_real"] == 0 and c["t_bad"] == 0 and c["uv_bad"] == 0 and c["tie"] <= 1, c
    assert c["bit_identical"] == c["same_prim"], c


def test_tiny_hip_indexed_binding_compiles(tmp_path):
    """tinyhip::Scene( const BVH_GPU& ), Refit( const bvhvec4slice& ) and IntersectSpheres( .., const bvhvec4slice&, .. ) against the real tiny_bvh.h
    (examples/indexed_mesh.cpp; the program build() makes of it runs on the GPU in tests/test_mesh_gpu.py), and the existing hosts still compile"""
    for name in ("indexed_mesh", "speedtest_gpu_section", "sphere_bvh"):
        syntax_check(tmp_path, '#include "%s"\n' % os.path.join(ROOT, "examples", name + ".cpp"))
