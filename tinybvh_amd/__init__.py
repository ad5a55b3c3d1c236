"""tinybvh_amd — MI355X-native batched ray traversal behind tinybvh's GPU-layout API.

Thin Python mirror of the reference's host interface for this one path (class and method
names follow tiny_bvh.h: ``BVH_GPU`` / ``BVH4_GPU`` / ``BVH8_CWBVH`` with ``Build``,
``Intersect``, ``IsOccluded``), over the C ABI in ``include/tinybvh_amd.h``.  All compute
is in the HIP library; this package holds no traversal code and no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import os

import numpy as np

from . import _capi
from ._capi import AlphaTexture, BuildParams, Camera, Mesh, OmmSource, TbvhError, check, lib

LAYOUT_BVH2_WALD = 1
LAYOUT_BVH_DOUBLE = 3
LAYOUT_BVH_GPU = 5
LAYOUT_BVH4_GPU = 8
LAYOUT_CWBVH = 10
TRITEST_MOLLER_TRUMBORE, TRITEST_WATERTIGHT = 0, 1   # TBVH_TRITEST_* (tbvh_set_triangle_test)
LAYOUT_VOXELSET = 12
# wavefront materials: v0.w of a triangle's first vertex = type << 24 | 0xRRGGBB (wavefront.cl:12-13, 160)
MATERIAL_DIFFUSE, MATERIAL_LIGHT, MATERIAL_SPECULAR = 0, 1, 2

BVH_FAR = np.float32(1e30)

# first 64 bytes of tinybvh::Ray (tiny_bvh.h:689-709) == device struct Ray (traverse.cl:11-17)
RAY_DTYPE = np.dtype([
    ("O", "<f4", 3), ("mask", "<u4"),
    ("D", "<f4", 3), ("instIdx", "<u4"),
    ("rD", "<f4", 3), ("inst", "<u4"),
    ("t", "<f4"), ("u", "<f4"), ("v", "<f4"), ("prim", "<u4"),
])
assert RAY_DTYPE.itemsize == 64
# what rides beside a ray in the path tracer's queues (kernels.h: PathAux): throughput + pixel << 8 | depth << 4 | flags, or contribution + pixel
PATH_AUX_DTYPE = np.dtype([("T", "<f4", 3), ("pixel", "<u4")])


def safercp(x: np.ndarray) -> np.ndarray:
    """tinybvh_safercp (tiny_bvh.h:442): 1/x, or +-1e30 when |x| <= 1e-12."""
    x = np.asarray(x, dtype=np.float32)
    big = np.abs(x) > np.float32(1e-12)
    with np.errstate(divide="ignore"):
        r = np.where(big, np.float32(1.0) / np.where(big, x, np.float32(1.0)), np.where(x >= 0, BVH_FAR, -BVH_FAR))
    return r.astype(np.float32)


def make_rays(O: np.ndarray, D: np.ndarray, tmax=BVH_FAR, normalize: bool = True) -> np.ndarray:
    """Build ray records the way the tinybvh::Ray constructor does (tiny_bvh.h:695-703)."""
    O = np.ascontiguousarray(O, dtype=np.float32).reshape(-1, 3)
    D = np.ascontiguousarray(D, dtype=np.float32).reshape(-1, 3)
    if normalize:
        l = np.sqrt((D * D).sum(axis=1, dtype=np.float32)).astype(np.float32)
        rl = np.where(l == 0, np.float32(0), np.float32(1) / np.where(l == 0, np.float32(1), l)).astype(np.float32)
        D = (D * rl[:, None]).astype(np.float32)
    rays = np.zeros(O.shape[0], dtype=RAY_DTYPE)
    rays["O"] = O
    rays["D"] = D
    rays["rD"] = safercp(D)
    rays["mask"] = 0xFFFF
    rays["t"] = tmax
    return rays


def _ptr(a: np.ndarray) -> C.c_void_p:
    return C.c_void_p(a.ctypes.data)


class Context:
    """One HIP device (replaces tinyocl's process-global InitCL, tiny_ocl.h:945-1139)."""

    def __init__(self, device: int = 0):
        h = C.c_void_p()
        check(lib.tbvh_init(device, C.byref(h)), "tbvh_init")
        self._h = h
        self.device = device

    def close(self):
        if self._h:
            lib.tbvh_shutdown(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        check(lib.tbvh_synchronize(self._h), "tbvh_synchronize")

    def set_stream(self, hip_stream: Optional[int]):
        check(lib.tbvh_set_stream(self._h, C.c_void_p(hip_stream or 0)), "tbvh_set_stream")

    def set_overlap(self, enabled: bool):
        """Independent device-resident queries overlap within this context (tbvh_context_set_overlap; default on, TBVH_OVERLAP=0 turns it off)."""
        check(lib.tbvh_context_set_overlap(self._h, 1 if enabled else 0), "tbvh_context_set_overlap")

    def overlap_stats(self):
        """(query launches that took the second lane, joins taken) since the context was made (tbvh_debug_overlap_stats)."""
        out = (C.c_uint64 * 2)()
        check(lib.tbvh_debug_overlap_stats(self._h, out), "tbvh_debug_overlap_stats")
        return int(out[0]), int(out[1])

    def set_overlap_depth(self, depth: int):
        """How many launches one lane may start ahead of the other: 1 or 2 (tbvh_debug_set_overlap_depth; default 1, TBVH_OVERLAP_DEPTH)."""
        check(lib.tbvh_debug_set_overlap_depth(self._h, int(depth)), "tbvh_debug_set_overlap_depth")

    def set_probe_memory(self, enabled: bool):
        """Remember the coherence probe's verdicts per buffer and launch incoherent batches as one kernel (tbvh_debug_set_probe_memory; default on, TBVH_PROBE_MEMORY=0)."""
        check(lib.tbvh_debug_set_probe_memory(self._h, 1 if enabled else 0), "tbvh_debug_set_probe_memory")

    def probe_memory_stats(self):
        """(launches that left out the coherent flavor, verdicts read back) since the context was made (tbvh_debug_probe_memory_stats)."""
        out = (C.c_uint64 * 2)()
        check(lib.tbvh_debug_probe_memory_stats(self._h, out), "tbvh_debug_probe_memory_stats")
        return int(out[0]), int(out[1])

    def set_timing(self, enabled: bool):
        """Per-operation HIP-event timing on / off (tbvh_set_timing): off saves two event records per query."""
        check(lib.tbvh_set_timing(self._h, 1 if enabled else 0), "tbvh_set_timing")

    def copy_bandwidth_gbps(self, nbytes: int = 1 << 30, reps: int = 3) -> float:
        """Measured streaming-copy bandwidth of this device (tbvh_measure_copy_bandwidth), GB/s read + written."""
        g = C.c_double(0)
        check(lib.tbvh_measure_copy_bandwidth(self._h, nbytes, reps, C.byref(g)), "tbvh_measure_copy_bandwidth")
        return float(g.value)

    def read_bandwidth_gbps(self, nbytes: int = 1 << 30, reps: int = 3) -> float:
        """Measured read-only streaming bandwidth of this device (tbvh_measure_read_bandwidth), GB/s."""
        g = C.c_double(0)
        check(lib.tbvh_measure_read_bandwidth(self._h, nbytes, reps, C.byref(g)), "tbvh_measure_read_bandwidth")
        return float(g.value)

    def valu_issue_ginstr(self, reps: int = 3) -> float:
        """Measured VALU issue ceiling (1e9 wave64 instructions per second, whole chip) for the CWBVH node test's mix (tbvh_measure_valu_issue)."""
        g = C.c_double(0)
        check(lib.tbvh_measure_valu_issue(self._h, reps, C.byref(g)), "tbvh_measure_valu_issue")
        return float(g.value)

    def link_bandwidth_gbps(self, nbytes: int = 1 << 28, reps: int = 3):
        """Measured host link rates (tbvh_measure_link_bandwidth): (host-to-device, device-to-host) GB/s of a pinned hipMemcpyAsync."""
        up, down = C.c_double(0), C.c_double(0)
        check(lib.tbvh_measure_link_bandwidth(self._h, nbytes, reps, C.byref(up), C.byref(down)), "tbvh_measure_link_bandwidth")
        return float(up.value), float(down.value)

    def pinned_array(self, shape, dtype) -> np.ndarray:
        """A numpy array in page-locked host memory of the library's (tbvh_pinned_malloc): a packed RAY_DTYPE array that lives there goes up by DMA
        without the packing pass.  Give it back with pinned_free(array) (or it goes with the context)."""
        dt = np.dtype(dtype)
        n = int(np.prod(shape)) * dt.itemsize
        p = C.c_void_p()
        check(lib.tbvh_pinned_malloc(self._h, max(n, 1), C.byref(p)), "tbvh_pinned_malloc")
        buf = (C.c_char * max(n, 1)).from_address(p.value)
        a = np.frombuffer(buf, dtype=dt, count=int(np.prod(shape))).reshape(shape)
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[a.ctypes.data] = p.value
        return a

    def pinned_free(self, a: np.ndarray):
        p = getattr(self, "_pinned", {}).pop(a.ctypes.data, None)
        check(lib.tbvh_pinned_free(self._h, C.c_void_p(p if p is not None else a.ctypes.data)), "tbvh_pinned_free")

    def time_last_ms(self) -> float:
        return float(lib.tbvh_time_last_ms(self._h))

    def time_history(self, k: int):
        """HIP-event durations (ms) of the last k timed operations on this context, oldest first (tbvh_time_history): what a
        caller that enqueues its launches back to back reads ONCE instead of synchronizing after every launch."""
        buf = (C.c_float * max(int(k), 1))()
        cnt = C.c_uint32(0)
        check(lib.tbvh_time_history(self._h, buf, int(k), C.byref(cnt)), "tbvh_time_history")
        return [float(buf[i]) for i in range(cnt.value)]

    def set_debug_flags(self, flags: int):
        check(lib.tbvh_debug_set_flags(self._h, int(flags)), "tbvh_debug_set_flags")

    def last_probe(self):
        """(agreeing pairs, pairs, verdict) of the coherence probe of the most recent query: verdict 0 = no probe ran,
        1 = incoherent (strict schedule), 2 = coherent (tbvh_debug_last_probe)."""
        out = (C.c_uint32 * 3)()
        check(lib.tbvh_debug_last_probe(self._h, out), "tbvh_debug_last_probe")
        return int(out[0]), int(out[1]), int(out[2])

    # device buffers (replace tinyocl::Buffer for resident rays)
    def malloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        check(lib.tbvh_device_malloc(self._h, nbytes, C.byref(p)), "tbvh_device_malloc")
        return p.value

    def free(self, dptr: int):
        check(lib.tbvh_device_free(self._h, C.c_void_p(dptr)), "tbvh_device_free")

    def to_device(self, dptr: int, a: np.ndarray):
        a = np.ascontiguousarray(a)
        check(lib.tbvh_copy_to_device(self._h, C.c_void_p(dptr), _ptr(a), a.nbytes), "tbvh_copy_to_device")

    def from_device(self, a: np.ndarray, dptr: int):
        assert a.flags["C_CONTIGUOUS"]
        check(lib.tbvh_copy_from_device(self._h, _ptr(a), C.c_void_p(dptr), a.nbytes), "tbvh_copy_from_device")

    def flatten_mesh(self, verts, indices=None, d_out: int = 0) -> int:
        """tbvh_flatten_mesh_device: 3 float4 per triangle on the device (for generate_bounce / Wavefront.render, which stay flat-only).
        Returns the device pointer (allocated here with malloc() unless d_out is given)."""
        m, keep = _mesh(verts, indices)
        d = d_out or self.malloc(int(m.n_tris) * 48)
        check(lib.tbvh_flatten_mesh_device(self._h, C.byref(m), C.c_void_p(d)), "tbvh_flatten_mesh_device")
        return d

    def reset_hits(self, d_rays: int, n: int, tmax: float = 1e30):
        check(lib.tbvh_reset_hits_device(self._h, C.c_void_p(d_rays), n, float(tmax)), "tbvh_reset_hits_device")

    # ray generators
    def generate_primary(self, cam: Camera, d_rays: int, first: int, n: int):
        check(lib.tbvh_generate_primary_device(self._h, C.byref(cam), C.c_void_p(d_rays), first, n), "tbvh_generate_primary_device")

    def generate_bounce(self, d_verts: int, d_in: int, d_out: int, n: int, seed: int):
        check(lib.tbvh_generate_bounce_device(self._h, C.c_void_p(d_verts), C.c_void_p(d_in), C.c_void_p(d_out), n, seed), "tbvh_generate_bounce_device")

    def bin_rays(self, d_in: int, d_out: int, n: int, bounds6, cell_bits: int = 5, flags: int = 1, d_perm: int = 0):
        """Counting sort of a resident batch by (Morton code of the origin's cell, direction octant): tbvh_bin_rays_device."""
        b = (C.c_float * 6)(*[float(x) for x in bounds6])
        check(lib.tbvh_bin_rays_device(self._h, C.c_void_p(d_in), C.c_void_p(d_out), n, b, cell_bits, flags, C.c_void_p(d_perm or 0)), "tbvh_bin_rays_device")

    def generate_shadow(self, d_in: int, d_out: int, n: int, light, eps: float):
        l = (C.c_float * 3)(*[float(x) for x in light])
        check(lib.tbvh_generate_shadow_device(self._h, C.c_void_p(d_in), C.c_void_p(d_out), n, l, float(eps)), "tbvh_generate_shadow_device")


_DEVICE_BUILDERS = {"lbvh": 0, "ploc": 1, "sah": 2}   # tbvh_build_device_mesh's builder argument
_SBVH = "sbvh"                                        # the reference's BuildHQ tree: entry points of its own (tbvh_build_device_sbvh, _mesh)


def _device_builder(builder: str):
    """validates the name; the code tbvh_build_device_mesh takes for it (None for the SBVH, which that entry point does not build)"""
    if builder == _SBVH:
        return None
    if builder not in _DEVICE_BUILDERS:
        raise ValueError(f"BuildOnDevice: builder {builder!r} (one of {', '.join(sorted(list(_DEVICE_BUILDERS) + [_SBVH]))})")
    return _DEVICE_BUILDERS[builder]


def device_mesh(d_verts: int, n_verts: int, n_tris: int, d_indices: int = 0, stride_bytes: int = 16) -> Mesh:
    """A tbvh_mesh whose vertices (and indices, if any) are device memory: pass it wherever `verts` is taken together with indices=."""
    return Mesh(C.c_void_p(int(d_verts)), int(n_verts), int(stride_bytes), 1, C.c_void_p(int(d_indices)) if d_indices else None, int(n_tris))


def _is_mesh(verts, indices=None) -> bool:
    """Does (verts, indices) name the mesh form?  Yes with indices=, for a device_mesh(), for an (n, 3) array, and for a 2-D float32 view whose rows
    are not packed (interleaved[:, :3]: the row stride says where the vertices are).  Everything else — any packed array that reshapes to (3 n, 4),
    as before — is the flat form."""
    if indices is not None or isinstance(verts, Mesh):
        return True
    if not isinstance(verts, np.ndarray) or verts.ndim != 2:
        return False
    return verts.shape[1] == 3 or (verts.dtype == np.float32 and verts.shape[1] >= 3 and verts.strides[1] == 4 and verts.strides[0] != verts.shape[1] * 4)


def _mesh(verts, indices=None):
    """(tbvh_mesh, the arrays it points into) for a host mesh: verts any float32 array of shape (n_verts, k >= 3) whose row stride is a
    multiple of 4 — the stride is ndarray.strides[0], so interleaved[:, :3] is used in place —, indices (n_tris, 3) or flat uint32, or None
    (triangle i = vertices 3i, 3i + 1, 3i + 2).  A 16-byte row stride is a bvhvec4 array (w is read); any other stride reads x, y, z only.
    A Mesh made by device_mesh() passes through."""
    if isinstance(verts, Mesh):
        assert indices is None, "a device_mesh() carries its own indices"
        return verts, ()
    v = np.asarray(verts)
    if v.dtype != np.float32 or v.ndim != 2 or v.shape[1] < 3 or v.strides[1] != 4 or v.strides[0] % 4 or v.strides[0] < 12:
        v = np.ascontiguousarray(v, np.float32)
        assert v.ndim == 2 and v.shape[1] >= 3, "verts: (n_verts, k >= 3) float32"
    idx = None
    if indices is not None:
        idx = np.ascontiguousarray(indices, np.uint32).reshape(-1)
        assert idx.size % 3 == 0
        n_tris = idx.size // 3
    else:
        assert v.shape[0] % 3 == 0
        n_tris = v.shape[0] // 3
    m = Mesh(C.c_void_p(v.ctypes.data), v.shape[0], v.strides[0], 0, None if idx is None else C.c_void_p(idx.ctypes.data), n_tris)
    return m, (v, idx)


def host_build_bvh2_sah(verts, indices=None, max_leaf_tris: int = 0):
    """The reference's binned-SAH tree (BVH::Build, non-threaded numbering) by the library's sequential CPU twin (tbvh_host_build_bvh2_sah):
    (nodes32 (n, 8) uint32, prim_idx (n_tris,) uint32), every leaf's primitives ascending; max_leaf_tris > 0 = BVH::SplitLeafs afterwards."""
    m, keep = _mesh(verts, indices)
    nodes = np.zeros((max(2 * int(m.n_tris), 2), 8), np.uint32)
    idx = np.zeros(int(m.n_tris), np.uint32)
    n = C.c_uint64(0)
    check(lib.tbvh_host_build_bvh2_sah(C.byref(m), int(max_leaf_tris), _ptr(nodes), nodes.shape[0], _ptr(idx), idx.size, C.byref(n)), "tbvh_host_build_bvh2_sah")
    return nodes[:n.value].copy(), idx


def build_bvh2_sah(ctx, verts, indices=None, max_leaf_tris: int = 0):
    """The same tree built on the device (tbvh_build_bvh2_sah_device) and read back: byte for byte what host_build_bvh2_sah gives."""
    m, keep = _mesh(verts, indices)
    nodes = np.zeros((max(2 * int(m.n_tris), 2), 8), np.uint32)
    idx = np.zeros(int(m.n_tris), np.uint32)
    n = C.c_uint64(0)
    check(lib.tbvh_build_bvh2_sah_device(ctx._h, C.byref(m), int(max_leaf_tris), _ptr(nodes), nodes.shape[0], _ptr(idx), idx.size, 0, C.byref(n)),
          "tbvh_build_bvh2_sah_device")
    return nodes[:n.value].copy(), idx


def _boxes_arg(aabbs):
    """BVH::BuildAABB's layout from (n, 2, 4), (2 n, 4) or (n, 8) float32: box i = min at float4 2 i, max at 2 i + 1 (w ignored)"""
    a = np.ascontiguousarray(aabbs, np.float32)
    assert a.size % 8 == 0 and a.size > 0, "aabbs: n x {min float4, max float4}"
    return a.reshape(-1, 8)


def _sah_box_call(fn, name, head, n, max_leaf, width=8):
    nodes = np.zeros((max(2 * n, 2), width), np.uint32)
    idx = np.zeros(n, np.uint32)
    nn = C.c_uint64(0)
    check(fn(*head, n, *max_leaf, _ptr(nodes), nodes.shape[0], _ptr(idx), idx.size, C.byref(nn)), name)
    return nodes[:nn.value].copy(), idx


def host_build_bvh2_sah_boxes(aabbs, max_leaf: int = 0):
    """The reference's BVH::BuildAABB tree over boxes by the sequential CPU twin (tbvh_host_build_bvh2_sah_aabbs): (nodes32 (n, 8) uint32, prim_idx)."""
    a = _boxes_arg(aabbs)
    return _sah_box_call(lib.tbvh_host_build_bvh2_sah_aabbs, "tbvh_host_build_bvh2_sah_aabbs", (_ptr(a),), a.shape[0], (int(max_leaf),))


def host_build_bvh2_sah_spheres(spheres, max_leaf: int = 0):
    """The reference's BVH::Build( customGetAABB, n ) tree over spheres {x, y, z, r} (boxes pos -/+ r) by the CPU twin (tbvh_host_build_bvh2_sah_spheres)."""
    a = np.ascontiguousarray(spheres, np.float32).reshape(-1, 4)
    return _sah_box_call(lib.tbvh_host_build_bvh2_sah_spheres, "tbvh_host_build_bvh2_sah_spheres", (_ptr(a),), a.shape[0], (int(max_leaf),))


def host_build_tlas_sah(instances192):
    """The reference's TLAS over 192-byte instance records already updated (tbvh_host_build_tlas_sah): BVH::Build( BLASInstance*, n, 0, 0 ), then
    BVH_GPU::ConvertFrom: (nodes64 (n, 16) uint32 Aila-Laine nodes, instance indices with every leaf's ascending)."""
    a = np.ascontiguousarray(instances192).view(np.uint8).reshape(-1, 192)
    return _sah_box_call(lib.tbvh_host_build_tlas_sah, "tbvh_host_build_tlas_sah", (_ptr(a),), a.shape[0], (), width=16)


def build_bvh2_sah_boxes(ctx, aabbs, max_leaf: int = 0):
    """The BVH::BuildAABB tree built on the device (tbvh_build_bvh2_sah_device_aabbs) and read back: byte for byte what host_build_bvh2_sah_boxes gives.
    aabbs: a numpy array, or a (device_pointer, n) pair."""
    if isinstance(aabbs, tuple):
        ptr, n, on_device, a = C.c_void_p(int(aabbs[0])), int(aabbs[1]), 1, None
    else:
        a = _boxes_arg(aabbs)
        ptr, n, on_device = _ptr(a), a.shape[0], 0
    nodes = np.zeros((max(2 * n, 2), 8), np.uint32)
    idx = np.zeros(n, np.uint32)
    nn = C.c_uint64(0)
    check(lib.tbvh_build_bvh2_sah_device_aabbs(ctx._h, ptr, n, on_device, int(max_leaf), _ptr(nodes), nodes.shape[0], _ptr(idx), idx.size, 0, C.byref(nn)),
          "tbvh_build_bvh2_sah_device_aabbs")
    return nodes[:nn.value].copy(), idx


SBVH_STATS = ("n_refs", "n_spatial_splits", "n_unsplit_left", "n_unsplit_right", "n_fragment_splits", "n_one_sided_splits", "n_clipped_reclips",
              "n_budget_refusals", "n_failed_partitions")   # tbvh_sbvh_stats, field for field


def _sbvh_result(nodes, idx, n, m, st, stats):
    out = (nodes[:n.value].copy(), idx[:m.value].copy())
    return out + (dict(zip(SBVH_STATS, (int(x) for x in st))),) if stats else out


def host_build_bvh2_sbvh(verts, indices=None, max_leaf_tris: int = 0, stats: bool = False):
    """The reference's SBVH (BVH::BuildHQ after its Compact) by the library's sequential CPU twin (tbvh_host_build_bvh2_sbvh): (nodes32 (n, 8) uint32,
    prim_idx uint32: the references the leaves hold, in the reference's order), and with stats=True a dict of tbvh_sbvh_stats as a third item."""
    m, keep = _mesh(verts, indices)
    nodes = np.zeros((3 * int(m.n_tris) + 2, 8), np.uint32)
    idx = np.zeros(int(m.n_tris) + int(m.n_tris) // 2 + 1, np.uint32)
    n, k, st = C.c_uint64(0), C.c_uint64(0), (C.c_uint64 * len(SBVH_STATS))()
    check(lib.tbvh_host_build_bvh2_sbvh(C.byref(m), int(max_leaf_tris), _ptr(nodes), nodes.shape[0], _ptr(idx), idx.size, C.byref(n), C.byref(k), st),
          "tbvh_host_build_bvh2_sbvh")
    return _sbvh_result(nodes, idx, n, k, st, stats)


def build_bvh2_sbvh(ctx, verts, indices=None, max_leaf_tris: int = 0, stats: bool = False):
    """The same tree built on the device (tbvh_build_bvh2_sbvh_device) and read back: byte for byte what host_build_bvh2_sbvh gives."""
    m, keep = _mesh(verts, indices)
    nodes = np.zeros((3 * int(m.n_tris) + 2, 8), np.uint32)
    idx = np.zeros(int(m.n_tris) + int(m.n_tris) // 2 + 1, np.uint32)
    n, k, st = C.c_uint64(0), C.c_uint64(0), (C.c_uint64 * len(SBVH_STATS))()
    check(lib.tbvh_build_bvh2_sbvh_device(ctx._h, C.byref(m), int(max_leaf_tris), _ptr(nodes), nodes.shape[0], _ptr(idx), idx.size, 0, C.byref(n), C.byref(k), st),
          "tbvh_build_bvh2_sbvh_device")
    return _sbvh_result(nodes, idx, n, k, st, stats)


class HostBVH:
    """Blobs built on the host by the library's own builder (tbvh_host_build; with indices=, or a vertex array that is not (3 n, 4):
    tbvh_host_build_mesh — the same blobs, byte for byte, as for the flattened triangles)."""

    def __init__(self, verts: np.ndarray, layout: int, bins: int = 0, max_leaf_tris: int = 0, threads: int = 0,
                 optimal_collapse: bool = False, c_prim: float = 0.0, greedy_collapse: bool = False, split_budget: Optional[float] = None,
                 indices=None):
        self.indices = None
        self.mesh = None
        if not _is_mesh(verts, indices):
            verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 4)
            assert verts.shape[0] % 3 == 0
            self.n_tris = verts.shape[0] // 3
        else:   # an indexed and / or strided mesh
            self.mesh, keep = _mesh(verts, indices)
            verts, self.indices = keep if keep else (None, None)   # (a device_mesh(): the library answers that the host builder reads host memory)
            self.n_tris = int(self.mesh.n_tris)
        self.verts = verts
        self.layout = layout
        flags = (2 if optimal_collapse else 0) | (4 if greedy_collapse else 0) | (int(round(c_prim * 100)) << 8)
        if split_budget is not None:   # None: the layout's default (BVH8_CWBVH: 30 % extra references; the others: whole triangles)
            if split_budget > 0:       # TBVH_BUILD_SPLIT_TRIANGLES, budget in per cent of the triangle count
                flags |= 8 | (min(max(int(round(split_budget * 100)), 1), 255) << 24)
            else:
                flags |= 16            # TBVH_BUILD_WHOLE_TRIANGLES
        bp = BuildParams(bins, max_leaf_tris, threads, flags)
        h = C.c_void_p()
        if self.mesh is not None:
            check(lib.tbvh_host_build_mesh(C.byref(self.mesh), layout, C.byref(bp), C.byref(h)), "tbvh_host_build_mesh")
        else:
            check(lib.tbvh_host_build(_ptr(verts), self.n_tris, layout, C.byref(bp), C.byref(h)), "tbvh_host_build")
        self._h = h

    @classmethod
    def from_cwbvh_file(cls, path: str, expected_tris: int = 0) -> "HostBVH":
        """The blobs of a BVH8_CWBVH::Save file (tbvh_cwbvh_file_read); no BVH2 and no vertices come with it."""
        self = cls.__new__(cls)
        h = C.c_void_p(); n = C.c_uint64(0)
        self._h = None
        check(lib.tbvh_cwbvh_file_read(os.fsencode(path), expected_tris, C.byref(h), C.byref(n)), "tbvh_cwbvh_file_read")
        self._h = h
        self.verts = None
        self.n_tris = int(n.value)
        self.layout = LAYOUT_CWBVH
        return self

    def save_cwbvh(self, path: str) -> None:
        """Write this BVH8_CWBVH's blobs as a file BVH8_CWBVH::Load accepts (tbvh_cwbvh_file_write; tiny_bvh.h:5786-5795)."""
        assert self.layout == LAYOUT_CWBVH
        nodes, tris = self.blob(0, np.uint32, 4), self.blob(1, np.uint32, 4)
        check(lib.tbvh_cwbvh_file_write(os.fsencode(path), _ptr(nodes), nodes.shape[0], _ptr(tris), tris.shape[0], self.n_tris or tris.shape[0] // 3, None), "tbvh_cwbvh_file_write")

    def blob(self, which: int, dtype, width: int) -> np.ndarray:
        """Zero-copy numpy view of blob `which` (the view keeps this object alive)."""
        p = lib.tbvh_host_blob(self._h, which)
        n = lib.tbvh_host_blob_count(self._h, which)
        if not p or n == 0:
            return np.zeros((0, width), dtype=dtype)
        nbytes = n * np.dtype(dtype).itemsize * width
        buf = (C.c_char * nbytes).from_address(p)
        buf._owner = self   # the view keeps this object (and so the native blob) alive
        a = np.frombuffer(buf, dtype=dtype).reshape(n, width)
        a.flags.writeable = False
        return a

    # the Wald BVH2 every layout was encoded from (for the oracle)
    def bvh2_nodes(self) -> np.ndarray:
        return self.blob(0 if self.layout == LAYOUT_BVH2_WALD else 2, np.uint32, 8)

    def bvh2_prim_idx(self) -> np.ndarray:
        return self.blob(1 if self.layout in (LAYOUT_BVH2_WALD, LAYOUT_BVH_GPU) else 3, np.uint32, 1).reshape(-1)

    def __del__(self):
        try:
            if self._h:
                lib.tbvh_host_free(self._h)
                self._h = None
        except Exception:
            pass


class _Scene:
    """An uploaded layout.  Intersect / IsOccluded mirror X::Intersect(Ray&) /
    X::IsOccluded(const Ray&) of the reference, but over whole ray arrays."""

    layout = 0

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self._h = C.c_void_p()

    def free(self):
        if self._h and self.ctx._h:
            lib.tbvh_free_scene(self._h)
        self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    @property
    def device_bytes(self) -> int:
        return int(lib.tbvh_scene_device_bytes(self._h))

    def debug_bytes(self) -> list:
        """device_bytes term by term (tbvh_debug_scene_bytes; the eight words are include/tinybvh_amd_debug.h's): words 0 to 6 sum to device_bytes,
        word 7 is what the scene holds and does not count."""
        out = np.zeros(8, np.uint64)
        check(lib.tbvh_debug_scene_bytes(self._h, _ptr(out)), "tbvh_debug_scene_bytes")
        return [int(x) for x in out]

    def _build_mesh(self, layout: int, verts, indices, kw) -> "_Scene":
        """Build over an indexed / strided mesh on the host and upload (tbvh_host_build_mesh + tbvh_upload_host_mesh)."""
        self.host = HostBVH(verts, layout, indices=indices, **kw)
        check(lib.tbvh_upload_host_mesh(self.ctx._h, self.host._h, C.byref(self.host.mesh), C.byref(self._h)), "tbvh_upload_host_mesh")
        self._mesh_tris = int(self.host.mesh.n_tris)
        return self

    def _build_device_mesh(self, layout: int, verts, indices, max_leaf_tris: int, builder: str, radius: int) -> "_Scene":
        m, keep = _mesh(verts, indices)
        if builder == _SBVH:
            check(lib.tbvh_build_device_sbvh_mesh(self.ctx._h, C.byref(m), layout, max_leaf_tris, C.byref(self._h)), "tbvh_build_device_sbvh_mesh")
            self._mesh_tris = int(m.n_tris)
            return self
        check(lib.tbvh_build_device_mesh(self.ctx._h, C.byref(m), layout, max_leaf_tris if builder != "ploc" else 0, _device_builder(builder), radius,
                                         C.byref(self._h)), "tbvh_build_device_mesh")
        self._mesh_tris = int(m.n_tris)
        return self

    def _convert_mesh(self, layout: int, nodes32, prim_idx, verts, indices) -> "_Scene":
        nodes32 = np.ascontiguousarray(nodes32); prim_idx = np.ascontiguousarray(prim_idx, np.uint32)
        m, keep = _mesh(verts, indices)
        check(lib.tbvh_convert_bvh2_device_mesh(self.ctx._h, _ptr(nodes32), nodes32.nbytes // 32, _ptr(prim_idx), prim_idx.size, C.byref(m), 0, layout,
                                                C.byref(self._h)), "tbvh_convert_bvh2_device_mesh")
        self._mesh_tris = int(m.n_tris)
        return self

    def Refit(self, verts, on_device: bool = False, indices=None, mesh: bool = False):
        """Refit this BLAS on the device to moved vertices (tbvh_refit; BVH::Refit, tiny_bvh.h:3055-3093):
        verts is the (3 n_tris, 4) float32 vertex array (host) or a device pointer with n_tris = on_device.
        With indices=, a device_mesh(), a vertex array that is not (3 n, 4), or mesh=True: tbvh_refit_mesh — on a scene made from an indexed
        mesh, mesh=True with indices=None passes the shared vertices only and the scene's own index buffer is used."""
        if indices is not None or mesh or isinstance(verts, Mesh):
            if isinstance(verts, Mesh):
                m = verts
            else:
                v = np.asarray(verts)
                if v.dtype != np.float32 or v.ndim != 2 or v.strides[1] != 4 or v.strides[0] % 4 or v.strides[0] < 12:
                    v = np.ascontiguousarray(v, np.float32)
                idx = None if indices is None else np.ascontiguousarray(indices, np.uint32).reshape(-1)
                n_tris = idx.size // 3 if idx is not None else (getattr(self, "_mesh_tris", 0) or v.shape[0] // 3)
                m = Mesh(C.c_void_p(v.ctypes.data), v.shape[0], v.strides[0], 0, None if idx is None else C.c_void_p(idx.ctypes.data), n_tris)
            check(lib.tbvh_refit_mesh(self._h, C.byref(m)), "tbvh_refit_mesh")
            return self
        if on_device:
            ptr, n_tris = C.c_void_p(int(verts[0])), int(verts[1])
        else:
            verts = np.ascontiguousarray(verts, np.float32)
            assert verts.ndim == 2 and verts.shape[1] == 4 and verts.shape[0] % 3 == 0
            ptr, n_tris = _ptr(verts), verts.shape[0] // 3
        check(lib.tbvh_refit(self._h, ptr, n_tris, 1 if on_device else 0), "tbvh_refit")
        return self

    def SetOpacityMicroMaps(self, map_data, N: int):
        """BVHBase::SetOpacityMicroMaps (tiny_bvh.h:826): map_data = uint32 array of n_tris * ceil(N*N/32) words, or None to clear."""
        if map_data is None or N == 0:
            check(lib.tbvh_set_opacity_micromaps(self._h, None, 0, 0, 0), "tbvh_set_opacity_micromaps")
            return self
        m = np.ascontiguousarray(map_data, np.uint32).reshape(-1)
        wpt = (N * N + 31) // 32
        assert m.size % wpt == 0
        check(lib.tbvh_set_opacity_micromaps(self._h, _ptr(m), N, m.size // wpt, 0), "tbvh_set_opacity_micromaps")
        return self

    def SetTriangleTest(self, test: str, vertices=None):
        """The scene's triangle test (tbvh_set_triangle_test; WATERTIGHT_TRITEST, tiny_bvh.h:141): "moller-trumbore" (the default) or "watertight".
        vertices: the (3 n_tris, 4) float32 array the scene was built from, as Refit takes it, or a (device pointer, n_tris) pair; None on a scene that is
        watertight already.  Triangle BLASes only; the C entry point refuses everything else and says why."""
        codes = {"moller-trumbore": TRITEST_MOLLER_TRUMBORE, "watertight": TRITEST_WATERTIGHT}
        if test not in codes:
            raise ValueError(f"triangle test {test!r}: one of {sorted(codes)}")
        if vertices is None:
            ptr, n_tris, dev = None, 0, 0
        elif isinstance(vertices, tuple):
            ptr, n_tris, dev = C.c_void_p(int(vertices[0])), int(vertices[1]), 1
        else:
            vertices = np.ascontiguousarray(vertices, np.float32)
            assert vertices.ndim == 2 and vertices.shape[1] == 4 and vertices.shape[0] % 3 == 0
            ptr, n_tris, dev = _ptr(vertices), vertices.shape[0] // 3, 0
        check(lib.tbvh_set_triangle_test(self._h, codes[test], ptr, n_tris, dev), "tbvh_set_triangle_test")
        return self

    @property
    def triangle_test(self) -> str:
        r = lib.tbvh_scene_triangle_test(self._h)
        check(min(r, 0), "tbvh_scene_triangle_test")
        return "watertight" if r == TRITEST_WATERTIGHT else "moller-trumbore"

    def BakeOpacityMicroMaps(self, uv, textures, N: int = 32, indices=None, tri_texture=None):
        """Mesh::CreateOpacityMicroMaps( N ) of tiny_scene.h on the device, installed on this scene without a host round trip (tbvh_bake_set_opacity_micromaps):
        uv, textures, indices, tri_texture as bake_opacity_micromaps takes them, or an OmmSource made by device_omm_source()."""
        src, keep = _omm_source(uv, textures, indices, tri_texture)
        check(lib.tbvh_bake_set_opacity_micromaps(self._h, C.byref(src), N), "tbvh_bake_set_opacity_micromaps")
        del keep

    def download_blobs(self):
        """(nodes, triangle records) as (n, 4) uint32 arrays of 16-byte blocks, read back from the device."""
        out = []
        for which in (0, 1):
            nb = C.c_uint64(0)
            check(lib.tbvh_scene_download(self._h, which, None, 0, C.byref(nb)), "tbvh_scene_download")
            a = np.zeros((nb.value // 16, 4), np.uint32)
            if nb.value:
                check(lib.tbvh_scene_download(self._h, which, _ptr(a), nb.value, C.byref(nb)), "tbvh_scene_download")
            out.append(a)
        return tuple(out)

    def coherent_schedule(self, anyhit: bool = False):
        """(decision, samples of the deferred schedule, samples of the strict one, 1000 x strict / deferred time per ray): tbvh_debug_coherent_schedule."""
        out = (C.c_uint32 * 4)()
        check(lib.tbvh_debug_coherent_schedule(self._h, 1 if anyhit else 0, out), "tbvh_debug_coherent_schedule")
        return tuple(int(x) for x in out)

    def schedule_hint(self):
        """tbvh_scene_get_schedule_hint: {"closest_hit": [c0, c1, c2], "any_hit": [...]} per batch-size class (< 6 M, < 12 M, more rays); 0 undecided, 1 deferred + gated, 2 strict."""
        b = (C.c_uint8 * 8)()
        check(lib.tbvh_scene_get_schedule_hint(self._h, C.cast(b, C.c_void_p)), "tbvh_scene_get_schedule_hint")
        return {"closest_hit": [int(b[0]), int(b[1]), int(b[2])], "any_hit": [int(b[3]), int(b[4]), int(b[5])], "small_batches": [int(b[6]), int(b[7])]}   # small_batches: 768 k .. 1.5 M rays on a scene under 48 MB (closest-hit, any-hit)

    def set_schedule_hint(self, hint) -> None:
        """tbvh_scene_set_schedule_hint: pins the non-zero entries of a dict as schedule_hint() returns it; zero entries go back to measuring."""
        b = (C.c_uint8 * 8)(*(list(hint["closest_hit"]) + list(hint["any_hit"]) + list(hint.get("small_batches", [0, 0]))))
        check(lib.tbvh_scene_set_schedule_hint(self._h, C.cast(b, C.c_void_p)), "tbvh_scene_set_schedule_hint")

    def set_variant(self, v: int):
        check(lib.tbvh_set_variant(self._h, v), "tbvh_set_variant")

    def set_hybrid(self, packed_nodes: int):
        """BVH8_CWBVH: traverse a priority-ordered copy of the nodes whose first `packed_nodes` are packed and the others
        one per 128-byte line (tbvh_cwbvh_set_hybrid); < 0: back to the uploaded array."""
        check(lib.tbvh_cwbvh_set_hybrid(self._h, int(packed_nodes)), "tbvh_cwbvh_set_hybrid")

    def Intersect(self, rays: np.ndarray) -> np.ndarray:
        """rays: structured RAY_DTYPE array (64-byte records) or a (n, 128)-byte host Ray[] view;
        updated in place (bytes 44..63 of records that hit) and returned."""
        assert rays.flags["C_CONTIGUOUS"] and rays.flags["WRITEABLE"]
        stride = rays.strides[0] if rays.shape[0] else max(rays.dtype.itemsize, 64)
        check(lib.tbvh_intersect(self._h, _ptr(rays), rays.shape[0], stride), "tbvh_intersect")
        return rays

    def IsOccluded(self, rays: np.ndarray) -> np.ndarray:
        assert rays.flags["C_CONTIGUOUS"]
        out = np.zeros(rays.shape[0], dtype=np.uint8)
        stride = rays.strides[0] if rays.shape[0] else max(rays.dtype.itemsize, 64)
        check(lib.tbvh_occluded(self._h, _ptr(rays), rays.shape[0], stride, _ptr(out)), "tbvh_occluded")
        return out

    # device-resident, asynchronous
    def intersect_device(self, d_rays: int, n: int):
        check(lib.tbvh_intersect_device(self._h, C.c_void_p(d_rays), n), "tbvh_intersect_device")

    def intersect_device_fresh(self, d_rays: int, n: int, tmax: float = 1e30):
        check(lib.tbvh_intersect_device_fresh(self._h, C.c_void_p(d_rays), n, float(tmax)), "tbvh_intersect_device_fresh")

    def occluded_device(self, d_rays: int, n: int, d_out: int):
        check(lib.tbvh_occluded_device(self._h, C.c_void_p(d_rays), n, C.c_void_p(d_out)), "tbvh_occluded_device")


class _SphereQueries:
    """BVH::IntersectSphere (tiny_bvh.h:3140-3200) over a BLAS, batched (tbvh_intersect_spheres): does a sphere touch any triangle?
    verts is the vertex array the scene was built from (3 bvhvec4 per triangle), as Refit takes it."""

    def intersect_spheres(self, spheres: np.ndarray, verts: np.ndarray, indices=None) -> np.ndarray:
        """spheres: (n, 4) float32 {x, y, z, r}; returns uint8[n], 1 = the sphere touches a triangle.
        indices= (or a device_mesh() / a vertex array that is not (3 n, 4)): the mesh form, tbvh_intersect_spheres_mesh."""
        spheres = np.ascontiguousarray(spheres, np.float32).reshape(-1, 4)
        if _is_mesh(verts, indices):
            m, keep = _mesh(verts, indices)
            out = np.zeros(spheres.shape[0], np.uint8)
            check(lib.tbvh_intersect_spheres_mesh(self._h, _ptr(spheres), spheres.shape[0], C.byref(m), _ptr(out)), "tbvh_intersect_spheres_mesh")
            return out
        verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 4)
        assert verts.shape[0] % 3 == 0
        out = np.zeros(spheres.shape[0], np.uint8)
        check(lib.tbvh_intersect_spheres(self._h, _ptr(spheres), spheres.shape[0], _ptr(verts), verts.shape[0] // 3, _ptr(out)),
              "tbvh_intersect_spheres")
        return out

    def intersect_spheres_device(self, d_spheres: int, n: int, d_verts: int, n_tris: int, d_hit: int):
        """device arrays (16-byte spheres, 3 x 16-byte vertices per triangle, 1 byte per answer); asynchronous on the context's stream"""
        check(lib.tbvh_intersect_spheres_device(self._h, C.c_void_p(d_spheres), n, C.c_void_p(d_verts), n_tris, C.c_void_p(d_hit)),
              "tbvh_intersect_spheres_device")

    def intersect_spheres_mesh_device(self, d_spheres: int, n: int, mesh: Mesh, d_hit: int):
        """the same with a device_mesh(); asynchronous on the context's stream"""
        check(lib.tbvh_intersect_spheres_mesh_device(self._h, C.c_void_p(d_spheres), n, C.byref(mesh), C.c_void_p(d_hit)), "tbvh_intersect_spheres_mesh_device")

    def intersect_sphere(self, pos, r: float, verts: np.ndarray, indices=None) -> bool:
        """one sphere, as BVH::IntersectSphere( pos, r ) asks it"""
        s = np.array([[pos[0], pos[1], pos[2], r]], np.float32)
        return bool(self.intersect_spheres(s, verts, indices)[0])


class BVH_GPU(_SphereQueries, _Scene):
    """Aila-Laine 2-wide layout (tiny_bvh.h:1092-1127)."""
    layout = LAYOUT_BVH_GPU

    def Build(self, verts: np.ndarray, indices=None, **kw) -> "BVH_GPU":
        if _is_mesh(verts, indices):
            return self._build_mesh(LAYOUT_BVH_GPU, verts, indices, kw)
        self.host = HostBVH(verts, LAYOUT_BVH_GPU, **kw)
        return self.Upload(self.host.blob(0, np.uint32, 16), self.host.blob(1, np.uint32, 1), self.host.verts)

    def Upload(self, nodes64: np.ndarray, prim_idx: np.ndarray, verts: np.ndarray, indices=None) -> "BVH_GPU":
        """verts: the caller's bvhvec4 array, 3 per triangle; with indices= (BVH_GPU::Build( verts, indices, n )), a device_mesh() or a strided
        vertex array: tbvh_upload_bvh_gpu_mesh."""
        nodes64 = np.ascontiguousarray(nodes64); prim_idx = np.ascontiguousarray(prim_idx, dtype=np.uint32)
        if _is_mesh(verts, indices):
            m, keep = _mesh(verts, indices)
            check(lib.tbvh_upload_bvh_gpu_mesh(self.ctx._h, _ptr(nodes64), nodes64.nbytes // 64, _ptr(prim_idx), prim_idx.size, C.byref(m), C.byref(self._h)),
                  "tbvh_upload_bvh_gpu_mesh")
            self._mesh_tris = int(m.n_tris)
            return self
        verts = np.ascontiguousarray(verts, dtype=np.float32)
        check(lib.tbvh_upload_bvh_gpu(self.ctx._h, _ptr(nodes64), nodes64.nbytes // 64, _ptr(prim_idx), prim_idx.size,
                                      _ptr(verts), verts.size // 12, C.byref(self._h)), "tbvh_upload_bvh_gpu")
        return self

    def Update(self, nodes64: np.ndarray, prim_idx: np.ndarray, verts: np.ndarray, indices=None) -> "BVH_GPU":
        """In-place re-upload of a blob refitted / re-converted on the host (tbvh_update_bvh_gpu; mesh forms: tbvh_update_bvh_gpu_mesh): same handle, same device memory."""
        nodes64 = np.ascontiguousarray(nodes64); prim_idx = np.ascontiguousarray(prim_idx, dtype=np.uint32)
        if _is_mesh(verts, indices):
            m, keep = _mesh(verts, indices)
            check(lib.tbvh_update_bvh_gpu_mesh(self._h, _ptr(nodes64), nodes64.nbytes // 64, _ptr(prim_idx), prim_idx.size, C.byref(m)), "tbvh_update_bvh_gpu_mesh")
            return self
        verts = np.ascontiguousarray(verts, dtype=np.float32)
        check(lib.tbvh_update_bvh_gpu(self._h, _ptr(nodes64), nodes64.nbytes // 64, _ptr(prim_idx), prim_idx.size, _ptr(verts), verts.size // 12), "tbvh_update_bvh_gpu")
        return self


class BVH4_GPU(_SphereQueries, _Scene):
    """Quantized 4-wide layout with inline triangles (tiny_bvh.h:1245-1289)."""
    layout = LAYOUT_BVH4_GPU

    def Build(self, verts: np.ndarray, indices=None, **kw) -> "BVH4_GPU":
        if _is_mesh(verts, indices):
            return self._build_mesh(LAYOUT_BVH4_GPU, verts, indices, kw)
        self.host = HostBVH(verts, LAYOUT_BVH4_GPU, **kw)
        return self.Upload(self.host.blob(0, np.uint32, 4))

    def BuildOnDevice(self, verts: np.ndarray, max_leaf_tris: int = 4, builder: str = "lbvh", radius: int = 0, indices=None) -> "BVH4_GPU":
        """LBVH (tbvh_build_device), PLOC (tbvh_build_device_ploc) or, with builder="sah", the reference's binned-SAH tree (tbvh_build_device_sah), or with
        builder="sbvh" its spatial-split tree (BVH::BuildHQ: tbvh_build_device_sbvh) + 4-wide collapse + encode on the GPU (mesh forms: tbvh_build_device_mesh)."""
        _device_builder(builder)
        if _is_mesh(verts, indices):
            return self._build_device_mesh(LAYOUT_BVH4_GPU, verts, indices, max_leaf_tris, builder, radius)
        verts = np.ascontiguousarray(verts, np.float32)
        if builder == "ploc":
            check(lib.tbvh_build_device_ploc(self.ctx._h, _ptr(verts), verts.shape[0] // 3, 0, LAYOUT_BVH4_GPU, radius, C.byref(self._h)), "tbvh_build_device_ploc")
        elif builder == "sah":
            check(lib.tbvh_build_device_sah(self.ctx._h, _ptr(verts), verts.shape[0] // 3, 0, LAYOUT_BVH4_GPU, max_leaf_tris, C.byref(self._h)), "tbvh_build_device_sah")
        elif builder == _SBVH:
            check(lib.tbvh_build_device_sbvh(self.ctx._h, _ptr(verts), verts.shape[0] // 3, 0, LAYOUT_BVH4_GPU, max_leaf_tris, C.byref(self._h)), "tbvh_build_device_sbvh")
        else:
            check(lib.tbvh_build_device(self.ctx._h, _ptr(verts), verts.shape[0] // 3, 0, LAYOUT_BVH4_GPU, max_leaf_tris, C.byref(self._h)), "tbvh_build_device")
        return self

    def ConvertFromBVH2(self, nodes32: np.ndarray, prim_idx: np.ndarray, verts: np.ndarray, indices=None) -> "BVH4_GPU":
        """BVH4_GPU::ConvertFrom on the device (tbvh_convert_bvh2_device; mesh forms: tbvh_convert_bvh2_device_mesh)."""
        if _is_mesh(verts, indices):
            return self._convert_mesh(LAYOUT_BVH4_GPU, nodes32, prim_idx, verts, indices)
        nodes32 = np.ascontiguousarray(nodes32); prim_idx = np.ascontiguousarray(prim_idx, np.uint32); verts = np.ascontiguousarray(verts, np.float32)
        check(lib.tbvh_convert_bvh2_device(self.ctx._h, _ptr(nodes32), nodes32.nbytes // 32, _ptr(prim_idx), prim_idx.size, _ptr(verts), verts.shape[0] // 3,
                                           0, LAYOUT_BVH4_GPU, C.byref(self._h)), "tbvh_convert_bvh2_device")
        return self

    def Upload(self, blocks16: np.ndarray) -> "BVH4_GPU":
        blocks16 = np.ascontiguousarray(blocks16)
        check(lib.tbvh_upload_bvh4_gpu(self.ctx._h, _ptr(blocks16), blocks16.nbytes // 16, C.byref(self._h)), "tbvh_upload_bvh4_gpu")
        return self

    def Update(self, blocks16: np.ndarray) -> "BVH4_GPU":
        """In-place re-upload of a blob refitted / re-converted on the host (tbvh_update_bvh4_gpu)."""
        blocks16 = np.ascontiguousarray(blocks16)
        check(lib.tbvh_update_bvh4_gpu(self._h, _ptr(blocks16), blocks16.nbytes // 16), "tbvh_update_bvh4_gpu")
        return self


class BVH8_CWBVH(_SphereQueries, _Scene):
    """Compressed wide BVH (tiny_bvh.h:1334-1362)."""
    layout = LAYOUT_CWBVH

    def Build(self, verts: np.ndarray, indices=None, **kw) -> "BVH8_CWBVH":
        if _is_mesh(verts, indices):
            return self._build_mesh(LAYOUT_CWBVH, verts, indices, kw)
        self.host = HostBVH(verts, LAYOUT_CWBVH, **kw)
        return self.Upload(self.host.blob(0, np.uint32, 4), self.host.blob(1, np.uint32, 4))

    def BuildOnDevice(self, verts: np.ndarray, max_leaf_tris: int = 0, builder: str = "lbvh", radius: int = 0, indices=None) -> "BVH8_CWBVH":
        """LBVH (tbvh_build_device), PLOC (tbvh_build_device_ploc) or, with builder="sah", the reference's binned-SAH tree (tbvh_build_device_sah), or with
        builder="sbvh" its spatial-split tree (BVH::BuildHQ: tbvh_build_device_sbvh) + wide collapse + encode on the GPU; nothing is built on the host (mesh forms: tbvh_build_device_mesh)."""
        _device_builder(builder)
        if _is_mesh(verts, indices):
            return self._build_device_mesh(LAYOUT_CWBVH, verts, indices, max_leaf_tris, builder, radius)
        verts = np.ascontiguousarray(verts, np.float32)
        if builder == "ploc":
            check(lib.tbvh_build_device_ploc(self.ctx._h, _ptr(verts), verts.shape[0] // 3, 0, LAYOUT_CWBVH, radius, C.byref(self._h)), "tbvh_build_device_ploc")
        elif builder == "sah":
            check(lib.tbvh_build_device_sah(self.ctx._h, _ptr(verts), verts.shape[0] // 3, 0, LAYOUT_CWBVH, max_leaf_tris, C.byref(self._h)), "tbvh_build_device_sah")
        elif builder == _SBVH:
            check(lib.tbvh_build_device_sbvh(self.ctx._h, _ptr(verts), verts.shape[0] // 3, 0, LAYOUT_CWBVH, max_leaf_tris, C.byref(self._h)), "tbvh_build_device_sbvh")
        else:
            check(lib.tbvh_build_device(self.ctx._h, _ptr(verts), verts.shape[0] // 3, 0, LAYOUT_CWBVH, max_leaf_tris, C.byref(self._h)), "tbvh_build_device")
        return self

    def ConvertFromBVH2(self, nodes32: np.ndarray, prim_idx: np.ndarray, verts: np.ndarray, indices=None) -> "BVH8_CWBVH":
        """BVH8_CWBVH::ConvertFrom on the device (tbvh_convert_bvh2_device): a plain BVH2 (32-byte BVHNode
        array with leaves of at most 3 triangles, primIdx, vertices) goes up, the GPU collapses and encodes (mesh forms: tbvh_convert_bvh2_device_mesh)."""
        if _is_mesh(verts, indices):
            return self._convert_mesh(LAYOUT_CWBVH, nodes32, prim_idx, verts, indices)
        nodes32 = np.ascontiguousarray(nodes32); prim_idx = np.ascontiguousarray(prim_idx, np.uint32); verts = np.ascontiguousarray(verts, np.float32)
        check(lib.tbvh_convert_bvh2_device(self.ctx._h, _ptr(nodes32), nodes32.nbytes // 32, _ptr(prim_idx), prim_idx.size, _ptr(verts), verts.shape[0] // 3,
                                           0, LAYOUT_CWBVH, C.byref(self._h)), "tbvh_convert_bvh2_device")
        return self

    def Save(self, path: str, n_tris: int = 0, bounds=None) -> None:
        """BVH8_CWBVH::Save (tiny_bvh.h:5786-5795): a file BVH8_CWBVH::Load accepts.  The blobs come from the host
        copy if this scene was built here, else they are read back from the device."""
        host = getattr(self, "host", None)
        if host is not None:
            nodes, tris = host.blob(0, np.uint32, 4), host.blob(1, np.uint32, 4)
            n_tris = n_tris or host.n_tris
        else:
            nodes, tris = self.download_blobs()
        n_tris = n_tris or tris.shape[0] // 3
        b = None if bounds is None else np.ascontiguousarray(bounds, np.float32).reshape(6)
        check(lib.tbvh_cwbvh_file_write(os.fsencode(path), _ptr(nodes), nodes.shape[0], _ptr(tris), tris.shape[0], n_tris,
                                        None if b is None else _ptr(b)), "tbvh_cwbvh_file_write")

    def Load(self, path: str, expected_tris: int = 0) -> "BVH8_CWBVH":
        """BVH8_CWBVH::Load (tiny_bvh.h:5797-5820) + upload: also reads files written by the reference itself."""
        self.host = HostBVH.from_cwbvh_file(path, expected_tris)
        return self.Upload(self.host.blob(0, np.uint32, 4), self.host.blob(1, np.uint32, 4))

    def Upload(self, nodes16: np.ndarray, tris16: np.ndarray) -> "BVH8_CWBVH":
        nodes16 = np.ascontiguousarray(nodes16); tris16 = np.ascontiguousarray(tris16)
        check(lib.tbvh_upload_cwbvh(self.ctx._h, _ptr(nodes16), nodes16.nbytes // 16, _ptr(tris16), tris16.nbytes // 16,
                                    C.byref(self._h)), "tbvh_upload_cwbvh")
        return self

    def Update(self, nodes16: np.ndarray, tris16: np.ndarray) -> "BVH8_CWBVH":
        """In-place re-upload of a blob refitted / re-converted on the host (tbvh_update_cwbvh): BVH::Refit + ConvertFrom of the
        reference's animation flow without freeing the scene; TLASes over this BLAS keep working."""
        nodes16 = np.ascontiguousarray(nodes16); tris16 = np.ascontiguousarray(tris16)
        check(lib.tbvh_update_cwbvh(self._h, _ptr(nodes16), nodes16.nbytes // 16, _ptr(tris16), tris16.nbytes // 16), "tbvh_update_cwbvh")
        return self


LAYOUT_CLASSES = {LAYOUT_BVH_GPU: BVH_GPU, LAYOUT_BVH4_GPU: BVH4_GPU, LAYOUT_CWBVH: BVH8_CWBVH}


def intersect_sharded(replicas: list, rays: np.ndarray) -> np.ndarray:
    """ONE ray array over several devices (tbvh_intersect_sharded): replicas[i] is the same BVH uploaded
    through its own Context; contiguous wave-aligned shards, one host thread per device, results written in place."""
    assert rays.flags["C_CONTIGUOUS"] and rays.dtype.itemsize in (64, 128)
    arr = (C.c_void_p * len(replicas))(*[r._h for r in replicas])
    check(lib.tbvh_intersect_sharded(arr, len(replicas), _ptr(rays), rays.shape[0], rays.dtype.itemsize), "tbvh_intersect_sharded")
    return rays


def occluded_sharded(replicas: list, rays: np.ndarray) -> np.ndarray:
    assert rays.flags["C_CONTIGUOUS"] and rays.dtype.itemsize in (64, 128)
    occ = np.zeros(rays.shape[0], np.uint8)
    arr = (C.c_void_p * len(replicas))(*[r._h for r in replicas])
    check(lib.tbvh_occluded_sharded(arr, len(replicas), _ptr(rays), rays.shape[0], rays.dtype.itemsize, _ptr(occ)), "tbvh_occluded_sharded")
    return occ


def intersect_sharded_device(replicas: list, d_rays: list, n_rays: list, fresh: bool = True, tmax: float = 1e30):
    """Device-resident shards (tbvh_intersect_sharded_device): d_rays[i] / n_rays[i] live on the device of replicas[i]; one host thread
    enqueues all launches, then waits.  Returns (kernel ms per device, host dispatch ms per device)."""
    k = len(replicas)
    sc = (C.c_void_p * k)(*[r._h for r in replicas])
    dp = (C.c_void_p * k)(*[int(p) for p in d_rays])
    nn = (C.c_uint64 * k)(*[int(x) for x in n_rays])
    km, dm = (C.c_float * k)(), (C.c_float * k)()
    check(lib.tbvh_intersect_sharded_device(sc, k, dp, nn, 1 if fresh else 0, float(tmax), km, dm), "tbvh_intersect_sharded_device")
    return [float(x) for x in km], [float(x) for x in dm]


def occluded_sharded_device(replicas: list, d_rays: list, n_rays: list, d_occ: list):
    k = len(replicas)
    sc = (C.c_void_p * k)(*[r._h for r in replicas])
    dp = (C.c_void_p * k)(*[int(p) for p in d_rays])
    do = (C.c_void_p * k)(*[int(p) for p in d_occ])
    nn = (C.c_uint64 * k)(*[int(x) for x in n_rays])
    km, dm = (C.c_float * k)(), (C.c_float * k)()
    check(lib.tbvh_occluded_sharded_device(sc, k, dp, nn, do, km, dm), "tbvh_occluded_sharded_device")
    return [float(x) for x in km], [float(x) for x in dm]


def wavefront_render_sharded(wfs: list, scenes_: list, d_verts: list, cam: Camera, light_pos, light_color=(1.0, 1.0, 1.0), sky_lo=(0.6, 0.7, 0.8), sky_hi=(0.2, 0.4, 0.9),
                             eps: float = 1e-3, max_depth: int = 3, seed: int = 1, clear: bool = True, light_size=(0.0, 0.0)):
    """One frame over several devices (tbvh_wavefront_render_sharded): wfs[i] is the band of the image (Wavefront.set_band) rendered on
    the device of scenes_[i].  Returns per band {"extend_rays", "shadow_rays", "frame_ms", "dispatch_ms"}."""
    k = len(wfs)
    p = _capi.WfParams()
    p.light_pos[:] = [float(x) for x in light_pos]; p.light_color[:] = [float(x) for x in light_color]
    p.sky_lo[:] = [float(x) for x in sky_lo]; p.sky_hi[:] = [float(x) for x in sky_hi]
    p.eps, p.max_depth, p.seed, p.clear = float(eps), int(max_depth), int(seed), int(clear)
    p.light_size[:] = [float(x) for x in light_size]; p.flags = 0; p.sample_index = 0xFFFFFFFF
    wa = (C.c_void_p * k)(*[w._h for w in wfs])
    sa = (C.c_void_p * k)(*[s._h for s in scenes_])
    va = (C.c_void_p * k)(*[int(v) if v else None for v in d_verts])
    st = (_capi.WfStats * k)()
    dm = (C.c_float * k)()
    check(lib.tbvh_wavefront_render_sharded(wa, sa, va, k, C.byref(cam), C.byref(p), st, dm), "tbvh_wavefront_render_sharded")
    return [{"extend_rays": [int(x) for x in st[i].extend_rays[:max_depth]], "shadow_rays": [int(x) for x in st[i].shadow_rays[:max_depth]],
             "frame_ms": float(st[i].frame_ms), "dispatch_ms": float(dm[i])} for i in range(k)]


def wavefront_read_sharded(wfs: list, width: int, full_height: int) -> np.ndarray:
    img = np.zeros((full_height, width, 4), np.float32)
    wa = (C.c_void_p * len(wfs))(*[w._h for w in wfs])
    check(lib.tbvh_wavefront_read_sharded(wa, len(wfs), _ptr(img)), "tbvh_wavefront_read_sharded")
    return img


def device_count() -> int:
    return int(lib.tbvh_device_count())


# BLASInstance, 192 bytes (tiny_bvh.h:1443-1457); transform is row-major with the translation in
# elements 3, 7, 11 (tiny_bvh.h:513-528)
INSTANCE_DTYPE = np.dtype([
    ("transform", "<f4", 16), ("invTransform", "<f4", 16),
    ("aabbMin", "<f4", 3), ("blasIdx", "<u4"), ("aabbMax", "<f4", 3), ("mask", "<u4"), ("pad", "<u4", 8),
])
assert INSTANCE_DTYPE.itemsize == 192


def make_instances(transforms: np.ndarray, blas_idx, mask: int = 0xFFFF) -> np.ndarray:
    """BLASInstance records from (n, 4, 4) row-major transforms; invTransform and the bounds are
    filled by TLAS.Build (BLASInstance::Update, tiny_bvh.h:8386-8400)."""
    t = np.ascontiguousarray(transforms, np.float32).reshape(-1, 16)
    inst = np.zeros(t.shape[0], INSTANCE_DTYPE)
    inst["transform"] = t
    inst["invTransform"] = np.eye(4, dtype=np.float32).reshape(16)
    inst["blasIdx"] = blas_idx
    inst["mask"] = mask
    return inst


TLAS_FAMILIES = ("TlasSphere", "Tlas4", "Tlas8", "TlasVoxel", "Tlas2", "TlasFlat")   # tlas_plan.h: TlasFamily
TLAS_VIEWS = ("own", "copy8", "copy4")                                                # tlas_plan.h: TlasView


def tlas_facts_dict(w) -> dict:
    """one case of tbvh_debug_tlas_plan's fact words, named"""
    blas = [{"layout": int(x) & 0xFF, "pinned": bool(int(x) >> 8 & 1), "has8": bool(int(x) >> 9 & 1), "has4": bool(int(x) >> 10 & 1)} for x in w[5:]]
    return {"any_hit_seen": bool(w[1]), "has_nodes": bool(w[2]), "cap8": int(w[3]), "cap4": int(w[4]), "blas": blas, "words": np.array(w, np.uint64)}


def tlas_plan_dict(w) -> dict:
    """one case of tbvh_debug_tlas_plan's plan words, named"""
    kind = lambda k, shift: {"layout": int(w[k]), "mix": bool(w[k + 1]), "family": TLAS_FAMILIES[int(w[k + 2])], "entry_bytes": int(w[k + 3]),
                             "views": [TLAS_VIEWS[int(x) >> shift & 0xFF] for x in w[13:]]}
    return {"closest": kind(0, 0), "any": kind(4, 8), "any_own": bool(w[8]), "want8": bool(w[9]), "fits8": bool(w[10]), "want4": bool(w[11]), "fits4": bool(w[12]),
            "words": np.array(w, np.uint32)}


class TLAS(_Scene):
    """Top-level BVH over BLAS instances: BVH_GPU nodes over BLASInstance records
    (BVH_GPU::Build(BLASInstance*, ...), tiny_bvh.h:4575-4581; tiny_bvh_gpu2.cpp:108-136)."""
    layout = LAYOUT_BVH_GPU

    def Build(self, instances: np.ndarray, blas: list) -> "TLAS":
        """instances: INSTANCE_DTYPE array with transform/blasIdx/mask set (updated in place);
        blas: uploaded BLAS scenes (BVH8_CWBVH, BVH4_GPU or BVH_GPU, also mixed) built with .Build()."""
        assert instances.dtype == INSTANCE_DTYPE and instances.flags["C_CONTIGUOUS"]
        bounds = np.zeros((len(blas), 6), np.float32)
        for i, b in enumerate(blas):
            if getattr(b, "_bounds", None) is None:      # root box of the BLAS, computed once
                v = b.host.verts[:, :3]
                b._bounds = np.concatenate([v.min(0), v.max(0)]).astype(np.float32)
            bounds[i] = b._bounds
        h = C.c_void_p()
        check(lib.tbvh_host_build_tlas(_ptr(instances), instances.shape[0], _ptr(bounds), len(blas), C.byref(h)), "tbvh_host_build_tlas")
        host = HostBVH.__new__(HostBVH)
        host._h = h; host.layout = LAYOUT_BVH_GPU; host.verts = None; host.n_tris = instances.shape[0]
        self.host = host
        self.instances = instances
        self.blas = list(blas)
        nodes = host.blob(0, np.uint32, 16); idx = host.blob(1, np.uint32, 1)
        if self._h:
            return self.Update(nodes, idx, instances)
        return self.Upload(nodes, idx, instances, blas)

    def Upload(self, nodes64: np.ndarray, tlas_idx: np.ndarray, instances: np.ndarray, blas: list) -> "TLAS":
        nodes64 = np.ascontiguousarray(nodes64); tlas_idx = np.ascontiguousarray(tlas_idx, np.uint32)
        arr = (C.c_void_p * len(blas))(*[b._h for b in blas])
        check(lib.tbvh_upload_tlas(self.ctx._h, _ptr(nodes64), nodes64.nbytes // 64, _ptr(tlas_idx), tlas_idx.size, _ptr(instances),
                                   instances.shape[0], arr, len(blas), C.byref(self._h)), "tbvh_upload_tlas")
        self.blas = list(blas)  # BLAS scenes must outlive the TLAS
        return self

    def Update(self, nodes64: np.ndarray, tlas_idx: np.ndarray, instances: np.ndarray) -> "TLAS":
        nodes64 = np.ascontiguousarray(nodes64); tlas_idx = np.ascontiguousarray(tlas_idx, np.uint32)
        check(lib.tbvh_update_tlas(self._h, _ptr(nodes64), nodes64.nbytes // 64, _ptr(tlas_idx), tlas_idx.size, _ptr(instances), instances.shape[0]),
              "tbvh_update_tlas")
        return self


    def debug_plan(self):
        """(facts, plan) as dicts: the facts this TLAS would state right now and the plan it has stored (tbvh_debug_tlas_state; the word layout is
        tbvh_debug_tlas_plan's, include/tinybvh_amd_debug.h); each also carries its raw words under "words"."""
        n = len(self.blas)
        fw, pw = np.zeros(5 + n, np.uint64), np.zeros(13 + n, np.uint32)
        check(lib.tbvh_debug_tlas_state(self._h, _ptr(fw), _ptr(pw)), "tbvh_debug_tlas_state")
        return tlas_facts_dict(fw), tlas_plan_dict(pw)

    def _blas_bounds(self, blas: list) -> np.ndarray:
        bounds = np.zeros((len(blas), 6), np.float32)
        for i, b in enumerate(blas):
            if getattr(b, "_bounds", None) is None:      # root box of the BLAS, computed once
                v = b.host.verts[:, :3]
                b._bounds = np.concatenate([v.min(0), v.max(0)]).astype(np.float32)
            bounds[i] = b._bounds
        return bounds

    def SetBuilder(self, builder: str) -> "TLAS":
        """The tree RebuildOnDevice builds from now on: "lbvh" (the default) or "sah", the reference's own BVH::Build( BLASInstance*, n ) tree
        (tbvh_tlas_set_builder)."""
        if builder not in ("lbvh", "sah"):
            raise ValueError(f"TLAS.SetBuilder: builder {builder!r} (lbvh or sah)")
        check(lib.tbvh_tlas_set_builder(self._h, {"lbvh": 0, "sah": 2}[builder]), "tbvh_tlas_set_builder")
        return self

    def RebuildOnDevice(self, transforms=None, on_device: bool = False, builder=None) -> "TLAS":
        """Per-frame rebuild on the GPU (tbvh_rebuild_tlas_device): instance update + LBVH TLAS (or the reference's SAH TLAS: builder="sah",
        which stays set, as after SetBuilder), no host build and no node upload.  transforms: (n, 16) float32 array (host), a device pointer (int,
        on_device=True), or None to keep the transforms already in the device records."""
        if builder is not None:
            self.SetBuilder(builder)
        bounds = self._blas_bounds(self.blas)   # sent with the first call, and again when a BLAS's box has changed (SphereBVH.RebuildOnDevice / Refit)
        last = getattr(self, "_bounds_last", None)
        if getattr(self, "_bounds_sent", False) and (last is None or np.array_equal(bounds, last)):
            bounds = None
        if transforms is None:
            t = None
        elif on_device:
            t = C.c_void_p(int(transforms))
        else:
            transforms = np.ascontiguousarray(transforms, np.float32)
            assert transforms.size == self.instances.shape[0] * 16
            t = _ptr(transforms)
        check(lib.tbvh_rebuild_tlas_device(self._h, t, 1 if on_device else 0, _ptr(bounds) if bounds is not None else None,
                                           len(self.blas) if bounds is not None else 0), "tbvh_rebuild_tlas_device")
        self._bounds_sent = True
        if bounds is not None:
            self._bounds_last = bounds
        return self

    def Download(self):
        """(nodes64 as (n,16) uint32, tlas_idx, instances) currently on the device."""
        n = self.instances.shape[0]
        nn = C.c_uint64(0)
        check(lib.tbvh_tlas_download(self._h, None, 0, None, 0, None, 0, C.byref(nn)), "tbvh_tlas_download")
        nodes = np.zeros((nn.value, 16), np.uint32); idx = np.zeros(n, np.uint32); inst = np.zeros(n, INSTANCE_DTYPE)
        check(lib.tbvh_tlas_download(self._h, _ptr(nodes), nn.value, _ptr(idx), n, _ptr(inst), n, C.byref(nn)), "tbvh_tlas_download")
        return nodes, idx, inst


class Wavefront:
    """Device-resident wavefront path tracer (tbvh_wavefront_*): one call enqueues a whole frame
    (Generate, {Extend, Shade} x depth, Connect) with all queues and counters on the device."""

    def __init__(self, ctx: Context, width: int, height: int):
        self.ctx, self.width, self.height = ctx, width, height
        h = C.c_void_p()
        check(lib.tbvh_wavefront_create(ctx._h, width, height, C.byref(h)), "tbvh_wavefront_create")
        self._h = h

    def render(self, scene: _Scene, d_verts: int, cam: Camera, light_pos, light_color=(1.0, 1.0, 1.0), sky_lo=(0.6, 0.7, 0.8), sky_hi=(0.2, 0.4, 0.9),
               eps: float = 1e-3, max_depth: int = 3, seed: int = 1, clear: bool = True, stats: bool = True,
               light_size=(0.0, 0.0), one_diffuse_bounce: bool = False, reference_letter: bool = False, sample_index: int = 0xFFFFFFFF):
        p = _capi.WfParams()
        p.light_pos[:] = [float(x) for x in light_pos]; p.light_color[:] = [float(x) for x in light_color]
        p.sky_lo[:] = [float(x) for x in sky_lo]; p.sky_hi[:] = [float(x) for x in sky_hi]
        p.eps, p.max_depth, p.seed, p.clear = float(eps), int(max_depth), int(seed), int(clear)
        p.light_size[:] = [float(x) for x in light_size]; p.flags = (1 if one_diffuse_bounce else 0) | (2 if reference_letter else 0)
        p.sample_index = int(sample_index) & 0xFFFFFFFF
        st = _capi.WfStats()
        check(lib.tbvh_wavefront_render(self._h, scene._h, C.c_void_p(d_verts) if d_verts else None, C.byref(cam), C.byref(p), C.byref(st) if stats else None), "tbvh_wavefront_render")
        if not stats:
            return None
        return {"extend_rays": [int(x) for x in st.extend_rays[:max_depth]], "shadow_rays": [int(x) for x in st.shadow_rays[:max_depth]], "frame_ms": float(st.frame_ms)}

    def set_band(self, first_row: int, full_height: int):
        """This object renders rows [first_row, first_row + height) of an image of full_height rows (tbvh_wavefront_set_band)."""
        check(lib.tbvh_wavefront_set_band(self._h, int(first_row), int(full_height)), "tbvh_wavefront_set_band")
        return self

    def read(self) -> np.ndarray:
        img = np.zeros((self.height, self.width, 4), np.float32)
        check(lib.tbvh_wavefront_read(self._h, _ptr(img)), "tbvh_wavefront_read")
        return img

    def set_blue_noise(self, table) -> None:
        """The demos' 128 x 128 x 8 blue-noise table (uint32 words), or None to remove it (tbvh_wavefront_set_blue_noise)."""
        if table is None:
            check(lib.tbvh_wavefront_set_blue_noise(self._h, None, 0), "tbvh_wavefront_set_blue_noise")
            return
        t = np.ascontiguousarray(table, np.uint32).reshape(-1)
        check(lib.tbvh_wavefront_set_blue_noise(self._h, _ptr(t), t.size), "tbvh_wavefront_set_blue_noise")

    def set_blas_vertices(self, d_verts_per_blas: list) -> None:
        """TLAS scenes: the device vertex array of every BLAS, in blasIdx order (tbvh_wavefront_set_blas_vertices)."""
        arr = (C.c_void_p * len(d_verts_per_blas))(*[int(p) for p in d_verts_per_blas])
        check(lib.tbvh_wavefront_set_blas_vertices(self._h, arr, len(d_verts_per_blas)), "tbvh_wavefront_set_blas_vertices")

    def debug_queues(self) -> dict:
        """The queues as the last render left them (tbvh_debug_wavefront_queues; a development aid, call it before finalize): "rays" / "aux" the two
        path queues (RAY_DTYPE, PATH_AUX_DTYPE), "shadow" / "shadow_aux" / "occ" the shadow queue, "path_counts"[d] (d = 0 .. 8) and "shadow_counts"[d]
        (d = 0 .. 7) the per-depth counters.  Arrays have the capacity width x height; the counters say how many entries are live."""
        n = self.width * self.height
        rays = [np.zeros(n, RAY_DTYPE) for _ in range(2)]; aux = [np.zeros(n, PATH_AUX_DTYPE) for _ in range(2)]
        shadow = np.zeros(n, RAY_DTYPE); shadow_aux = np.zeros(n, PATH_AUX_DTYPE); occ = np.zeros(n, np.uint8); cnt = np.zeros(18, np.uint64)
        check(lib.tbvh_debug_wavefront_queues(self._h, _ptr(rays[0]), _ptr(aux[0]), _ptr(rays[1]), _ptr(aux[1]), _ptr(shadow), _ptr(shadow_aux), _ptr(occ), _ptr(cnt)),
              "tbvh_debug_wavefront_queues")
        return {"rays": rays, "aux": aux, "shadow": shadow, "shadow_aux": shadow_aux, "occ": occ,
                "path_counts": [int(x) for x in cnt[:9]], "shadow_counts": [int(x) for x in cnt[9:17]]}

    def finalize(self, scale: float = 1.0) -> np.ndarray:
        """Finalize of wavefront.cl:275-286: (height, width) uint32 0x00RRGGBB."""
        px = np.zeros((self.height, self.width), np.uint32)
        check(lib.tbvh_wavefront_finalize(self._h, float(scale), _ptr(px)), "tbvh_wavefront_finalize")
        return px

    def close(self):
        if self._h and self.ctx._h:
            lib.tbvh_wavefront_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- double precision: BVH_Double, RayEx, BLASInstanceEx (tiny_bvh.h:733-761, 1035-1090, 1462-1474) --------------------------------------
BVH_DBL_FAR = 1e300   # tiny_bvh.h:145

RAYEX_DTYPE = np.dtype([
    ("O", "<f8", 3), ("D", "<f8", 3), ("rD", "<f8", 3),
    ("t", "<f8"), ("u", "<f8"), ("v", "<f8"), ("inst", "<u8"), ("prim", "<u8"),
    ("instIdx", "<u8"), ("mask", "<u8"),
])
assert RAYEX_DTYPE.itemsize == 128

INSTANCE_EX_DTYPE = np.dtype([
    ("transform", "<f8", 16), ("invTransform", "<f8", 16),
    ("aabbMin", "<f8", 3), ("blasIdx", "<u8"), ("aabbMax", "<f8", 3), ("mask", "<u8"),
])
assert INSTANCE_EX_DTYPE.itemsize == 320

NODE_DBL_DTYPE = np.dtype([("aabbMin", "<f8", 3), ("aabbMax", "<f8", 3), ("leftFirst", "<u8"), ("triCount", "<u8")])   # BVH_Double::BVHNode
assert NODE_DBL_DTYPE.itemsize == 64


def make_rays_ex(O: np.ndarray, D: np.ndarray, tmax=BVH_DBL_FAR, mask: int = 0xFFFF) -> np.ndarray:
    """RayEx records as the RayEx constructor makes them (tiny_bvh.h:744-755): D normalised with 1 / sqrt, rD = 1 / D unguarded
    (an axis-parallel ray gets rD = +-inf), hit = {tmax, 0, 0}, instIdx 0, mask & 0xFFFF."""
    O = np.ascontiguousarray(O, dtype=np.float64).reshape(-1, 3)
    D = np.ascontiguousarray(D, dtype=np.float64).reshape(-1, 3)
    with np.errstate(divide="ignore", invalid="ignore"):
        rl = 1.0 / np.sqrt(D[:, 0] * D[:, 0] + D[:, 1] * D[:, 1] + D[:, 2] * D[:, 2])
        D = D * rl[:, None]
        rD = 1.0 / D
    rays = np.zeros(O.shape[0], dtype=RAYEX_DTYPE)
    rays["O"] = O
    rays["D"] = D
    rays["rD"] = rD
    rays["t"] = tmax
    rays["mask"] = mask & 0xFFFF
    return rays


def make_instances_ex(transforms: np.ndarray, blas_idx, mask: int = 0xFFFF) -> np.ndarray:
    """BLASInstanceEx records from (n, 4, 4) row-major double transforms; invTransform and the bounds are filled by
    TLAS_Double.Build (BLASInstanceEx::Update, tiny_bvh.h:8432-8472)."""
    t = np.ascontiguousarray(transforms, np.float64).reshape(-1, 16)
    inst = np.zeros(t.shape[0], INSTANCE_EX_DTYPE)
    inst["transform"] = t
    inst["invTransform"] = np.eye(4).reshape(16)
    inst["blasIdx"] = blas_idx
    inst["mask"] = mask
    return inst


class HostBVHDouble:
    """Blobs of the library's double-precision builders (tbvh_host_build_double / tbvh_host_build_tlas_double): nodes (NODE_DBL_DTYPE)
    and the uint64 prim (TLAS: instance) indices."""

    def __init__(self, h: C.c_void_p):
        self._h = h

    def nodes(self) -> np.ndarray:
        return self._view(0, NODE_DBL_DTYPE)

    def prim_idx(self) -> np.ndarray:
        return self._view(1, np.dtype("<u8"))

    def _view(self, which: int, dtype) -> np.ndarray:
        p = lib.tbvh_host_blob(self._h, which)
        n = lib.tbvh_host_blob_count(self._h, which)
        if not p or n == 0:
            return np.zeros(0, dtype)
        buf = (C.c_char * (n * dtype.itemsize)).from_address(p)
        buf._owner = self
        a = np.frombuffer(buf, dtype=dtype)
        a.flags.writeable = False
        return a

    def __del__(self):
        try:
            if self._h:
                lib.tbvh_host_free(self._h)
                self._h = None
        except Exception:
            pass


def host_build_double(verts: np.ndarray) -> HostBVHDouble:
    """tbvh_host_build_double over a (3 n, 3) float64 triangle soup."""
    verts = np.ascontiguousarray(verts, np.float64).reshape(-1, 3)
    assert verts.shape[0] % 3 == 0
    h = C.c_void_p()
    check(lib.tbvh_host_build_double(_ptr(verts), verts.shape[0] // 3, C.byref(h)), "tbvh_host_build_double")
    return HostBVHDouble(h)


def host_build_tlas_double(instances: np.ndarray, blas_bounds: np.ndarray) -> HostBVHDouble:
    """tbvh_host_build_tlas_double: instances (INSTANCE_EX_DTYPE, updated in place) over BLASes with bounds (n_blas, 6) float64."""
    assert instances.dtype == INSTANCE_EX_DTYPE and instances.flags["C_CONTIGUOUS"]
    bounds = np.ascontiguousarray(blas_bounds, np.float64).reshape(-1, 6)
    h = C.c_void_p()
    check(lib.tbvh_host_build_tlas_double(_ptr(instances), instances.shape[0], _ptr(bounds), bounds.shape[0], C.byref(h)), "tbvh_host_build_tlas_double")
    return HostBVHDouble(h)


class _SceneDouble(_Scene):
    """A BVH_DOUBLE scene: RayEx queries only (tbvh_intersect_ex / tbvh_occluded_ex); every fp32 entry point refuses it."""
    layout = LAYOUT_BVH_DOUBLE

    def Intersect(self, rays: np.ndarray) -> np.ndarray:
        """rays: RAYEX_DTYPE array, updated in place (records that hit) and returned."""
        assert rays.dtype == RAYEX_DTYPE and rays.flags["C_CONTIGUOUS"] and rays.flags["WRITEABLE"]
        check(lib.tbvh_intersect_ex(self._h, _ptr(rays), rays.shape[0]), "tbvh_intersect_ex")
        return rays

    def IsOccluded(self, rays: np.ndarray) -> np.ndarray:
        assert rays.dtype == RAYEX_DTYPE and rays.flags["C_CONTIGUOUS"]
        out = np.zeros(rays.shape[0], dtype=np.uint8)
        check(lib.tbvh_occluded_ex(self._h, _ptr(rays), rays.shape[0], _ptr(out)), "tbvh_occluded_ex")
        return out

    def intersect_device(self, d_rays: int, n: int):
        check(lib.tbvh_intersect_ex_device(self._h, C.c_void_p(d_rays), n), "tbvh_intersect_ex_device")

    def occluded_device(self, d_rays: int, n: int, d_out: int):
        check(lib.tbvh_occluded_ex_device(self._h, C.c_void_p(d_rays), n, C.c_void_p(d_out)), "tbvh_occluded_ex_device")


class BVH_Double(_SceneDouble):
    """BVH_Double (tiny_bvh.h:1035-1090) on the device: Intersect / IsOccluded in fp64 over RayEx records."""

    def Build(self, verts: np.ndarray) -> "BVH_Double":
        """verts: (3 n, 3) float64 triangle soup (BVH_Double::verts)."""
        self.verts = np.ascontiguousarray(verts, np.float64).reshape(-1, 3)
        self.host = host_build_double(self.verts)
        return self.Upload(self.host.nodes(), self.host.prim_idx(), self.verts)

    def Upload(self, nodes: np.ndarray, prim_idx: np.ndarray, verts: np.ndarray) -> "BVH_Double":
        """nodes: BVH_Double::bvhNode (NODE_DBL_DTYPE or raw 64-byte records), prim_idx: uint64 primIdx, verts: float64 (3 n, 3)."""
        nodes = np.ascontiguousarray(nodes); prim_idx = np.ascontiguousarray(prim_idx, np.uint64)
        verts = np.ascontiguousarray(verts, np.float64)
        self.verts = verts
        self.n_tris = verts.size // 9
        check(lib.tbvh_upload_bvh_double(self.ctx._h, _ptr(nodes), nodes.nbytes // 64, _ptr(prim_idx), prim_idx.size, _ptr(verts), verts.size // 9,
                                         C.byref(self._h)), "tbvh_upload_bvh_double")
        return self

    def Refit(self, verts, on_device: bool = False) -> "BVH_Double":
        """Same topology, new vertices (tbvh_refit_double; asynchronous).  verts: (3 n, 3) float64 of the scene's triangle count, or with
        on_device=True a device pointer to as many doubles.  self.verts follows (device-resident vertices: dropped; `bounds` then reads the
        refitted root box).  TLASes over this BLAS keep stale instance boxes until their RebuildOnDevice()."""
        n_tris = self.n_tris
        if on_device:
            check(lib.tbvh_refit_double(self._h, C.c_void_p(verts), n_tris, 1), "tbvh_refit_double")
            self.verts = None
        else:
            verts = np.ascontiguousarray(verts, np.float64)
            check(lib.tbvh_refit_double(self._h, _ptr(verts), verts.size // 9, 0), "tbvh_refit_double")
            self.verts = verts
        return self

    def Download(self) -> np.ndarray:
        """The node array as it is on the device (NODE_DBL_DTYPE); synchronizes."""
        n = C.c_uint64(0)
        check(lib.tbvh_double_download(self._h, None, 0, C.byref(n)), "tbvh_double_download")
        nodes = np.zeros(n.value, NODE_DBL_DTYPE)
        check(lib.tbvh_double_download(self._h, _ptr(nodes), n.value, None), "tbvh_double_download")
        return nodes

    @property
    def bounds(self) -> np.ndarray:
        """aabbMin, aabbMax of the vertices (what BLASInstanceEx::Update reads from a BLAS: the root's box)."""
        if self.verts is None:
            root = self.Download()[0]
            return np.concatenate([root["aabbMin"], root["aabbMax"]])
        v = self.verts.reshape(-1, 3)
        return np.concatenate([v.min(0), v.max(0)])


class TLAS_Double(_SceneDouble):
    """A BVH_Double over BLASInstanceEx records (BVH_Double::Build(BLASInstanceEx*, ...); IntersectTLAS / IsOccludedTLAS)."""

    def Build(self, instances: np.ndarray, blas: list) -> "TLAS_Double":
        """instances: INSTANCE_EX_DTYPE with transform / blasIdx / mask set (updated in place); blas: uploaded BVH_Double scenes."""
        bounds = np.stack([b.bounds for b in blas])
        self.host = host_build_tlas_double(instances, bounds)
        return self.Upload(self.host.nodes(), self.host.prim_idx(), instances, blas)

    def Upload(self, nodes: np.ndarray, tlas_idx: np.ndarray, instances: np.ndarray, blas: list) -> "TLAS_Double":
        nodes = np.ascontiguousarray(nodes); tlas_idx = np.ascontiguousarray(tlas_idx, np.uint64)
        instances = np.ascontiguousarray(instances)
        arr = (C.c_void_p * len(blas))(*[b._h for b in blas])
        check(lib.tbvh_upload_tlas_double(self.ctx._h, _ptr(nodes), nodes.nbytes // 64, _ptr(tlas_idx), tlas_idx.size, _ptr(instances), instances.shape[0],
                                          arr, len(blas), C.byref(self._h)), "tbvh_upload_tlas_double")
        self.instances = instances
        self.blas = list(blas)   # the BLAS scenes must outlive the TLAS
        self._n_idx = tlas_idx.size
        return self

    def RebuildOnDevice(self, transforms=None, on_device: bool = False) -> "TLAS_Double":
        """BLASInstanceEx::Update of every instance + a new TLAS, on the device (tbvh_rebuild_tlas_double_device; asynchronous).  transforms:
        (n_inst, 4, 4) float64 row-major, with on_device=True a device pointer to as many doubles, or None: the transforms the records hold.
        The BLAS bounds are read from the BLASes as they are now (after BVH_Double.Refit: the refitted ones)."""
        if transforms is None:
            check(lib.tbvh_rebuild_tlas_double_device(self._h, None, 0), "tbvh_rebuild_tlas_double_device")
        elif on_device:
            check(lib.tbvh_rebuild_tlas_double_device(self._h, C.c_void_p(transforms), 1), "tbvh_rebuild_tlas_double_device")
        else:
            t = np.ascontiguousarray(transforms, np.float64)
            assert t.size == 16 * self.instances.shape[0], "one 4 x 4 transform per instance"
            check(lib.tbvh_rebuild_tlas_double_device(self._h, _ptr(t), 0), "tbvh_rebuild_tlas_double_device")
        self._n_idx = self.instances.shape[0]   # one leaf per instance
        return self

    def Update(self, nodes: np.ndarray, idx: np.ndarray, instances: np.ndarray) -> "TLAS_Double":
        """A TLAS built on the host into the same scene (tbvh_update_tlas_double): the BLAS list stays; validated like Upload, and a refused
        update leaves the old TLAS answering."""
        nodes = np.ascontiguousarray(nodes); idx = np.ascontiguousarray(idx, np.uint64)
        instances = np.ascontiguousarray(instances)
        check(lib.tbvh_update_tlas_double(self._h, _ptr(nodes), nodes.nbytes // 64, _ptr(idx), idx.size, _ptr(instances), instances.shape[0]), "tbvh_update_tlas_double")
        self.instances = instances
        self._n_idx = idx.size
        return self

    def Download(self):
        """(nodes, instance indices, instances) as they are on the device: NODE_DBL_DTYPE, uint64, INSTANCE_EX_DTYPE; synchronizes."""
        n_inst = self.instances.shape[0]
        n = C.c_uint64(0)
        check(lib.tbvh_tlas_double_download(self._h, None, 0, None, 0, None, 0, C.byref(n)), "tbvh_tlas_double_download")
        nodes = np.zeros(n.value, NODE_DBL_DTYPE); idx = np.zeros(self._n_idx, np.uint64); inst = np.zeros(n_inst, INSTANCE_EX_DTYPE)
        check(lib.tbvh_tlas_double_download(self._h, _ptr(nodes), n.value, _ptr(idx), idx.size, _ptr(inst), n_inst, None), "tbvh_tlas_double_download")
        return nodes, idx, inst


# ---- double precision, custom geometry: sphere BLASes (BVH_Double::Build( customGetAABB, n ) + the double demos' sphere callback) ------------
def _spheres_dbl(spheres) -> np.ndarray:
    """(n, 4) float64 {x, y, z, r}: the demos' struct Sphere { bvhdbl3 pos; double r; }"""
    return np.ascontiguousarray(spheres, np.float64).reshape(-1, 4)


def host_build_custom_spheres_double(spheres: np.ndarray) -> HostBVHDouble:
    """tbvh_host_build_custom_spheres_double over (n, 4) float64 spheres {x, y, z, r}: a BVH_Double over the boxes pos -/+ r."""
    sph = _spheres_dbl(spheres)
    h = C.c_void_p()
    check(lib.tbvh_host_build_custom_spheres_double(_ptr(sph), sph.shape[0], C.byref(h)), "tbvh_host_build_custom_spheres_double")
    return HostBVHDouble(h)


class SphereBVH_Double(_SceneDouble):
    """A BVH_Double over custom geometry whose primitives are spheres {x, y, z, r} in float64, traced on the device with the sphere callback of
    the reference's double anim demo (the sphere forms of kernels_double.hip, DESIGN.md par. 9).  Intersect / IsOccluded take RayEx records; a hit writes
    t, prim and inst = instIdx and leaves u, v as they were.  TLAS_Double takes it as a BLAS, alone or next to BVH_Double BLASes."""

    def Build(self, spheres: np.ndarray) -> "SphereBVH_Double":
        """The library's host builder over the boxes pos -/+ r, then Upload."""
        self.host = host_build_custom_spheres_double(spheres)
        return self.Upload(self.host.nodes(), self.host.prim_idx(), spheres)

    def Upload(self, nodes: np.ndarray, prim_idx: np.ndarray, spheres: np.ndarray) -> "SphereBVH_Double":
        """The reference's own arrays after Build( customGetAABB, n ): BVH_Double::bvhNode (NODE_DBL_DTYPE or raw 64-byte records), primIdx
        (uint64) and the spheres by primitive index (tbvh_upload_custom_spheres_double: validated before anything is allocated)."""
        nodes = np.ascontiguousarray(nodes); prim_idx = np.ascontiguousarray(prim_idx, np.uint64)
        sph = _spheres_dbl(spheres)
        if self._h:
            self.free()
            self._h = C.c_void_p()
        check(lib.tbvh_upload_custom_spheres_double(self.ctx._h, _ptr(nodes), nodes.nbytes // 64, _ptr(prim_idx), prim_idx.size, _ptr(sph), sph.shape[0],
                                                    C.byref(self._h)), "tbvh_upload_custom_spheres_double")
        self.spheres = sph
        return self

    @staticmethod
    def _sphere_arg(spheres):
        """(pointer, n, on_device, host array or None) of a numpy array of {x, y, z, r} or a (device_pointer, n) pair"""
        if isinstance(spheres, tuple):
            return C.c_void_p(int(spheres[0])), int(spheres[1]), 1, None
        a = _spheres_dbl(spheres)
        return _ptr(a), a.shape[0], 0, a

    def BuildOnDevice(self, spheres) -> "SphereBVH_Double":
        """An LBVH over the boxes pos -/+ r, one sphere per leaf, built on the device (tbvh_build_device_custom_spheres_double).  spheres: a
        numpy array or a (device_pointer, n) pair."""
        ptr, n, on_device, keep = self._sphere_arg(spheres)
        if self._h:
            self.free()
            self._h = C.c_void_p()
        check(lib.tbvh_build_device_custom_spheres_double(self.ctx._h, ptr, n, on_device, C.byref(self._h)), "tbvh_build_device_custom_spheres_double")
        self.spheres = keep
        return self

    def RebuildOnDevice(self, spheres) -> "SphereBVH_Double":
        """A new tree over moved spheres in the same scene (tbvh_rebuild_custom_spheres_double_device); a TLAS_Double over it needs no new
        upload, only its RebuildOnDevice() for the instance boxes."""
        ptr, n, on_device, keep = self._sphere_arg(spheres)
        check(lib.tbvh_rebuild_custom_spheres_double_device(self._h, ptr, n, on_device), "tbvh_rebuild_custom_spheres_double_device")
        self.spheres = keep
        return self

    def Download(self):
        """(nodes as NODE_DBL_DTYPE, prim_idx, the gathered spheres in prim_idx order) as they are on the device now
        (tbvh_custom_spheres_double_download)."""
        nn, ni = C.c_uint64(0), C.c_uint64(0)
        check(lib.tbvh_custom_spheres_double_download(self._h, None, 0, None, 0, None, 0, C.byref(nn), C.byref(ni)), "tbvh_custom_spheres_double_download")
        nodes = np.zeros(nn.value, NODE_DBL_DTYPE); idx = np.zeros(ni.value, np.uint64); gathered = np.zeros((ni.value, 4), np.float64)
        check(lib.tbvh_custom_spheres_double_download(self._h, _ptr(nodes), nn.value, _ptr(idx), ni.value, _ptr(gathered), ni.value, None, None),
              "tbvh_custom_spheres_double_download")
        return nodes, idx, gathered

    @property
    def bounds(self) -> np.ndarray:
        """aabbMin, aabbMax of the root box (what BLASInstanceEx::Update reads from a BLAS)."""
        if self.spheres is None:   # device-resident spheres: the root as it is on the device
            n = C.c_uint64(0)
            check(lib.tbvh_double_download(self._h, None, 0, C.byref(n)), "tbvh_double_download")
            nodes = np.zeros(n.value, NODE_DBL_DTYPE)
            check(lib.tbvh_double_download(self._h, _ptr(nodes), n.value, None), "tbvh_double_download")
            return np.concatenate([nodes[0]["aabbMin"], nodes[0]["aabbMax"]])
        s = self.spheres
        return np.concatenate([(s[:, :3] - s[:, 3:4]).min(0), (s[:, :3] + s[:, 3:4]).max(0)])


# ---- voxel sets: VoxelSet (tiny_bvh.h:988-1030, 3772-4158) -----------------------------------------------------------------------------
VOXEL_OBJECT_DIM = 256   # VoxelSet::objectDim, the reference's compiled value (the only one supported)


def load_voxel_file(path: str) -> np.ndarray:
    """A voxel file of the reference's demos (tiny_bvh_voxel.cpp:44-48): gzip, a bvhint3 size, then size.x * size.y * size.z uint32 values
    values[x + y * size.x + z * size.x * size.y].  Returns them as a dense (z, y, x) uint32 array."""
    import gzip
    with gzip.open(path, "rb") as f:
        raw = f.read()
    size = np.frombuffer(raw[:12], "<i4")
    nx, ny, nz = (int(v) for v in size)
    n = nx * ny * nz
    assert nx > 0 and ny > 0 and nz > 0 and len(raw) >= 12 + 4 * n, "truncated voxel file"
    return np.frombuffer(raw[12:12 + 4 * n], "<u4").reshape(nz, ny, nx).copy()


class HostVoxelSet:
    """The three arrays of tbvh_host_build_voxelset: grid (32768 uint32), bricks (n_bricks x 512 uint32, brick 0 included), top grid (16 uint32)."""

    def __init__(self, h: C.c_void_p):
        self._h = h

    def _view(self, which: int) -> np.ndarray:
        p = lib.tbvh_host_blob(self._h, which)
        n = lib.tbvh_host_blob_count(self._h, which)
        if not p or n == 0:
            return np.zeros(0, np.uint32)
        return np.ctypeslib.as_array((C.c_uint32 * n).from_address(p)).copy()

    def arrays(self):
        return self._view(0), self._view(1), self._view(2)

    def __del__(self):
        try:
            if self._h:
                lib.tbvh_host_free(self._h)
                self._h = None
        except Exception:
            pass


def host_build_voxelset(dense: np.ndarray):
    """(grid, bricks, top) of a VoxelSet filled from a dense (z, y, x) uint32 array (0 = empty) in tiny_bvh_voxel.cpp's loop order, then
    UpdateTopGrid: the reference's arrays byte for byte (tbvh_host_build_voxelset)."""
    d = np.ascontiguousarray(dense, np.uint32)
    assert d.ndim == 3
    nz, ny, nx = d.shape
    h = C.c_void_p()
    check(lib.tbvh_host_build_voxelset(_ptr(d), nx, ny, nz, C.byref(h)), "tbvh_host_build_voxelset")
    return HostVoxelSet(h).arrays()


class VoxelSet(_Scene):
    """VoxelSet (tiny_bvh.h:988-1030) on the device: a 256^3 brick map over the unit cube, traced by a three-level DDA (kernels_voxel.hip).
    Set / UpdateTopGrid fill it on the host as the reference does; the first query (or Upload) puts it on the device.  Intersect / IsOccluded
    take the ordinary Ray records (RAY_DTYPE); a hit writes t, prim = the voxel's value and inst = instIdx, and is recorded only if it wins
    against the record's hit (DESIGN.md par. 10).  _bounds is the unit cube, so TLAS.Build takes voxel sets as BLASes (all of them voxel sets)."""
    layout = LAYOUT_VOXELSET

    def __init__(self, ctx: Context):
        super().__init__(ctx)
        self._bounds = np.array([0, 0, 0, 1, 1, 1], np.float32)
        self._dense = None     # Set() collects here (x, y, z, v), applied in call order
        self._pending = []

    def Set(self, x, y, z, v) -> "VoxelSet":
        """VoxelSet::Set (tiny_bvh.h:3786-3807) for scalars or equal-length arrays, applied in order (later calls win).  Takes effect on
        the device at UpdateTopGrid."""
        x, y, z, v = (np.atleast_1d(np.asarray(a)).astype(np.int64) for a in (x, y, z, v))
        x, y, z, v = np.broadcast_arrays(x, y, z, v)
        if x.size and (x.min() < 0 or y.min() < 0 or z.min() < 0 or max(x.max(), y.max(), z.max()) >= VOXEL_OBJECT_DIM):
            raise ValueError("voxel coordinates are 0..255")
        self._pending.append((x.ravel(), y.ravel(), z.ravel(), (v.ravel() & 0xFFFFFFFF).astype(np.uint32)))
        return self

    def UpdateTopGrid(self) -> "VoxelSet":
        """VoxelSet::UpdateTopGrid (tiny_bvh.h:3809-3827), and the (re-)upload of the set.  The brick numbering is that of a reference set
        filled in tiny_bvh_voxel.cpp's loop order (x outermost, z innermost), whatever order Set was called in."""
        if self._dense is None:
            self._dense = np.zeros((VOXEL_OBJECT_DIM,) * 3, np.uint32)
        for x, y, z, v in self._pending:
            self._dense[z, y, x] = v
        self._pending = []
        zz, yy, xx = np.nonzero(self._dense)
        ext = (int(xx.max()) + 1, int(yy.max()) + 1, int(zz.max()) + 1) if xx.size else (1, 1, 1)
        return self.Build(self._dense[:ext[2], :ext[1], :ext[0]])

    def Build(self, dense: np.ndarray) -> "VoxelSet":
        """Set every non-zero voxel of a dense (z, y, x) uint32 array (extents up to 256) and UpdateTopGrid, then upload."""
        grid, bricks, top = host_build_voxelset(dense)
        return self.Upload(grid, bricks, top)

    def Upload(self, grid: np.ndarray, bricks: np.ndarray, top: np.ndarray) -> "VoxelSet":
        """The reference's three arrays verbatim (tbvh_upload_voxelset): grid 32768 uint32, bricks n_bricks x 512 uint32 (brick 0 included;
        an unused pool tail may be left off), top grid 16 uint32."""
        grid = np.ascontiguousarray(grid, np.uint32).reshape(-1); bricks = np.ascontiguousarray(bricks, np.uint32).reshape(-1)
        top = np.ascontiguousarray(top, np.uint32).reshape(-1)
        assert grid.size == 32768 and top.size == 16 and bricks.size % 512 == 0
        if self._h:
            self.free()
            self._h = C.c_void_p()
        check(lib.tbvh_upload_voxelset(self.ctx._h, _ptr(grid), _ptr(bricks), bricks.size // 512, _ptr(top), C.byref(self._h)), "tbvh_upload_voxelset")
        self.arrays = (grid, bricks, top)
        return self

    # ---- editing on the device (capi_voxel_edit.hip, DESIGN.md par. 21): the set is changed where it lies, TLASes over it keep working ----------
    def CreateOnDevice(self, brick_capacity: int = 1024) -> "VoxelSet":
        """An empty set on the device as the reference's constructor leaves it (tbvh_voxelset_create): grid zero, freeBrickPtr = 1, top grid zero."""
        if self._h:
            self.free()
            self._h = C.c_void_p()
        check(lib.tbvh_voxelset_create(self.ctx._h, int(brick_capacity), C.byref(self._h)), "tbvh_voxelset_create")
        return self

    def Reserve(self, n_bricks: int) -> "VoxelSet":
        """Room for n_bricks bricks (brick 0 included) without another reallocation (tbvh_voxelset_reserve)."""
        check(lib.tbvh_voxelset_reserve(self._h, int(n_bricks)), "tbvh_voxelset_reserve")
        return self

    def Capacity(self):
        """(capacity, used) in bricks, brick 0 included (tbvh_voxelset_capacity)."""
        cap, used = C.c_uint64(0), C.c_uint64(0)
        check(lib.tbvh_voxelset_capacity(self._h, C.byref(cap), C.byref(used)), "tbvh_voxelset_capacity")
        return int(cap.value), int(used.value)

    def SetOnDevice(self, xyzv, n: int = None) -> "VoxelSet":
        """VoxelSet::Set for a batch of records {x, y, z, v}, the result that of calling Set on them in turn (tbvh_voxelset_set): an (n, 4) uint32 host
        array, or a device pointer (int) with n=.  The top grid follows at UpdateTopGridOnDevice, as in the reference."""
        if isinstance(xyzv, int):
            check(lib.tbvh_voxelset_set(self._h, C.c_void_p(xyzv), int(n), 1), "tbvh_voxelset_set")
            return self
        recs = np.ascontiguousarray(xyzv, np.uint32).reshape(-1, 4)
        check(lib.tbvh_voxelset_set(self._h, _ptr(recs), recs.shape[0], 0), "tbvh_voxelset_set")
        return self

    def UpdateTopGridOnDevice(self) -> "VoxelSet":
        """VoxelSet::UpdateTopGrid on the device (tbvh_voxelset_update_top_grid)."""
        check(lib.tbvh_voxelset_update_top_grid(self._h), "tbvh_voxelset_update_top_grid")
        return self

    def Arrays(self):
        """(grid, bricks[:used], top) as the device holds them now (tbvh_voxelset_download)."""
        n = C.c_uint64(0)
        check(lib.tbvh_voxelset_download(self._h, None, None, 0, None, C.byref(n)), "tbvh_voxelset_download")
        grid = np.zeros(32768, np.uint32); bricks = np.zeros(n.value * 512, np.uint32); top = np.zeros(16, np.uint32)
        check(lib.tbvh_voxelset_download(self._h, _ptr(grid), _ptr(bricks), n.value, _ptr(top), None), "tbvh_voxelset_download")
        return grid, bricks, top

    def Voxelize(self, scene, bmin, max_size, ext, shading=None, color: int = 0xFFFFFF, max_hits_per_ray: int = 4096) -> dict:
        """The scene-to-voxels loop of tiny_bvh_foliage.cpp:222-258 on the device (tbvh_voxelize_device): 3 x 256^2 axis rays marched through `scene` (a
        triangle BLAS or a TLAS over triangle BLASes), every opaque hit a Set on this set, then UpdateTopGrid.  bmin, max_size, ext: voxelize_bounds();
        shading: a Shading table (alpha 0 skips a hit, the albedo is the value) or None (every hit gets `color`).  Returns the statistics."""
        from ._capi import VoxelizeParams, VoxelizeStats
        p = VoxelizeParams((C.c_float * 3)(*[float(v) for v in bmin]), float(max_size), (C.c_float * 3)(*[float(v) for v in ext]), int(color), int(max_hits_per_ray))
        st = VoxelizeStats()
        check(lib.tbvh_voxelize_device(scene._h, shading._h if shading is not None else None, C.byref(p), self._h, C.byref(st)), "tbvh_voxelize_device")
        return {"rounds": int(st.rounds), "records": int(st.records), "rays_cut": int(st.rays_cut), "bricks": int(st.bricks)}

    def Normals(self, rays, n: int = None, d_out: int = 0, stride: int = 64):
        """VoxelSet::GetNormal for a batch of hit records (tbvh_voxel_normals): a RAY_DTYPE host array -> an (n, 4) float32 array {nx, ny, nz, 0}
        (zeros for a miss), or a device pointer (int) with n= and d_out= (tbvh_voxel_normals_device)."""
        return voxel_normals(self.ctx, self, rays, n, d_out, stride)


def voxelize_bounds(bounds6):
    """The bounding cube of tiny_bvh_foliage.cpp:216-220 from scene bounds (min xyz, max xyz): (bmin, maxSize, ext) with ext = bmax - bmin,
    maxSize its largest component and bmin = c - 0.525 * maxSize, in fp32, every product and sum rounded."""
    b = np.asarray(bounds6, np.float32).reshape(6)
    lo, hi = b[:3], b[3:]
    ext = (hi - lo).astype(np.float32)
    c = ((hi + lo) * np.float32(0.5)).astype(np.float32)
    m = np.float32(ext[1] if ext[1] > ext[0] else ext[0])
    if ext[2] > m:
        m = np.float32(ext[2])
    return (c - np.float32(0.525) * m).astype(np.float32), m, ext


def voxelize_matrix(bmin, max_size) -> np.ndarray:
    """The demo's matrix T (tiny_bvh_foliage.cpp:256-262), row-major 4 x 4: world space into the voxel object's unit cube."""
    s = np.float32(1.0) / np.float32(max_size)
    T = np.zeros((4, 4), np.float32)
    T[0, 0] = T[1, 1] = T[2, 2] = s
    T[:3, 3] = -np.asarray(bmin, np.float32) * s
    T[3, 3] = 1
    return T


def voxel_normals(ctx: Context, scene, rays, n: int = None, d_out: int = 0, stride: int = 64):
    """GetNormal for hit records of one voxel set (scene None or a VoxelSet) or of a TLAS over voxel sets, whose normals come back in the hit
    instance's object space (tbvh_voxel_normals / tbvh_voxel_normals_device; see VoxelSet.Normals)."""
    h = scene._h if scene is not None else None
    if isinstance(rays, int):
        check(lib.tbvh_voxel_normals_device(ctx._h, h, C.c_void_p(rays), int(stride), int(n), C.c_void_p(d_out)), "tbvh_voxel_normals_device")
        return d_out
    rays = np.ascontiguousarray(rays)
    out = np.zeros((rays.shape[0], 4), np.float32)
    check(lib.tbvh_voxel_normals(ctx._h, h, _ptr(rays), rays.dtype.itemsize, rays.shape[0], _ptr(out)), "tbvh_voxel_normals")
    return out


def host_voxel_normals(rays, instances=None):
    """The CPU twin of voxel_normals (tbvh_host_voxel_normals): instances = the TLAS's BLASInstance records, or None for one set."""
    rays = np.ascontiguousarray(rays)
    out = np.zeros((rays.shape[0], 4), np.float32)
    inst = None if instances is None else np.ascontiguousarray(instances)
    check(lib.tbvh_host_voxel_normals(None if inst is None else _ptr(inst), 0 if inst is None else inst.shape[0], _ptr(rays), rays.dtype.itemsize, rays.shape[0],
                                      _ptr(out)), "tbvh_host_voxel_normals")
    return out


class HostVoxelEdit(HostVoxelSet):
    """The CPU twin of the device editing calls: an empty set (the reference's constructor) or a copy of given arrays, Set per record in turn,
    UpdateTopGrid (tbvh_host_voxelset_create / _set / _update_top_grid); arrays() are its grid, used bricks and top grid."""

    def __init__(self):
        h = C.c_void_p()
        check(lib.tbvh_host_voxelset_create(C.byref(h)), "tbvh_host_voxelset_create")
        super().__init__(h)

    def Set(self, xyzv) -> "HostVoxelEdit":
        recs = np.ascontiguousarray(xyzv, np.uint32).reshape(-1, 4)
        check(lib.tbvh_host_voxelset_set(self._h, _ptr(recs), recs.shape[0]), "tbvh_host_voxelset_set")
        return self

    def UpdateTopGrid(self) -> "HostVoxelEdit":
        check(lib.tbvh_host_voxelset_update_top_grid(self._h), "tbvh_host_voxelset_update_top_grid")
        return self


# ---- custom geometry: sphere BLASes (BVH::Build( customGetAABB, n ) + the anim demo's sphere callback) ----------------------------------------
def host_build_custom_spheres(spheres: np.ndarray):
    """(nodes32 as (n, 8) uint32, prim_idx) of the library's BVH over the boxes pos -/+ r of spheres {x, y, z, r} (tbvh_host_build_custom_spheres)."""
    sph = np.ascontiguousarray(spheres, np.float32).reshape(-1, 4)
    h = C.c_void_p()
    check(lib.tbvh_host_build_custom_spheres(_ptr(sph), sph.shape[0], C.byref(h)), "tbvh_host_build_custom_spheres")
    try:
        out = []
        for which, width in ((0, 8), (1, 1)):
            n = int(lib.tbvh_host_blob_count(h, which))
            p = lib.tbvh_host_blob(h, which)
            a = np.ctypeslib.as_array((C.c_uint32 * (n * width)).from_address(p)).copy()
            out.append(a.reshape(n, width) if width > 1 else a)
    finally:
        lib.tbvh_host_free(h)
    return out[0], out[1]


class SphereBVH(_Scene):
    """A BVH over custom geometry (BVH::Build( customGetAABB, n ), tiny_bvh.h:2190-2219) whose primitives are spheres {x, y, z, r}, traced on
    the device with the sphere callback of the reference's anim demo (kernels_custom.hip, DESIGN.md par. 12).  Intersect / IsOccluded take the
    ordinary Ray records (RAY_DTYPE); a hit writes t, prim and inst = instIdx and leaves u, v as they were.  _bounds is the root box, so
    TLAS.Build / Upload / RebuildOnDevice take it as a BLAS, alone or next to triangle BLASes."""
    layout = LAYOUT_BVH2_WALD

    def Build(self, spheres: np.ndarray) -> "SphereBVH":
        """The library's host builder over the boxes pos -/+ r, then Upload."""
        nodes, prim_idx = host_build_custom_spheres(spheres)
        return self.Upload(nodes, prim_idx, spheres)

    def Upload(self, nodes32: np.ndarray, prim_idx: np.ndarray, spheres: np.ndarray) -> "SphereBVH":
        """The reference's own arrays: BVH::bvhNode (32-byte Wald nodes, usedNodes of them), BVH::primIdx (idxCount) and the spheres
        {x, y, z, r} by primitive index (tbvh_upload_custom_spheres: validated before anything is allocated)."""
        nodes32 = np.ascontiguousarray(nodes32).view(np.uint32).reshape(-1, 8)
        prim_idx = np.ascontiguousarray(prim_idx, np.uint32).reshape(-1)
        spheres = np.ascontiguousarray(spheres, np.float32).reshape(-1, 4)
        if self._h:
            self.free()
            self._h = C.c_void_p()
        check(lib.tbvh_upload_custom_spheres(self.ctx._h, _ptr(nodes32), nodes32.shape[0], _ptr(prim_idx), prim_idx.size, _ptr(spheres),
                                             spheres.shape[0], C.byref(self._h)), "tbvh_upload_custom_spheres")
        self.nodes, self.prim_idx, self.spheres = nodes32, prim_idx, spheres
        self._bounds = np.concatenate([nodes32[0, 0:3].view(np.float32), nodes32[0, 4:7].view(np.float32)]).astype(np.float32)
        return self

    # ---- sphere sets that move: build, rebuild and refit on the device (tbvh_build_device_custom_spheres and its neighbours) ----
    @staticmethod
    def _sphere_arg(spheres):
        """(pointer, n, on_device, keep-alive) of a numpy array of {x, y, z, r} or a (device_pointer, n) pair"""
        if isinstance(spheres, tuple):
            return C.c_void_p(int(spheres[0])), int(spheres[1]), 1, None
        a = np.ascontiguousarray(spheres, np.float32).reshape(-1, 4)
        return _ptr(a), a.shape[0], 0, a

    def _after_device_call(self, host_spheres) -> "SphereBVH":
        """_bounds = the new root box (24 bytes read back), so that TLAS.Build / RebuildOnDevice take the scene as a BLAS; the host mirrors
        (nodes, prim_idx) are stale until Download()."""
        b = np.zeros(6, np.float32)
        check(lib.tbvh_custom_spheres_bounds(self._h, _ptr(b)), "tbvh_custom_spheres_bounds")
        self._bounds = b
        self.nodes = self.prim_idx = None
        if host_spheres is not None:
            self.spheres = host_spheres
        return self

    def BuildOnDevice(self, spheres, builder: str = "lbvh", max_leaf: int = 0, radius: int = 0) -> "SphereBVH":
        """LBVH (max_leaf 1..4 spheres per leaf, 0 = 1) or PLOC (radius 1..32, 0 = 16) over the boxes pos -/+ r, on the device
        (tbvh_build_device_custom_spheres), or builder="sah": the reference's own BVH::Build( customGetAABB, n ) tree (max_leaf 0 = its leaves,
        1..4 = SplitLeafs; tbvh_build_device_custom_spheres_sah).  spheres: a numpy array or a (device_pointer, n) pair."""
        ptr, n, on_device, keep = self._sphere_arg(spheres)
        if builder not in ("lbvh", "ploc", "sah"):
            raise ValueError(f"SphereBVH.BuildOnDevice: builder {builder!r} (lbvh, ploc or sah)")
        if self._h:
            self.free()
            self._h = C.c_void_p()
        if builder == "sah":
            check(lib.tbvh_build_device_custom_spheres_sah(self.ctx._h, ptr, n, on_device, int(max_leaf), C.byref(self._h)), "tbvh_build_device_custom_spheres_sah")
            return self._after_device_call(keep)
        check(lib.tbvh_build_device_custom_spheres(self.ctx._h, ptr, n, on_device, {"lbvh": 0, "ploc": 1}[builder], int(max_leaf), int(radius),
                                                   C.byref(self._h)), "tbvh_build_device_custom_spheres")
        return self._after_device_call(keep)

    def RebuildOnDevice(self, spheres) -> "SphereBVH":
        """A new tree over moved spheres in the same scene, with the builder it remembers (tbvh_rebuild_custom_spheres_device); a TLAS over
        it needs no new upload, only its RebuildOnDevice() for the instance boxes."""
        ptr, n, on_device, keep = self._sphere_arg(spheres)
        check(lib.tbvh_rebuild_custom_spheres_device(self._h, ptr, n, on_device), "tbvh_rebuild_custom_spheres_device")
        return self._after_device_call(keep)

    def Refit(self, spheres, on_device: bool = False) -> "SphereBVH":
        """Same topology, new boxes and records (tbvh_refit_custom_spheres).  spheres: a numpy array, a (device_pointer, n) pair, or with
        on_device=True a device pointer to as many spheres as the scene holds."""
        if on_device and not isinstance(spheres, tuple):
            spheres = (int(spheres), self.spheres.shape[0])
        ptr, n, dev, keep = self._sphere_arg(spheres)
        check(lib.tbvh_refit_custom_spheres(self._h, ptr, n, dev), "tbvh_refit_custom_spheres")
        return self._after_device_call(keep)

    def Download(self):
        """(nodes32 as (n, 8) uint32, prim_idx, the gathered spheres in prim_idx order) as they are on the device now
        (tbvh_custom_spheres_download); fills self.nodes / self.prim_idx."""
        nn, ni = C.c_uint64(0), C.c_uint64(0)
        check(lib.tbvh_custom_spheres_download(self._h, None, 0, None, 0, None, 0, C.byref(nn), C.byref(ni)), "tbvh_custom_spheres_download")
        nodes = np.zeros((nn.value, 8), np.uint32); idx = np.zeros(ni.value, np.uint32); gathered = np.zeros((ni.value, 4), np.float32)
        check(lib.tbvh_custom_spheres_download(self._h, _ptr(nodes), nn.value, _ptr(idx), ni.value, _ptr(gathered), ni.value, C.byref(nn), C.byref(ni)),
              "tbvh_custom_spheres_download")
        self.nodes, self.prim_idx = nodes, idx
        return nodes, idx, gathered


# ---- opacity micromaps baked from alpha textures (capi_omm.hip) ---------------------------------------------------------------------------
OMM_NO_TEXTURE = 0xFFFFFFFF


def _alpha_texels(tex) -> np.ndarray:
    """(h, w) uint32 texels, alpha in bits 24-31, from an (h, w) uint32 array (used in place when packed) or an (h, w, 4) uint8 RGBA array"""
    t = np.asarray(tex)
    if t.ndim == 3 and t.shape[2] == 4 and t.dtype == np.uint8:
        return np.ascontiguousarray(t).view("<u4").reshape(t.shape[0], t.shape[1])   # (bytes R, G, B, A: A is the top byte of the little-endian word)
    assert t.ndim == 2 and t.dtype == np.uint32, "a texture: (h, w) uint32 or (h, w, 4) uint8"
    return np.ascontiguousarray(t)


def device_omm_source(d_uv: int, n_uv: int, n_tris: int, textures, d_indices: int = 0, d_tri_texture: int = 0, uv_stride_bytes: int = 8) -> OmmSource:
    """A tbvh_omm_source whose arrays are device memory; textures: a list of (device pointer, width, height).  Pass it as `uv` of the bake calls."""
    arr = (AlphaTexture * max(len(textures), 1))(*[AlphaTexture(C.c_void_p(int(p)), int(w), int(h)) for p, w, h in textures])
    src = OmmSource(C.c_void_p(int(d_uv)), int(n_uv), int(uv_stride_bytes), 1, C.c_void_p(int(d_indices)) if d_indices else None, int(n_tris),
                    C.c_void_p(int(d_tri_texture)) if d_tri_texture else None, arr, len(textures))
    src._keep = arr
    return src


def _omm_source(uv, textures=None, indices=None, tri_texture=None):
    """(tbvh_omm_source, the arrays it points into) for host arrays: uv any float32 array of shape (n_uv, k >= 2) whose row stride is a multiple of 4 — the
    stride is ndarray.strides[0], so interleaved[:, 3:5] is used in place —, textures one texture or a list of them ((h, w) uint32 or (h, w, 4) uint8 RGBA),
    indices (n_tris, 3) or flat uint32 or None (triangle i = UVs 3i, 3i + 1, 3i + 2), tri_texture (n_tris,) uint32 (OMM_NO_TEXTURE: opaque) or None (texture 0).
    An OmmSource made by device_omm_source() passes through."""
    if isinstance(uv, OmmSource):
        assert textures is None and indices is None and tri_texture is None, "a device_omm_source() carries its own arrays"
        return uv, ()
    v = np.asarray(uv)
    if v.dtype != np.float32 or v.ndim != 2 or v.shape[1] < 2 or v.strides[1] != 4 or v.strides[0] % 4 or v.strides[0] < 8:
        v = np.ascontiguousarray(v, np.float32)
        assert v.ndim == 2 and v.shape[1] >= 2, "uv: (n_uv, k >= 2) float32"
    if isinstance(textures, np.ndarray) and (textures.ndim == 2 or (textures.ndim == 3 and textures.dtype == np.uint8)):
        textures = [textures]
    tex = [_alpha_texels(t) for t in (textures or [])]
    arr = (AlphaTexture * max(len(tex), 1))(*[AlphaTexture(C.c_void_p(t.ctypes.data), t.shape[1], t.shape[0]) for t in tex])
    idx = tt = None
    if indices is not None:
        idx = np.ascontiguousarray(indices, np.uint32).reshape(-1)
        assert idx.size % 3 == 0
        n_tris = idx.size // 3
    else:
        n_tris = v.shape[0] // 3
    if tri_texture is not None:
        tt = np.ascontiguousarray(tri_texture, np.uint32).reshape(-1)
        assert tt.size == n_tris, "tri_texture: one per triangle"
    src = OmmSource(C.c_void_p(v.ctypes.data), v.shape[0], v.strides[0], 0, None if idx is None else C.c_void_p(idx.ctypes.data), n_tris,
                    None if tt is None else C.c_void_p(tt.ctypes.data), arr, len(tex))
    return src, (v, idx, tt, tex, arr)


def omm_words(N: int) -> int:
    return (N * N + 31) // 32


def host_bake_opacity_micromaps(uv, textures, N: int = 32, indices=None, tri_texture=None) -> np.ndarray:
    """Mesh::CreateOpacityMicroMaps( N ) on the CPU (tbvh_host_bake_opacity_micromaps): the (n_tris, (N * N + 31) // 32) uint32 words."""
    src, keep = _omm_source(uv, textures, indices, tri_texture)
    out = np.zeros((int(src.n_tris), omm_words(N) if N > 0 else 1), np.uint32)
    check(lib.tbvh_host_bake_opacity_micromaps(C.byref(src), N, _ptr(out)), "tbvh_host_bake_opacity_micromaps")
    del keep
    return out


def bake_opacity_micromaps(ctx: "Context", uv, textures=None, N: int = 32, indices=None, tri_texture=None, d_out: int = 0):
    """The same on the device (tbvh_bake_opacity_micromaps).  d_out == 0: the words come back as an (n_tris, words) array; otherwise they stay in device memory at
    d_out (asynchronous for a device_omm_source()) and nothing is returned."""
    src, keep = _omm_source(uv, textures, indices, tri_texture)
    if d_out:
        check(lib.tbvh_bake_opacity_micromaps(ctx._h, C.byref(src), N, C.c_void_p(int(d_out))), "tbvh_bake_opacity_micromaps")
        del keep
        return None
    out = np.zeros((int(src.n_tris), omm_words(N) if N > 0 else 1), np.uint32)
    d = ctx.malloc(max(out.nbytes, 4))
    try:
        check(lib.tbvh_bake_opacity_micromaps(ctx._h, C.byref(src), N, C.c_void_p(d)), "tbvh_bake_opacity_micromaps")
        ctx.from_device(out, d)
    finally:
        ctx.free(d)
    del keep
    return out


# ---- skinned / morph-target meshes posed on the device (capi_pose.hip) -------------------------------------------------------------------
def _skin_arrays(rest, joints, weights):
    rest = np.asarray(rest, np.float32)
    if rest.ndim == 2 and rest.shape[1] == 3:   # (n, 3) positions: the bvhvec4 array the library takes, w = 0 (not read)
        rest = np.concatenate([rest, np.zeros((rest.shape[0], 1), np.float32)], 1)
    rest = np.ascontiguousarray(rest, np.float32).reshape(-1, 4)
    joints = np.ascontiguousarray(joints, np.uint32).reshape(-1, 4)
    weights = np.ascontiguousarray(weights, np.float32).reshape(-1, 4)
    assert rest.shape[0] == joints.shape[0] == weights.shape[0], "rest, joints and weights: one row of 4 per vertex"
    return rest, joints, weights


def host_pose_skin(rest, joints, weights, joint_mats) -> np.ndarray:
    """Mesh::SetPose( skin ) on the CPU (tbvh_host_pose_skin): the (n_verts, 4) posed vertices, w = 0.  joint_mats: (n_joints, 16) or (n_joints, 4, 4),
    row-major."""
    rest, joints, weights = _skin_arrays(rest, joints, weights)
    mats = np.ascontiguousarray(joint_mats, np.float32).reshape(-1, 16)
    out = np.zeros((rest.shape[0], 4), np.float32)
    check(lib.tbvh_host_pose_skin(_ptr(rest), rest.shape[0], _ptr(joints), _ptr(weights), _ptr(mats), mats.shape[0], _ptr(out)), "tbvh_host_pose_skin")
    return out


def host_pose_morph(positions, weights) -> np.ndarray:
    """Mesh::SetPose( weights ) on the CPU (tbvh_host_pose_morph): positions (n_targets + 1, n_verts, 3), pose 0 the base; the (n_verts, 4) posed
    vertices, w = 1."""
    pos = np.ascontiguousarray(positions, np.float32)
    assert pos.ndim == 3 and pos.shape[2] == 3, "positions: (n_targets + 1, n_verts, 3)"
    w = np.ascontiguousarray(weights, np.float32).reshape(-1)
    out = np.zeros((pos.shape[1], 4), np.float32)
    check(lib.tbvh_host_pose_morph(_ptr(pos), pos.shape[1], w.size, _ptr(w) if w.size else None, _ptr(out)), "tbvh_host_pose_morph")
    return out


def host_pose_fat_tris(fat_tris, verts16, normals16, indices=None, skin: bool = True) -> np.ndarray:
    """The FatTri half of Mesh::SetPose on the CPU (tbvh_host_pose_update_fat_tris): a copy of fat_tris (FATTRI_DTYPE) rewritten from posed vertices
    (host_pose_skin / host_pose_morph) and posed normals (host_pose_skin_normals / host_pose_morph_normals), both (n_verts, 4)."""
    f = np.array(fat_tris, FATTRI_DTYPE).reshape(-1)
    v = np.ascontiguousarray(verts16, np.float32).reshape(-1, 4); n = np.ascontiguousarray(normals16, np.float32).reshape(-1, 4)
    assert v.shape == n.shape
    idx = None if indices is None else np.ascontiguousarray(indices, np.uint32).reshape(-1, 3)
    check(lib.tbvh_host_pose_update_fat_tris(_ptr(f), f.size, _ptr(v), _ptr(n), v.shape[0], None if idx is None else _ptr(idx), 1 if skin else 0), "tbvh_host_pose_update_fat_tris")
    return f


def host_pose_skin_normals(normals, joints, weights, joint_mats) -> np.ndarray:
    """(n_verts, 4) posed normals of a skin pose (tbvh_host_pose_skin_normals): normalize( transform_vector( normal, the vertex's blended matrix ) ), w = 0"""
    nrm = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    _, joints, weights = _skin_arrays(np.zeros((nrm.shape[0], 4), np.float32), joints, weights)
    mats = np.ascontiguousarray(joint_mats, np.float32).reshape(-1, 16)
    out = np.zeros((nrm.shape[0], 4), np.float32)
    check(lib.tbvh_host_pose_skin_normals(nrm.shape[0], _ptr(joints), _ptr(weights), _ptr(mats), mats.shape[0], _ptr(nrm), _ptr(out)), "tbvh_host_pose_skin_normals")
    return out


def host_pose_morph_normals(normals) -> np.ndarray:
    """(n_verts, 4) normals of a morph pose (tbvh_host_pose_morph_normals): normalize( base + the target normals ), no weights, as the reference has it"""
    nrm = np.ascontiguousarray(normals, np.float32)
    assert nrm.ndim == 3 and nrm.shape[2] == 3, "normals: (n_targets + 1, n_verts, 3)"
    out = np.zeros((nrm.shape[1], 4), np.float32)
    check(lib.tbvh_host_pose_morph_normals(_ptr(nrm), nrm.shape[1], nrm.shape[0] - 1, _ptr(out)), "tbvh_host_pose_morph_normals")
    return out


class Pose:
    """A skinned or morph-target mesh posed on the device (tbvh_pose_*; Mesh::SetPose of tiny_scene.h): Skin() or Morph() once, then per frame
    SetPose( joint matrices | morph weights ) and Refit( scene )."""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self._h = C.c_void_p()
        self.kind = None
        self.n_verts = 0

    def Skin(self, rest, joints, weights, n_joints: int) -> "Pose":
        """rest (n_verts, 4) or (n_verts, 3), joints (n_verts, 4) uint32, weights (n_verts, 4); n_verts counts VERTICES (shared ones once)."""
        assert not self._h, "this Pose is already made"
        rest, joints, weights = _skin_arrays(rest, joints, weights)
        check(lib.tbvh_pose_create_skin(self.ctx._h, _ptr(rest), rest.shape[0], _ptr(joints), _ptr(weights), int(n_joints), 0, C.byref(self._h)), "tbvh_pose_create_skin")
        self.kind, self.n_verts, self.n_params = "skin", rest.shape[0], int(n_joints)
        return self

    def SkinOnDevice(self, d_rest: int, d_joints: int, d_weights: int, n_verts: int, n_joints: int) -> "Pose":
        """The same from device-resident arrays (copied; the joint indices are then checked by the kernel)."""
        assert not self._h, "this Pose is already made"
        check(lib.tbvh_pose_create_skin(self.ctx._h, C.c_void_p(d_rest), n_verts, C.c_void_p(d_joints), C.c_void_p(d_weights), int(n_joints), 1, C.byref(self._h)),
              "tbvh_pose_create_skin")
        self.kind, self.n_verts, self.n_params = "skin", int(n_verts), int(n_joints)
        return self

    def Morph(self, positions) -> "Pose":
        """positions (n_targets + 1, n_verts, 3): pose 0 is the base."""
        assert not self._h, "this Pose is already made"
        pos = np.ascontiguousarray(positions, np.float32)
        assert pos.ndim == 3 and pos.shape[2] == 3 and pos.shape[0] >= 1, "positions: (n_targets + 1, n_verts, 3)"
        check(lib.tbvh_pose_create_morph(self.ctx._h, _ptr(pos), pos.shape[1], pos.shape[0] - 1, 0, C.byref(self._h)), "tbvh_pose_create_morph")
        self.kind, self.n_verts, self.n_params = "morph", pos.shape[1], pos.shape[0] - 1
        return self

    def SetPose(self, params, on_device: bool = False) -> "Pose":
        """Skin: the joint matrices, (n_joints, 16) or (n_joints, 4, 4) row-major; morph: the n_targets weights.  on_device: params is a device
        pointer to that many.  Asynchronous; a host array may be reused on return."""
        skin = self.kind == "skin"
        if on_device:
            ptr, n = C.c_void_p(int(params)), self.n_params
        else:
            a = np.ascontiguousarray(params, np.float32)
            a = a.reshape(-1, 16) if skin else a.reshape(-1)
            ptr, n = (_ptr(a) if a.size else None), a.shape[0]
        if skin:
            check(lib.tbvh_pose_set_skin(self._h, ptr, n, 1 if on_device else 0), "tbvh_pose_set_skin")
        else:
            check(lib.tbvh_pose_set_morph(self._h, ptr, n, 1 if on_device else 0), "tbvh_pose_set_morph")
        return self

    def Refit(self, scene: "_Scene") -> "Pose":
        """tbvh_pose_refit: refit `scene` from the posed vertices (through the scene's own index buffer when it holds one)."""
        check(lib.tbvh_pose_refit(self._h, scene._h), "tbvh_pose_refit")
        return self

    def AttachFatTris(self, shading: "Shading", slot: int, normals, indices=None) -> "Pose":
        """tbvh_pose_attach_fat_tris: from now on every SetPose also rewrites the FatTri records of `slot` of `shading` (vertex0..2, vN0..2 and, for a skin,
        Nx Ny Nz).  normals: skin (n_verts, 3) rest normals, morph (n_targets + 1, n_verts, 3); indices: (n_tris, 3) for an indexed pose."""
        nrm = np.ascontiguousarray(normals, np.float32)
        want = self.n_verts * 3 * (self.n_params + 1 if self.kind == "morph" else 1)
        assert nrm.size == want, "normals: (n_verts, 3) for a skin, (n_targets + 1, n_verts, 3) for a morph pose"
        idx = None if indices is None else np.ascontiguousarray(indices, np.uint32).reshape(-1, 3)
        n_tris = self.n_verts // 3 if idx is None else idx.shape[0]
        check(lib.tbvh_pose_attach_fat_tris(self._h, shading._h, int(slot), _ptr(nrm), None if idx is None else _ptr(idx), n_tris, 0), "tbvh_pose_attach_fat_tris")
        return self

    def Vertices(self):
        """(device pointer of the posed vertices, n_verts)"""
        p = C.c_void_p(); n = C.c_uint64(0)
        check(lib.tbvh_pose_vertices(self._h, C.byref(p), C.byref(n)), "tbvh_pose_vertices")
        return p.value, int(n.value)

    def Download(self) -> np.ndarray:
        out = np.zeros((self.n_verts, 4), np.float32)
        check(lib.tbvh_pose_download(self._h, _ptr(out), self.n_verts), "tbvh_pose_download")
        return out

    def free(self):
        if self._h and self.ctx._h:   # (a closed context has freed its poses itself: tbvh_shutdown)
            lib.tbvh_pose_free(self._h)
        self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# ---- the animated scene graph (capi_scenegraph.hip, scenegraph_host.cpp) ------------------------------------------------------------------
SCENEGRAPH_FRESH_JOINTS = 1
GRAPH_LINEAR, GRAPH_SPLINE, GRAPH_STEP = 0, 1, 2
GRAPH_VEC3, GRAPH_QUAT, GRAPH_FLOAT = 0, 1, 2
GRAPH_TRS, GRAPH_LOCAL, GRAPH_COMBINED, GRAPH_CHANNEL_T, GRAPH_CHANNEL_K, GRAPH_INSTANCES, GRAPH_JOINTS, GRAPH_WEIGHTS, GRAPH_STALE, GRAPH_TRIG = range(10)
_GRAPH_ARRAYS = (("parent", np.int32), ("visit_order", np.uint32), ("translation", np.float32), ("rotation", np.float32), ("scale", np.float32), ("matrix", np.float32),
                 ("local_transform", np.float32), ("n_weights", np.uint32), ("weights", np.float32), ("sampler_interpolation", np.uint32), ("sampler_type", np.uint32),
                 ("sampler_key_offset", np.uint32), ("sampler_value_offset", np.uint32), ("key_times", np.float32), ("key_values", np.float32),
                 ("channel_animation", np.uint32), ("channel_sampler", np.uint32), ("channel_node", np.uint32), ("channel_target", np.uint32),
                 ("node_of_instance", np.uint32), ("skin_mesh_node", np.uint32), ("skin_joint_offset", np.uint32), ("skin_joint_node", np.uint32),
                 ("skin_inverse_bind", np.float32))


def scenegraph_desc(d: dict):
    """tbvh_scenegraph_desc from a dict of arrays named as the struct's members (missing or None: NULL), plus "flags" and "n_animations".  The counts come
    from the arrays: parent (nodes), sampler_interpolation, channel_node, node_of_instance, skin_mesh_node.  Returns (struct, the arrays it points into)."""
    keep = {}
    desc = _capi.SceneGraphDesc()
    for name, dt in _GRAPH_ARRAYS:
        a = d.get(name)
        if a is None:
            continue
        keep[name] = a = np.ascontiguousarray(a, dt).reshape(-1)
        setattr(desc, name, a.ctypes.data if a.size else None)
    n = lambda k: keep[k].size if k in keep else 0
    desc.flags = int(d.get("flags", 0))
    desc.n_nodes, desc.n_samplers, desc.n_channels, desc.n_instances, desc.n_skin_uses = n("parent"), n("sampler_interpolation"), n("channel_node"), n("node_of_instance"), n("skin_mesh_node")
    desc.n_animations = int(d.get("n_animations", (int(keep["channel_animation"].max()) + 1) if n("channel_animation") else 0))
    return desc, keep


class _GraphBase:
    """What SceneGraph (device) and HostSceneGraph (CPU) share: the calls differ in their prefix and in where the output pointers live."""
    _prefix = ""

    def _fn(self, name):
        return getattr(lib, self._prefix + name)

    def _made(self, keep):
        n = lambda k: keep[k].size if k in keep else 0
        self.n_nodes, self.n_channels, self.n_instances, self.n_skin_uses = n("parent"), n("channel_node"), n("node_of_instance"), n("skin_mesh_node")
        self.n_joints = int(keep["skin_joint_offset"][-1]) if self.n_skin_uses else 0
        self.n_weights = int(keep["n_weights"].sum()) if "n_weights" in keep else 0

    def Advance(self, dt: float):
        """Scene::UpdateSceneGraph( dt ) without the BLAS / TLAS builds"""
        check(self._fn("advance")(self._h, float(dt)), self._prefix + "advance")
        return self

    def AdvanceAnimation(self, animation: int, dt: float):
        check(self._fn("advance_animation")(self._h, int(animation), float(dt)), self._prefix + "advance_animation")
        return self

    def UpdateNodes(self):
        check(self._fn("update_nodes")(self._h), self._prefix + "update_nodes")
        return self

    def SetTime(self, animation: int, t: float):
        check(self._fn("set_time")(self._h, int(animation), float(t)), self._prefix + "set_time")
        return self

    def Reset(self, animation: int):
        check(self._fn("reset")(self._h, int(animation)), self._prefix + "reset")
        return self

    def SetLocal(self, node: int, mat16):
        m = np.ascontiguousarray(mat16, np.float32).reshape(16)
        check(self._fn("set_local")(self._h, int(node), _ptr(m)), self._prefix + "set_local")
        return self

    def InstanceTransforms(self):
        """(pointer to n_instances x 16 floats, n_instances): feeds TLAS.RebuildOnDevice( ptr, on_device=True )"""
        p = C.c_void_p(); n = C.c_uint64(0)
        check(self._fn("instance_transforms")(self._h, C.byref(p), C.byref(n)), self._prefix + "instance_transforms")
        return p.value, int(n.value)

    def JointMatrices(self, skin_use: int):
        """(pointer to n_joints x 16 floats, n_joints) of one skin use: feeds Pose.SetPose( ptr, on_device=True )"""
        p = C.c_void_p(); n = C.c_uint32(0)
        check(self._fn("joint_matrices")(self._h, int(skin_use), C.byref(p), C.byref(n)), self._prefix + "joint_matrices")
        return p.value, int(n.value)

    def MorphWeights(self, node: int):
        """(pointer to the node's morph weights, their number): feeds a morph Pose.SetPose( ptr, on_device=True )"""
        p = C.c_void_p(); n = C.c_uint32(0)
        check(self._fn("morph_weights")(self._h, int(node), C.byref(p), C.byref(n)), self._prefix + "morph_weights")
        return p.value, int(n.value)

    def Download(self, what: int) -> np.ndarray:
        """GRAPH_TRS (n, 10), GRAPH_LOCAL / GRAPH_COMBINED (n, 16), GRAPH_CHANNEL_T / _K (channels,), GRAPH_INSTANCES (instances, 16), GRAPH_JOINTS (joints, 16),
        GRAPH_WEIGHTS, GRAPH_STALE (joints,), GRAPH_TRIG (channels,).  Synchronous; raises for a device-detected bad index."""
        shape, dt = {GRAPH_TRS: ((self.n_nodes, 10), np.float32), GRAPH_LOCAL: ((self.n_nodes, 16), np.float32), GRAPH_COMBINED: ((self.n_nodes, 16), np.float32),
                     GRAPH_CHANNEL_T: ((self.n_channels,), np.float32), GRAPH_CHANNEL_K: ((self.n_channels,), np.int32), GRAPH_INSTANCES: ((self.n_instances, 16), np.float32),
                     GRAPH_JOINTS: ((self.n_joints, 16), np.float32), GRAPH_WEIGHTS: ((self.n_weights,), np.float32), GRAPH_STALE: ((self.n_joints,), np.uint32),
                     GRAPH_TRIG: ((self.n_channels,), np.uint32)}[what]
        out = np.zeros(shape, dt)
        buf = out if out.size else np.zeros(1, dt)
        check(self._fn("download")(self._h, int(what), _ptr(buf), out.nbytes), self._prefix + "download")
        return out


class SceneGraph(_GraphBase):
    """An animated scene graph kept on the device (tbvh_scenegraph_*; Scene::UpdateSceneGraph of tiny_scene.h): made once from a dict of arrays
    (scenegraph_desc), then per frame Advance( dt ); the instance transforms, joint matrices and morph weights stay in device memory."""
    _prefix = "tbvh_scenegraph_"

    def __init__(self, ctx: Context, desc: dict):
        self.ctx = ctx
        self._h = C.c_void_p()
        st, keep = scenegraph_desc(desc)
        check(lib.tbvh_scenegraph_create(ctx._h, C.byref(st), C.byref(self._h)), "tbvh_scenegraph_create")
        self._made(keep)

    def free(self):
        if self._h and self.ctx._h:   # (a closed context has freed its graphs itself: tbvh_shutdown)
            lib.tbvh_scenegraph_free(self._h)
        self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class HostSceneGraph(_GraphBase):
    """The same object on the CPU (tbvh_host_scenegraph_*): the same arithmetic header compiled for the host, no context."""
    _prefix = "tbvh_host_scenegraph_"

    def __init__(self, desc: dict):
        self._h = C.c_void_p()
        st, keep = scenegraph_desc(desc)
        check(lib.tbvh_host_scenegraph_create(C.byref(st), C.byref(self._h)), "tbvh_host_scenegraph_create")
        self._made(keep)

    def SetTRS(self, trs10):
        """every node's translation, rotation (w x y z), scale at once; the nodes' "written" marks stay as the channels left them"""
        a = np.ascontiguousarray(trs10, np.float32)
        assert a.size == self.n_nodes * 10
        check(lib.tbvh_debug_host_scenegraph_set_trs(self._h, _ptr(a), self.n_nodes), "tbvh_debug_host_scenegraph_set_trs")
        return self

    def free(self):
        if self._h:
            lib.tbvh_host_scenegraph_free(self._h)
        self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# ---- hits resolved to shading data (capi_shade.hip) --------------------------------------------------------------------------------------
# tinyscene::FatTri, 192 bytes, taken verbatim
FATTRI_DTYPE = np.dtype([
    ("u0", "<f4"), ("u1", "<f4"), ("u2", "<f4"), ("ltriIdx", "<i4"),
    ("v0", "<f4"), ("v1", "<f4"), ("v2", "<f4"), ("material", "<u4"),
    ("vN0", "<f4", 3), ("Nx", "<f4"), ("vN1", "<f4", 3), ("Ny", "<f4"), ("vN2", "<f4", 3), ("Nz", "<f4"),
    ("vertex0", "<f4", 3), ("u0_2", "<f4"), ("vertex1", "<f4", 3), ("u1_2", "<f4"), ("vertex2", "<f4", 3), ("u2_2", "<f4"),
    ("T", "<f4", 3), ("area", "<f4"), ("B", "<f4", 3), ("invArea", "<f4"),
    ("alpha", "<f4", 3), ("LOD", "<f4"), ("v0_2", "<f4"), ("v1_2", "<f4"), ("v2_2", "<f4"), ("dummy4", "<f4"),
])
assert FATTRI_DTYPE.itemsize == 192
# tbvh_material: Material::color (value, textureID) and Material::normals.textureID; NO_TEXTURE stands for textureID == -1
MATERIAL_DTYPE = np.dtype([("color", "<f4", 3), ("color_texture", "<u4"), ("normal_texture", "<u4")])
assert MATERIAL_DTYPE.itemsize == 20
NO_TEXTURE = 0xFFFFFFFF
# what tbvh_shade_hits writes per ray, 48 bytes; "no surface" (a miss): all zero except alpha = -1
SHADED_DTYPE = np.dtype([("albedo", "<f4", 3), ("alpha", "<f4"), ("N", "<f4", 3), ("material", "<u4"), ("iN", "<f4", 3), ("texel", "<u4")])
assert SHADED_DTYPE.itemsize == 48


class ShadedHits(np.ndarray):
    """The (n, 12) float32 records of ShadeHits, with the fields by name: .albedo (n, 3), .alpha (n,), .N (n, 3), .material (n,) uint32, .iN (n, 3),
    .texel (n,) uint32, .surface (n,) bool."""

    @property
    def records(self):
        return np.asarray(self).view(SHADED_DTYPE).reshape(-1)

    albedo = property(lambda self: self.records["albedo"])
    alpha = property(lambda self: self.records["alpha"])
    N = property(lambda self: self.records["N"])
    material = property(lambda self: self.records["material"])
    iN = property(lambda self: self.records["iN"])
    texel = property(lambda self: self.records["texel"])
    surface = property(lambda self: self.records["alpha"] >= 0)


def _shade_tables(materials, textures):
    mats = np.ascontiguousarray(materials, MATERIAL_DTYPE).reshape(-1)
    tex = [_alpha_texels(t) for t in (textures or [])]
    arr = (AlphaTexture * max(len(tex), 1))(*[AlphaTexture(C.c_void_p(t.ctypes.data), t.shape[1], t.shape[0]) for t in tex])
    return mats, tex, arr


def _aligned(a: np.ndarray, dtype=None) -> np.ndarray:
    """`a`, C-contiguous, at a 16-byte aligned address (copied when it is not)"""
    a = np.ascontiguousarray(a, dtype)
    if a.ctypes.data & 15:
        raw = np.empty(a.nbytes + 16, np.uint8)
        off = -raw.ctypes.data & 15
        b = raw[off:off + a.nbytes].view(a.dtype).reshape(a.shape)
        b[...] = a
        return b
    return a


def host_shade_hits(materials, textures, fat_tris, rays, instances=None) -> ShadedHits:
    """GetShadingData on the CPU (tbvh_host_shade_hits).  fat_tris: one FATTRI_DTYPE array per BLAS slot (None: a slot without records); instances:
    the TLAS's (n, 48) float32 / 192-byte BLASInstance records, or None for a single BLAS (slot 0, identity); rays: RAY_DTYPE records (or 128-byte
    ones: any array whose rows are the records)."""
    mats, tex, arr = _shade_tables(materials, textures)
    slots = [None if f is None else _aligned(f, FATTRI_DTYPE).reshape(-1) for f in fat_tris]
    ptrs = (C.c_void_p * len(slots))(*[None if f is None else f.ctypes.data for f in slots])
    counts = np.array([0 if f is None else f.size for f in slots], np.uint64)
    rays = _aligned(rays)
    n, stride = rays.shape[0], rays.strides[0]
    inst = None if instances is None else _aligned(instances)
    n_inst = 0 if inst is None else inst.nbytes // 192
    out = _aligned(np.zeros((n, 12), np.float32))
    check(lib.tbvh_host_shade_hits(_ptr(mats), mats.size, arr, len(tex), ptrs, _ptr(counts), len(slots), None if inst is None else _ptr(inst), n_inst,
                                   _ptr(rays) if n else None, n, stride, _ptr(out) if n else None), "tbvh_host_shade_hits")
    return out.view(ShadedHits)


class Shading:
    """A shading table (tbvh_shading_*; GetShadingData of the reference's renderers): materials (MATERIAL_DTYPE) and textures ((h, w) uint32 arrays as
    Texture::idata) once, SetFatTris( slot, FATTRI_DTYPE array ) per BLAS, then ShadeHits( scene, rays ) after every Intersect."""

    def __init__(self, ctx: Context, materials, textures=None):
        self.ctx = ctx
        self._h = C.c_void_p()
        mats, tex, arr = _shade_tables(materials, textures)
        check(lib.tbvh_shading_create(ctx._h, _ptr(mats), mats.size, arr, len(tex), 0, C.byref(self._h)), "tbvh_shading_create")
        self.n_tris = {}

    def SetFatTris(self, slot: int, fat_tris=None, d_fat_tris: int = 0, n_tris: int = 0) -> "Shading":
        """The slot's FatTri records (slot = the blasIdx the instances carry), copied; a second call replaces them.  d_fat_tris / n_tris: from device memory."""
        if d_fat_tris:
            check(lib.tbvh_shading_set_fat_tris(self._h, int(slot), C.c_void_p(int(d_fat_tris)), int(n_tris), 1), "tbvh_shading_set_fat_tris")
        else:
            f = np.ascontiguousarray(fat_tris, FATTRI_DTYPE).reshape(-1)
            n_tris = f.size
            check(lib.tbvh_shading_set_fat_tris(self._h, int(slot), _ptr(f) if n_tris else None, n_tris, 0), "tbvh_shading_set_fat_tris")
        self.n_tris[int(slot)] = int(n_tris)
        return self

    def FatTris(self, slot: int):
        """(device pointer of the slot's records, n_tris)"""
        p = C.c_void_p(); n = C.c_uint64(0)
        check(lib.tbvh_shading_fat_tris(self._h, int(slot), C.byref(p), C.byref(n)), "tbvh_shading_fat_tris")
        return p.value, int(n.value)

    def Download(self, slot: int) -> np.ndarray:
        out = np.zeros(self.FatTris(slot)[1], FATTRI_DTYPE)
        check(lib.tbvh_shading_download_fat_tris(self._h, int(slot), _ptr(out), out.size), "tbvh_shading_download_fat_tris")
        return out

    def ShadeHits(self, scene: "_Scene", rays: np.ndarray) -> ShadedHits:
        """tbvh_shade_hits: the (n, 12) float32 records for host ray records as Intersect left them (rows 64 or 128 bytes apart)."""
        rays = np.ascontiguousarray(rays)
        n = rays.shape[0]
        out = np.zeros((n, 12), np.float32)
        check(lib.tbvh_shade_hits(self._h, scene._h, _ptr(rays) if n else None, n, rays.strides[0] if n else 64, _ptr(out) if n else None), "tbvh_shade_hits")
        return out.view(ShadedHits)

    def ShadeHitsDevice(self, scene: "_Scene", d_rays: int, n: int, d_out48: int, stride: int = 64) -> "Shading":
        """tbvh_shade_hits_device: asynchronous on the context's stream, 48 bytes per ray into d_out48."""
        check(lib.tbvh_shade_hits_device(self._h, scene._h, C.c_void_p(int(d_rays)), int(n), int(stride), C.c_void_p(int(d_out48))), "tbvh_shade_hits_device")
        return self

    def free(self):
        if self._h and self.ctx._h:   # (a closed context has freed its tables itself: tbvh_shutdown)
            lib.tbvh_shading_free(self._h)
        self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# ---- a viewer frame lit and finished on the device (capi_viewer.hip) ------------------------------------------------------------------------
VIEWER_GLTF, VIEWER_FOLIAGE = 0, 1


def viewer_camera(eye, p1, p2, p3, width: int, height: int) -> Camera:
    """The view pyramid of the reference's viewers (eye and the corners p1, p2, p3 as UpdateCamera leaves them) for a width x height frame."""
    cam = Camera()
    for name, v in (("eye", eye), ("p1", p1), ("p2", p2), ("p3", p3)):
        getattr(cam, name)[:] = [float(np.float32(x)) for x in v]
    cam.width, cam.height, cam.spp_x, cam.spp_y = int(width), int(height), 1, 1
    return cam


def _light_dir(light_dir):
    if light_dir is None:
        return None, None
    l = np.ascontiguousarray(light_dir, np.float32).reshape(3)
    return l, _ptr(l)


def _sky_pixels(pixels):
    """(h, w, 3) float32, C-contiguous: SkyDome::pixels"""
    p = np.ascontiguousarray(pixels, np.float32)
    if p.ndim != 3 or p.shape[2] != 3:
        raise ValueError("sky pixels: an (h, w, 3) float32 array")
    return p


def load_sky_bin(path: str) -> np.ndarray:
    """The reference's `.hdr.bin` sky cache (SkyDome::Load: two ints, then width * height texels of 3 floats) as an (h, w, 3) array — the cached texels, which
    SkyDome::Load then squares and scales: host_sky_prepare."""
    with open(path, "rb") as f:
        w, h = (int(x) for x in np.frombuffer(f.read(8), "<i4"))
        if w <= 0 or h <= 0:
            raise ValueError(f"{path}: a {w} x {h} sky")
        data = np.frombuffer(f.read(12 * w * h), "<f4")
    if data.size != 3 * w * h:
        raise ValueError(f"{path}: {data.size} floats for a {w} x {h} sky")
    return data.reshape(h, w, 3).copy()


def host_sky_prepare(pixels, scale=(1.0, 1.0, 1.0), from_hdr: bool = False) -> np.ndarray:
    """The two arithmetic passes of SkyDome::Load (tbvh_host_sky_prepare) on a copy: sqrtf when the texels come straight from the HDR file, then p * p * scale."""
    p = _sky_pixels(pixels).copy()
    s = np.ascontiguousarray(scale, np.float32).reshape(3)
    check(lib.tbvh_host_sky_prepare(_ptr(p), p.shape[0] * p.shape[1], _ptr(s), int(bool(from_hdr))), "tbvh_host_sky_prepare")
    return p


def host_sky_sample(pixels, dirs) -> np.ndarray:
    """SampleSky on the CPU (tbvh_host_sky_sample): (n, 4) float32 = the texel as ( z, y, x ) and the bits of its index.  pixels None: no sky, all zero."""
    d = np.zeros((np.asarray(dirs).shape[0], 4), np.float32)
    d[:, :3] = np.asarray(dirs, np.float32)[:, :3]
    out = np.zeros_like(d)
    if pixels is None:
        check(lib.tbvh_host_sky_sample(None, 0, 0, _ptr(d), d.shape[0], _ptr(out)), "tbvh_host_sky_sample")
    else:
        p = _sky_pixels(pixels)
        check(lib.tbvh_host_sky_sample(_ptr(p), p.shape[1], p.shape[0], _ptr(d), d.shape[0], _ptr(out)), "tbvh_host_sky_sample")
    return out


def host_viewer_generate(cam: Camera, first: int = 0, n=None) -> np.ndarray:
    """WorkerThread's rays on the CPU (tbvh_host_viewer_generate): ray i is pixel ( i % width, i / width )."""
    n = cam.width * cam.height - first if n is None else int(n)
    rays = _aligned(np.zeros(max(n, 0), RAY_DTYPE))
    check(lib.tbvh_host_viewer_generate(C.byref(cam), _ptr(rays) if n else None, int(first), n), "tbvh_host_viewer_generate")
    return rays


def host_viewer_continue(materials, n_textures: int, rays: np.ndarray, out48: np.ndarray):
    """The gltf alpha rule and continue step on host records, in place (tbvh_host_viewer_continue): the (n,) bool array of the records that stepped on."""
    mats = np.ascontiguousarray(materials, MATERIAL_DTYPE).reshape(-1)
    n = rays.shape[0]
    if rays.ctypes.data & 15 or not rays.flags.c_contiguous or not rays.flags.writeable:
        raise ValueError("host_viewer_continue: rays must be a writeable, C-contiguous, 16-byte aligned array")
    o = _aligned(out48, np.float32)
    went = np.zeros(n, np.uint8)
    check(lib.tbvh_host_viewer_continue(_ptr(mats), mats.size, int(n_textures), _ptr(rays) if n else None, rays.strides[0] if n else 64, _ptr(o) if n else None, n, _ptr(went), None),
          "tbvh_host_viewer_continue")
    return went.astype(bool)


def host_viewer_shadow_rays(rays: np.ndarray, light_dir=None) -> np.ndarray:
    r = _aligned(rays)
    n = r.shape[0]
    out = _aligned(np.zeros(n, RAY_DTYPE))
    l, lp = _light_dir(light_dir)
    check(lib.tbvh_host_viewer_shadow_rays(_ptr(r) if n else None, r.strides[0] if n else 64, n, lp, _ptr(out) if n else None), "tbvh_host_viewer_shadow_rays")
    return out


def host_viewer_light(mode: int, sky_pixels, rays: np.ndarray, out48: np.ndarray, occ=None, light_dir=None) -> np.ndarray:
    """One colour per record on the CPU (tbvh_host_viewer_light): (n, 4) float32 ( r, g, b, 0 )."""
    r = _aligned(rays)
    n = r.shape[0]
    o = _aligned(out48, np.float32)
    rgb = _aligned(np.zeros((n, 4), np.float32))
    p = None if sky_pixels is None else _sky_pixels(sky_pixels)
    oc = None if occ is None else np.ascontiguousarray(occ, np.uint8)
    l, lp = _light_dir(light_dir)
    check(lib.tbvh_host_viewer_light(int(mode), None if p is None else _ptr(p), 0 if p is None else p.shape[1], 0 if p is None else p.shape[0], _ptr(r) if n else None,
                                     r.strides[0] if n else 64, _ptr(o) if n else None, None if oc is None else _ptr(oc), n, lp, _ptr(rgb) if n else None), "tbvh_host_viewer_light")
    return rgb


def host_viewer_pack(rgb: np.ndarray) -> np.ndarray:
    c = _aligned(rgb, np.float32).reshape(-1, 4)
    out = np.zeros(c.shape[0], np.uint32)
    check(lib.tbvh_host_viewer_pack(_ptr(c) if c.shape[0] else None, c.shape[0], _ptr(out) if c.shape[0] else None), "tbvh_host_viewer_pack")
    return out


def viewer_generate(ctx: Context, cam: Camera, d_rays: int, first: int = 0, n=None):
    """tbvh_viewer_generate_device: asynchronous, 64 bytes per ray into d_rays."""
    n = cam.width * cam.height - first if n is None else int(n)
    check(lib.tbvh_viewer_generate_device(ctx._h, C.byref(cam), C.c_void_p(int(d_rays)), int(first), n), "tbvh_viewer_generate_device")


def viewer_shadow_rays(ctx: Context, d_rays: int, n: int, d_shadow: int, light_dir=None, stride: int = 64):
    l, lp = _light_dir(light_dir)
    check(lib.tbvh_viewer_shadow_rays_device(ctx._h, C.c_void_p(int(d_rays)), int(stride), int(n), lp, C.c_void_p(int(d_shadow))), "tbvh_viewer_shadow_rays_device")


def viewer_light(ctx: Context, mode: int, sky, d_rays: int, d_out48: int, n: int, d_rgb: int, d_occ: int = 0, light_dir=None, stride: int = 64, shading=None):
    """tbvh_viewer_light_device: asynchronous; sky: a SkyDome or None."""
    l, lp = _light_dir(light_dir)
    check(lib.tbvh_viewer_light_device(ctx._h, int(mode), None if shading is None else shading._h, None if sky is None else sky._h, C.c_void_p(int(d_rays)), int(stride),
                                       C.c_void_p(int(d_out48)), C.c_void_p(int(d_occ)) if d_occ else None, int(n), lp, C.c_void_p(int(d_rgb))), "tbvh_viewer_light_device")


def viewer_pack(ctx: Context, d_rgb: int, n: int, d_pixels: int):
    check(lib.tbvh_viewer_pack_device(ctx._h, C.c_void_p(int(d_rgb)), int(n), C.c_void_p(int(d_pixels))), "tbvh_viewer_pack_device")


class SkyDome:
    """A sky dome on the device (tbvh_sky_*): pixels as SkyDome::pixels, an (h, w, 3) float32 array, copied."""

    def __init__(self, ctx: Context, pixels):
        self.ctx = ctx
        self._h = C.c_void_p()
        p = _sky_pixels(pixels)
        self.height, self.width = p.shape[:2]
        check(lib.tbvh_sky_create(ctx._h, _ptr(p), self.width, self.height, 0, C.byref(self._h)), "tbvh_sky_create")

    def SampleDevice(self, d_dirs: int, n: int, d_out: int) -> "SkyDome":
        check(lib.tbvh_sky_sample_device(self._h, C.c_void_p(int(d_dirs)), int(n), C.c_void_p(int(d_out))), "tbvh_sky_sample_device")
        return self

    def free(self):
        if self._h and self.ctx._h:   # (a closed context has freed its skies itself: tbvh_shutdown)
            lib.tbvh_sky_free(self._h)
        self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Viewer:
    """A frame of the reference's CPU viewers rendered on the device (tbvh_viewer_*): Render( scene, shading, sky, cam ) goes from the camera to pixels
    without leaving it; Pixels() are the 0x00BBGGRR words, RGB() the colours before the clamp, Rays() the final ray records."""

    def __init__(self, ctx: Context, width: int, height: int):
        self.ctx = ctx
        self.width, self.height = int(width), int(height)
        self._h = C.c_void_p()
        check(lib.tbvh_viewer_create(ctx._h, self.width, self.height, C.byref(self._h)), "tbvh_viewer_create")

    def Render(self, scene: "_Scene", shading: Shading, sky, cam: Camera, mode: int = VIEWER_GLTF, light_dir=None, max_rounds: int = 0, stats: bool = True):
        """tbvh_viewer_render.  stats: wait for the frame and return {"rays": per round, "shadow_rays", "frame_ms"}; False: asynchronous, returns None."""
        p = _capi.ViewerParams()
        p.mode, p.max_rounds, p.flags = int(mode), int(max_rounds), 0
        if light_dir is not None:
            p.light_dir[:] = [float(np.float32(x)) for x in light_dir]
        st = _capi.ViewerStats()
        check(lib.tbvh_viewer_render(self._h, scene._h, shading._h, None if sky is None else sky._h, C.byref(cam), C.byref(p), C.byref(st) if stats else None), "tbvh_viewer_render")
        if not stats:
            return None
        return {"rays": [int(x) for x in st.rays], "shadow_rays": int(st.shadow_rays), "frame_ms": float(st.frame_ms)}

    def Pixels(self) -> np.ndarray:
        out = np.zeros((self.height, self.width), np.uint32)
        check(lib.tbvh_viewer_read_pixels(self._h, _ptr(out)), "tbvh_viewer_read_pixels")
        return out

    def RGB(self) -> np.ndarray:
        out = np.zeros((self.height, self.width, 4), np.float32)
        check(lib.tbvh_viewer_read_rgb(self._h, _ptr(out)), "tbvh_viewer_read_rgb")
        return out

    def RaysDevice(self) -> int:
        p = C.c_void_p()
        check(lib.tbvh_viewer_rays(self._h, C.byref(p)), "tbvh_viewer_rays")
        return p.value

    def Rays(self) -> np.ndarray:
        """the final ray records (a continued pixel's record is the one of its last round), copied back"""
        out = np.zeros(self.width * self.height, RAY_DTYPE)
        self.ctx.from_device(out, self.RaysDevice())
        return out

    def free(self):
        if self._h and self.ctx._h:   # (a closed context has freed its viewers itself: tbvh_shutdown)
            lib.tbvh_viewer_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
