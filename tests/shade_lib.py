"""Shared by the shading tests (test_shade_host.py, test_shade_gpu.py), tools/make_shade_golden.py and tools/shade_bench.py (so: NumPy and the compilers only, no
GPU library; the tests' scene is in tests/shade_fixtures.py): the plain-C restatement of GetShadingData (tests/oracle_shade.c), the real
reference behind tests/shade_ref_shim.cpp (compiled per session into a pytest temp dir when the reference checkout is present), and the goldens under
tests/golden/shade (DESIGN.md par. 16)."""
import ctypes as C
import os

import numpy as np

import native_build as nb
from native_build import _p, _u32, _u64, _vp

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "shade")
NO_TEXTURE = 0xFFFFFFFF
# oracle_shade.c's flags
WRAPPED, REF_OUT_OF_BOUNDS, NO_SURFACE, BAD_INDEX, TU_INTEGER = 1, 2, 4, 8, 16

FATTRI_DTYPE = np.dtype([
    ("u0", "<f4"), ("u1", "<f4"), ("u2", "<f4"), ("ltriIdx", "<i4"),
    ("v0", "<f4"), ("v1", "<f4"), ("v2", "<f4"), ("material", "<u4"),
    ("vN0", "<f4", 3), ("Nx", "<f4"), ("vN1", "<f4", 3), ("Ny", "<f4"), ("vN2", "<f4", 3), ("Nz", "<f4"),
    ("vertex0", "<f4", 3), ("u0_2", "<f4"), ("vertex1", "<f4", 3), ("u1_2", "<f4"), ("vertex2", "<f4", 3), ("u2_2", "<f4"),
    ("T", "<f4", 3), ("area", "<f4"), ("B", "<f4", 3), ("invArea", "<f4"),
    ("alpha", "<f4", 3), ("LOD", "<f4"), ("v0_2", "<f4"), ("v1_2", "<f4"), ("v2_2", "<f4"), ("dummy4", "<f4"),
])
MATERIAL_DTYPE = np.dtype([("color", "<f4", 3), ("color_texture", "<u4"), ("normal_texture", "<u4")])
assert FATTRI_DTYPE.itemsize == 192 and MATERIAL_DTYPE.itemsize == 20


class _Tex(C.Structure):
    _fields_ = [("texels", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32)]


def _slots(fat_tris):
    slots = [None if f is None else np.ascontiguousarray(f, FATTRI_DTYPE).reshape(-1) for f in fat_tris]
    ptrs = (C.c_void_p * len(slots))(*[None if f is None else f.ctypes.data for f in slots])
    return slots, ptrs


class Restatement:
    """shade(...): ((n, 12) float32 records, (n,) uint32 flags) — tests/oracle_shade.c"""

    def __init__(self, so):
        self.lib = C.CDLL(so)
        self.lib.osh_shade.restype = None
        self.lib.osh_shade.argtypes = [_vp, _u32, _vp, _vp, _u32, _vp, _vp, _u32, _vp, _u32, _vp, _u32, _u64, _vp, _vp]

    def shade(self, materials, textures, fat_tris, rays, instances=None, slot_no_surface=None):
        mats = np.ascontiguousarray(materials, MATERIAL_DTYPE).reshape(-1)
        tex = [np.ascontiguousarray(t, np.uint32) for t in textures]
        arr = (_Tex * max(len(tex), 1))(*[_Tex(t.ctypes.data, t.shape[1], t.shape[0]) for t in tex])
        slots, ptrs = _slots(fat_tris)
        counts = np.array([0 if f is None else f.size for f in slots], np.uint64)
        rays = np.ascontiguousarray(rays)
        n = rays.shape[0]
        inst = None if instances is None else np.ascontiguousarray(instances)
        sns = None if slot_no_surface is None else np.ascontiguousarray(slot_no_surface, np.uint8)
        out = np.full((n, 12), np.float32(7.5), np.float32)
        flags = np.zeros(n, np.uint32)
        self.lib.osh_shade(None if inst is None else _p(inst), 0 if inst is None else inst.nbytes // 192, ptrs, _p(counts), len(slots), None if sns is None else _p(sns),
                           _p(mats), mats.size, arr, len(tex), _p(rays), rays.strides[0] if n else 64, n, _p(out), _p(flags))
        return out, flags


class RealReference:
    """shade(...): (n, 12) float32 with words 0..10 from the real GetShadingData (word 11, the texel's bits, is 0).  Only for records that are in-range hits
    whose texel reads lie inside the textures: the reference has no checks."""

    def __init__(self, so):
        self.lib = C.CDLL(so)
        self.lib.sref_shade.restype = None
        self.lib.sref_shade.argtypes = [_vp, _u32, _vp, _vp, _u32, _vp, _u32, _vp, _vp, _vp, _u32, _vp, _u32, _u32, _vp]
        self.lib.sref_setpose_skin.restype = self.lib.sref_setpose_morph.restype = None
        self.lib.sref_setpose_skin.argtypes = [_vp, _u32, _vp, _vp, _vp, _vp, _u32, _vp]
        self.lib.sref_setpose_morph.argtypes = [_vp, _vp, _u32, _u32, _vp, _vp]

    def setpose_skin(self, fat, rest, joints, weights, normals, mats):
        """the real Mesh::SetPose( skin ) over a FLAT mesh: a copy of `fat` as the reference leaves its triangles"""
        f = np.array(fat, FATTRI_DTYPE).reshape(-1)
        rest = np.ascontiguousarray(rest, np.float32).reshape(-1, 4); joints = np.ascontiguousarray(joints, np.uint32); weights = np.ascontiguousarray(weights, np.float32)
        nrm = np.ascontiguousarray(normals, np.float32).reshape(-1, 3); mats = np.ascontiguousarray(mats, np.float32).reshape(-1, 16)
        assert rest.shape[0] == 3 * f.size == nrm.shape[0]
        self.lib.sref_setpose_skin(_p(rest), rest.shape[0], _p(joints), _p(weights), _p(nrm), _p(mats), mats.shape[0], _p(f))
        return f

    def setpose_morph(self, fat, positions, normals, weights):
        f = np.array(fat, FATTRI_DTYPE).reshape(-1)
        pos = np.ascontiguousarray(positions, np.float32); nrm = np.ascontiguousarray(normals, np.float32); w = np.ascontiguousarray(weights, np.float32)
        assert pos.shape == nrm.shape and pos.shape[1] == 3 * f.size and w.size == pos.shape[0] - 1
        self.lib.sref_setpose_morph(_p(pos), _p(nrm), pos.shape[1], pos.shape[0] - 1, _p(w), _p(f))
        return f

    def shade(self, materials, textures, fat_tris, rays, instances):
        mats = np.ascontiguousarray(materials, MATERIAL_DTYPE).reshape(-1)
        tex = [np.ascontiguousarray(t, np.uint32) for t in textures]
        tptr = (C.c_void_p * max(len(tex), 1))(*[t.ctypes.data for t in tex])
        widths = np.array([t.shape[1] for t in tex] or [0], np.uint32)
        heights = np.array([t.shape[0] for t in tex] or [0], np.uint32)
        slots, ptrs = _slots(fat_tris)
        counts = np.array([0 if f is None else f.size for f in slots], np.uint32)
        rays = np.ascontiguousarray(rays)
        inst = np.ascontiguousarray(instances)
        out = np.full((rays.shape[0], 12), np.float32(7.5), np.float32)
        self.lib.sref_shade(_p(inst), inst.nbytes // 192, ptrs, _p(counts), len(slots), _p(mats.view(np.uint32)), mats.size, tptr, _p(widths), _p(heights), len(tex),
                            _p(rays), rays.strides[0], rays.shape[0], _p(out))
        return out


def compile_oracle(d):
    return Restatement(nb.compile_c_oracle(d, "oracle_shade"))


def compile_ref_shim(d):
    """The real GetShadingData with oracle/Makefile's flags; None when the reference is absent"""
    so = nb.compile_ref_shim(d, "shade_ref_shim.cpp", scene_header=True, need=("tiny_bvh.h", "tiny_scene.h", "tiny_bvh_foliage.cpp"))
    return so and RealReference(so)


def golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


# ---- the FatTri half of SetPose ---------------------------------------------------------------------------------------------------------------
WRITTEN_WORDS = slice(8, 32)   # quarters 2 .. 7 of a FatTri: vN0 Nx, vN1 Ny, vN2 Nz, vertex0 ., vertex1 ., vertex2 . — every field SetPose writes
POSE_SMALL = 300               # the second frame of a pose golden is kept for this many triangles only (file size)


def words(fat):
    return np.ascontiguousarray(fat).view(np.uint32).reshape(-1, 48)


def skin_fields():
    return ["vertex0", "vertex1", "vertex2", "vN0", "vN1", "vN2", "Nx", "Ny", "Nz"]


def morph_fields():
    return ["vertex0", "vertex1", "vertex2", "vN0", "vN1", "vN2"]


def only_these_changed(before, after, fields):
    """every byte of `after` outside `fields` equals `before`"""
    a, b = np.array(before), np.array(after)
    for f in fields:
        a[f] = b[f]
    return a.tobytes() == b.tobytes()

