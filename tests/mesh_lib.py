"""Shared by the indexed-mesh tests and tools/make_mesh_golden.py: the real reference behind tests/mesh_ref_shim.cpp (compiled per session into a
pytest temp dir), the golden directory, and the one mesh, ray set, sphere set and moved frame the goldens are made of (DESIGN.md par. 13)."""
import ctypes as C
import os

import numpy as np

import native_build as nb
import tinybvh_amd as tb
from native_build import _i, _p, _u32, _u64, _vp
from tinybvh_amd import rays as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "mesh")
GOLDEN_STEP = 24   # every 24th triangle of the bunny: the golden file stays under 1 MB


class RefMesh:
    """The real reference (mesh_ref_shim.cpp).  Vertices go in as a dense (n_verts, stride / 4) float32 buffer, stride a multiple of 16."""

    def __init__(self, so):
        self.lib = L = C.CDLL(so)
        L.mref_build.argtypes = [_vp, _u32, _u32, _vp, _u32]
        L.mref_build.restype = _vp
        L.mref_free.argtypes = [_vp]
        L.mref_blob.argtypes = [_vp, _i, C.POINTER(_vp)]
        L.mref_blob.restype = _u64
        L.mref_intersect.argtypes = [_vp, _vp, _u64]
        L.mref_occluded.argtypes = [_vp, _vp, _u64, _vp]
        L.mref_spheres.argtypes = [_vp, _vp, _u64, _vp]
        L.mref_refit.argtypes = [_vp, _vp]

    def build(self, buf, indices=None):
        buf = np.ascontiguousarray(buf, np.float32)
        assert buf.ndim == 2 and buf.shape[1] % 4 == 0
        if indices is None:
            return self.lib.mref_build(_p(buf), buf.shape[0], buf.shape[1] * 4, None, buf.shape[0] // 3)
        idx = np.ascontiguousarray(indices, np.uint32).reshape(-1)
        return self.lib.mref_build(_p(buf), buf.shape[0], buf.shape[1] * 4, _p(idx), idx.size // 3)

    def free(self, h):
        self.lib.mref_free(h)

    def blob(self, h, which):
        """0 BVH_GPU nodes (n, 16) u32, 1 primIdx (n,), 2 Wald nodes (n, 8)"""
        p = _vp()
        n = self.lib.mref_blob(h, which, C.byref(p))
        width = {0: 16, 1: 1, 2: 8}[which]
        a = np.ctypeslib.as_array((C.c_uint32 * (n * width)).from_address(p.value)).reshape(n, width).copy()
        return a.reshape(-1) if which == 1 else a

    def intersect(self, h, rays):
        r = np.ascontiguousarray(rays).copy()
        self.lib.mref_intersect(h, _p(r), r.shape[0])
        return r

    def occluded(self, h, rays):
        r = np.ascontiguousarray(rays)
        out = np.zeros(r.shape[0], np.uint8)
        self.lib.mref_occluded(h, _p(r), r.shape[0], _p(out))
        return out

    def spheres(self, h, sp):
        sp = np.ascontiguousarray(sp, np.float32)
        out = np.zeros(sp.shape[0], np.uint8)
        self.lib.mref_spheres(h, _p(sp), sp.shape[0], _p(out))
        return out

    def refit(self, h, buf):
        buf = np.ascontiguousarray(buf, np.float32)
        self.lib.mref_refit(h, _p(buf))


def compile_ref_shim(d):
    """the reference with oracle/Makefile's flags; None when the reference is absent"""
    so = nb.compile_ref_shim(d, "mesh_ref_shim.cpp")
    return so and RefMesh(so)


mesh_ref = nb.ref_fixture("mesh_ref", compile_ref_shim)


# ---- the golden case ------------------------------------------------------------------------------------------------------------------
def bunny(step=8):
    """every step-th triangle of the committed bunny, vertices compacted: (positions (n, 4) with w = 0, indices (m, 3))"""
    d = np.load(os.path.join(HERE, "golden", "meshes", "bunny.npz"))
    idx = d["indices"][::step]
    used, inv = np.unique(idx.reshape(-1), return_inverse=True)
    pos = np.zeros((used.size, 4), np.float32)
    pos[:, :3] = d["positions"][used]
    return pos, np.ascontiguousarray(inv.reshape(-1, 3).astype(np.uint32))


def flatten(pos, idx):
    return np.ascontiguousarray(pos[idx.reshape(-1)])


def stride32(pos, junk=7.5):
    """dense 32-byte rows: the position, then finite junk (the reference loads the whole bvhvec4 and more of the row is never its business)"""
    buf = np.full((pos.shape[0], 8), junk, np.float32)
    buf[:, :3] = pos[:, :3]
    buf[:, 3] = 0
    return buf


def moved(pos, amount=0.02, seed=4):
    """the shared vertices displaced smoothly: every triangle around a vertex moves with it"""
    v = pos.copy()
    p = v[:, :3]
    rng = np.random.default_rng(seed)
    ext = float(np.linalg.norm(p.max(0) - p.min(0)))
    k = (rng.uniform(5.0, 20.0, (3, 3)) / ext).astype(np.float32); ph = rng.uniform(0, 6.28, 3).astype(np.float32)
    d = np.stack([np.sin(p @ k[0] + ph[0]), np.sin(p @ k[1] + ph[1]), np.sin(p @ k[2] + ph[2])], 1).astype(np.float32)
    v[:, :3] = p + np.float32(amount * ext) * d
    return v


def golden_rays(flat, n=3000, seed=17):
    """random rays through the box, camera rays from outside it, a quarter of those with a finite tmax"""
    lo, hi = flat[:, :3].min(0), flat[:, :3].max(0)
    ext = hi - lo
    a = R.random_rays(n // 2, lo - 0.2 * ext, hi + 0.2 * ext, seed=seed)
    rng = np.random.default_rng(seed + 1)
    m = n - n // 2
    eye = ((lo + hi) * 0.5 + np.array([0.3, 0.2, 2.5], np.float32) * ext).astype(np.float32)
    tgt = lo + rng.random((m, 3), dtype=np.float32) * ext
    b = tb.make_rays(np.broadcast_to(eye, (m, 3)).copy(), (tgt - eye).astype(np.float32))
    b["t"][::4] = np.float32(np.linalg.norm(ext) * 2.6)
    return np.concatenate([a, b])


def golden_spheres(flat, n=3000, seed=23):
    lo, hi = flat[:, :3].min(0), flat[:, :3].max(0)
    rng = np.random.default_rng(seed)
    sp = np.zeros((n, 4), np.float32)
    sp[:, :3] = lo + rng.random((n, 3), dtype=np.float32) * (hi - lo)
    sp[:, 3] = rng.random(n, dtype=np.float32) * np.float32(0.04 * np.linalg.norm(hi - lo))
    return sp
