"""Shared pieces of the custom-geometry (sphere BLAS) tests: the restatement (tests/oracle_custom.c) and the real reference behind
tests/custom_ref_shim.cpp, both compiled per session into a pytest temp dir, sphere sets, rays and TLAS scenes (DESIGN.md par. 12)."""
import ctypes as C
import os

import numpy as np

import native_build as nb
import tinybvh_amd as tb
from native_build import _i, _p, _u32, _u64, _vp
from tinybvh_amd import scenes

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "custom")


class _BlasDesc(C.Structure):
    _fields_ = [("kind", _u32), ("pad", _u32), ("nodes", _vp), ("primIdx", _vp), ("prims", _vp)]


class CustomOracle:
    """oracle_custom.c.  rule 0 = the reference's, 1 = the library's."""

    def __init__(self, so):
        self.lib = C.CDLL(so)
        L = self.lib
        L.cu_blas.argtypes = [_vp, _vp, _vp, _vp, _u64, _i, _vp]
        L.cu_blas.restype = _u64
        L.cu_brute.argtypes = [_vp, _u64, _vp, _u64, _i]
        L.cu_brute_unit.argtypes = [_vp, _u64, _vp, _u64]
        L.cu_tlas.argtypes = [_vp, _vp, _vp, _vp, _vp, _u64, _i, _vp]

    def intersect(self, nodes32, prim_idx, spheres, rays, rule=1):
        """a copy of rays, traced; also returns the deepest stack the walk needed"""
        r = np.ascontiguousarray(rays).copy()
        n, pi, sp = np.ascontiguousarray(nodes32).view(np.uint32), np.ascontiguousarray(prim_idx, np.uint32), np.ascontiguousarray(spheres, np.float32)
        depth = self.lib.cu_blas(_p(n), _p(pi), _p(sp), _p(r), r.shape[0], rule, None)
        return r, int(depth)

    def occluded(self, nodes32, prim_idx, spheres, rays, rule=1):
        r = np.ascontiguousarray(rays)
        out = np.zeros(r.shape[0], np.uint8)
        n, pi, sp = np.ascontiguousarray(nodes32).view(np.uint32), np.ascontiguousarray(prim_idx, np.uint32), np.ascontiguousarray(spheres, np.float32)
        self.lib.cu_blas(_p(n), _p(pi), _p(sp), _p(r), r.shape[0], rule, _p(out))
        return out

    def brute(self, spheres, rays, rule=1):
        r = np.ascontiguousarray(rays).copy()
        sp = np.ascontiguousarray(spheres, np.float32)
        self.lib.cu_brute(_p(sp), sp.shape[0], _p(r), r.shape[0], rule)
        return r

    def brute_unit(self, spheres, rays):
        r = np.ascontiguousarray(rays).copy()
        sp = np.ascontiguousarray(spheres, np.float32)
        self.lib.cu_brute_unit(_p(sp), sp.shape[0], _p(r), r.shape[0])
        return r

    def _tlas(self, tlas_nodes32, tlas_idx, instances, blas, rays, rule, occ):
        """blas: list of ("sph", nodes32, prim_idx, spheres) / ("tri", nodes32, prim_idx, verts)"""
        keep = []
        descs = (_BlasDesc * len(blas))()
        for i, (kind, nodes, pi, prims) in enumerate(blas):
            nodes = np.ascontiguousarray(nodes).view(np.uint32); pi = np.ascontiguousarray(pi, np.uint32); prims = np.ascontiguousarray(prims, np.float32)
            keep += [nodes, pi, prims]
            descs[i] = _BlasDesc(0 if kind == "sph" else 1, 0, nodes.ctypes.data, pi.ctypes.data, prims.ctypes.data)
        tn = np.ascontiguousarray(tlas_nodes32).view(np.uint32); ti = np.ascontiguousarray(tlas_idx, np.uint32); inst = np.ascontiguousarray(instances)
        self.lib.cu_tlas(_p(tn), _p(ti), _p(inst), C.cast(descs, _vp), _p(rays), rays.shape[0], rule, _p(occ) if occ is not None else None)

    def tlas_intersect(self, tlas_nodes32, tlas_idx, instances, blas, rays, rule=1):
        r = np.ascontiguousarray(rays).copy()
        self._tlas(tlas_nodes32, tlas_idx, instances, blas, r, rule, None)
        return r

    def tlas_occluded(self, tlas_nodes32, tlas_idx, instances, blas, rays, rule=1):
        r = np.ascontiguousarray(rays)
        out = np.zeros(r.shape[0], np.uint8)
        self._tlas(tlas_nodes32, tlas_idx, instances, blas, r, rule, out)
        return out


class RefCustom:
    """The real reference (custom_ref_shim.cpp)."""

    def __init__(self, so):
        self.lib = C.CDLL(so)
        L = self.lib
        L.cref_build_spheres.argtypes = [_vp, _u32]
        L.cref_build_spheres.restype = _vp
        L.cref_build_tris.argtypes = [_vp, _u32]
        L.cref_build_tris.restype = _vp
        L.cref_free.argtypes = [_vp]
        L.cref_blob.argtypes = [_vp, _i, C.POINTER(_vp)]
        L.cref_blob.restype = _u64
        L.cref_intersect.argtypes = [_vp, _vp, _u64]
        L.cref_occluded.argtypes = [_vp, _vp, _u64, _vp]
        L.cref_tlas_build.argtypes = [_vp, _u32, _vp, _u32]
        L.cref_tlas_build.restype = _vp
        L.cref_tlas_free.argtypes = [_vp]
        L.cref_tlas_blob.argtypes = [_vp, _i, C.POINTER(_vp)]
        L.cref_tlas_blob.restype = _u64
        L.cref_tlas_intersect.argtypes = [_vp, _vp, _u64]
        L.cref_tlas_occluded.argtypes = [_vp, _vp, _u64, _vp]

    def build_spheres(self, spheres):
        s = np.ascontiguousarray(spheres, np.float32)
        h = self.lib.cref_build_spheres(_p(s), s.shape[0])
        assert h, "every sphere slot of the shim is taken"
        return h

    def build_tris(self, verts):
        v = np.ascontiguousarray(verts, np.float32)
        return self.lib.cref_build_tris(_p(v), v.shape[0] // 3)

    def free(self, h):
        self.lib.cref_free(h)

    @staticmethod
    def _view(p, n, width):
        a = np.ctypeslib.as_array((C.c_uint32 * (n * width)).from_address(p.value)).copy()
        return a.reshape(n, width) if width > 1 else a

    def blob(self, h, which):
        """0 Wald nodes (n, 8) u32, 1 primIdx, 2 BVH_GPU::ConvertFrom nodes (n, 16) u32"""
        p = _vp()
        n = self.lib.cref_blob(h, which, C.byref(p))
        return self._view(p, n, {0: 8, 1: 1, 2: 16}[which])

    def intersect(self, h, rays):
        r = np.ascontiguousarray(rays).copy()
        self.lib.cref_intersect(h, _p(r), r.shape[0])
        return r

    def occluded(self, h, rays):
        r = np.ascontiguousarray(rays)
        out = np.zeros(r.shape[0], np.uint8)
        self.lib.cref_occluded(h, _p(r), r.shape[0], _p(out))
        return out

    def tlas_build(self, instances, blas_handles):
        inst = np.ascontiguousarray(instances)
        arr = (_vp * len(blas_handles))(*blas_handles)
        return self.lib.cref_tlas_build(_p(inst), inst.shape[0], arr, len(blas_handles))

    def tlas_free(self, h):
        self.lib.cref_tlas_free(h)

    def tlas_blob(self, h, which):
        """0 BVH_GPU::ConvertFrom nodes (n, 16) u32, 1 primIdx, 2 Wald nodes (n, 8) u32"""
        p = _vp()
        n = self.lib.cref_tlas_blob(h, which, C.byref(p))
        return self._view(p, n, {0: 16, 1: 1, 2: 8}[which])

    def tlas_intersect(self, h, rays):
        r = np.ascontiguousarray(rays).copy()
        self.lib.cref_tlas_intersect(h, _p(r), r.shape[0])
        return r

    def tlas_occluded(self, h, rays):
        r = np.ascontiguousarray(rays)
        out = np.zeros(r.shape[0], np.uint8)
        self.lib.cref_tlas_occluded(h, _p(r), r.shape[0], _p(out))
        return out


def compile_oracle(d):
    return CustomOracle(nb.compile_c_oracle(d, "oracle_custom"))


def compile_ref_shim(d):
    """the reference with oracle/Makefile's flags; None when the reference is absent"""
    so = nb.compile_ref_shim(d, "custom_ref_shim.cpp")
    return so and RefCustom(so)


cu_oracle = nb.oracle_fixture("oracle_custom", compile_oracle)
cu_ref = nb.ref_fixture("custom_ref", compile_ref_shim)


# ---- sphere sets ------------------------------------------------------------------------------------------------------------------------
def bunny_verts():
    """the reference's testdata/bunny.bin, bit for bit (tests/golden/meshes/bunny.npz)"""
    g = np.load(os.path.join(HERE, "golden", "meshes", "bunny.npz"))
    verts = np.empty((g["indices"].size, 4), np.float32)
    verts[:, :3] = g["positions"][g["indices"].ravel()]
    verts[:, 3] = g["w_bits"].view(np.float32)[0]
    return verts


def spheres_from_tris(verts, rmax, k):
    """one sphere per triangle as the demos make them: r = min(rmax, k * min(|v1 - v0|, |v2 - v0|)), pos = (v0 + v1 + v2) * 0.33333"""
    t = np.ascontiguousarray(verts, np.float32).reshape(-1, 3, 4)[:, :, :3]
    e1 = np.sqrt(((t[:, 1] - t[:, 0]) ** 2).sum(1, dtype=np.float32)).astype(np.float32)
    e2 = np.sqrt(((t[:, 2] - t[:, 0]) ** 2).sum(1, dtype=np.float32)).astype(np.float32)
    s = np.empty((t.shape[0], 4), np.float32)
    s[:, :3] = ((t[:, 0] + t[:, 1] + t[:, 2]) * np.float32(0.33333)).astype(np.float32)
    s[:, 3] = np.minimum(np.float32(rmax), np.float32(k) * np.minimum(e1, e2))
    return s


def sphere_set(name):
    if name == "bunny":        # tiny_bvh_anim.cpp's bunny spheres
        return spheres_from_tris(bunny_verts(), 1.2, 0.55)
    if name == "bunny16":      # every 16th of them (the committed goldens stay small)
        return np.ascontiguousarray(sphere_set("bunny")[::16])
    if name == "soup":         # a random cloud, overlapping spheres included
        rng = np.random.default_rng(7)
        s = np.empty((3000, 4), np.float32)
        s[:, :3] = rng.uniform(-10, 10, (3000, 3))
        s[:, 3] = rng.uniform(0.05, 0.8, 3000)
        return s
    if name == "atrium":       # tiny_bvh_custom.cpp's one sphere per triangle, on the Sponza stand-in
        return spheres_from_tris(scenes.atrium(20_000, seed=1), 0.35, 0.25)
    if name == "one":
        return np.array([[0.5, 0.25, -0.5, 0.75]], np.float32)
    if name == "dups":         # exact duplicates: ties at equal distance, the smaller prim wins
        s = sphere_set("soup")[:400]
        return np.concatenate([s, s, s[::-1]]).astype(np.float32)
    raise KeyError(name)


def rays_for(spheres, n, seed, kind="incoherent"):
    """camera-like (from outside towards the set), incoherent (origins in the box, random directions) or inside (origins at sphere centres)"""
    rng = np.random.default_rng(seed)
    lo, hi = spheres[:, :3].min(0) - spheres[:, 3].max(), spheres[:, :3].max(0) + spheres[:, 3].max()
    c, ext = (lo + hi) * 0.5, float((hi - lo).max())
    if kind == "camera":
        eye = c + np.array([0.2, 0.35, 1.6], np.float32) * ext
        tgt = c + rng.uniform(-0.45, 0.45, (n, 3)).astype(np.float32) * (hi - lo)
        return tb.make_rays(np.broadcast_to(eye, (n, 3)), tgt - eye)
    if kind == "inside":
        k = rng.integers(0, spheres.shape[0], n)
        O = spheres[k, :3] + rng.normal(0, 0.1, (n, 3)).astype(np.float32) * spheres[k, 3:4]
        return tb.make_rays(O, rng.normal(size=(n, 3)))
    return tb.make_rays(rng.uniform(lo, hi, (n, 3)), rng.normal(size=(n, 3)))


def shadow_rays(hits, light, eps=1e-3):
    """from each hit point towards the light, tmax = the distance to it (misses keep their direction and t = 1e30)"""
    h = hits["t"] < np.float32(1e30)
    P = (hits["O"] + hits["D"] * np.where(h, hits["t"], np.float32(0))[:, None]).astype(np.float32)
    L = (np.asarray(light, np.float32)[None, :] - P).astype(np.float32)
    d = np.sqrt((L * L).sum(1)).astype(np.float32)
    r = tb.make_rays(np.where(h[:, None], P + L / np.maximum(d, 1e-20)[:, None] * np.float32(eps), hits["O"]),
                     np.where(h[:, None], L, hits["D"]))
    r["t"] = np.where(h, d - np.float32(2 * eps), np.float32(1e30)).astype(np.float32)
    return r


def decorate(rays, seed):
    """non-zero incoming u, v and instIdx, some finite tmax: the kernels must leave u, v alone and pass instIdx through"""
    rng = np.random.default_rng(seed)
    r = rays.copy()
    r["u"] = rng.uniform(0, 1, r.shape[0]).astype(np.float32)
    r["v"] = rng.uniform(0, 1, r.shape[0]).astype(np.float32)
    r["instIdx"] = rng.integers(0, 1 << 31, r.shape[0]).astype(np.uint32)
    r["inst"] = 0xDEADBEEF
    r["prim"] = 0xFFFFFFFF
    fin = rng.random(r.shape[0]) < 0.25
    r["t"][fin] = rng.uniform(0.5, 8, int(fin.sum())).astype(np.float32)
    return r


def caterpillar(n):
    """a hand-made tree of depth n over n + 1 spheres on the x axis whose near child is always the subtree: a ray along +x pushes n far
    leaves (deeper than any LDS stack top); node 1 unused as in the reference"""
    sph = np.zeros((n + 1, 4), np.float32)
    sph[:, 0] = np.arange(n + 1, 0, -1, dtype=np.float32) * 3.0   # sphere i at x = 3 (n + 1 - i): sphere 0 the farthest
    sph[:, 3] = 1.0
    nodes = np.zeros((2 * n + 2, 8), np.uint32)
    f = nodes.view(np.float32)

    def box(k, lo, hi):
        f[k, 0:3] = [sph[hi - 1, 0] - 1, -1, -1]
        f[k, 4:7] = [sph[lo, 0] + 1, 1, 1]

    box(0, 0, n + 1)
    nodes[0, 3] = 2
    for level in range(n):
        left, right = 2 + 2 * level, 3 + 2 * level       # left: the leaf of sphere `level`, right: the rest
        box(left, level, level + 1); nodes[left, 3] = level; nodes[left, 7] = 1
        box(right, level + 1, n + 1)
        if level == n - 1:
            nodes[right, 3] = n; nodes[right, 7] = 1
        else:
            nodes[right, 3] = 4 + 2 * level
    return nodes, np.arange(n + 1, dtype=np.uint32), sph


def same_records(a, b):
    """byte-for-byte equality of 64-byte records"""
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1, 64), np.ascontiguousarray(b).view(np.uint8).reshape(-1, 64)


def mismatches(a, b):
    x, y = same_records(a, b)
    return int((x != y).any(1).sum())
