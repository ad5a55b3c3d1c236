"""Shared pieces of the fp64 custom-geometry (sphere BLAS) tests: the restatement (tests/oracle_custom_double.c, compiled per session without
contraction), sphere sets, rays, hand-made trees and the numpy restatement of the device builder over sphere boxes (DESIGN.md par. 9)."""
import ctypes as C
import os

import numpy as np

import native_build as nb
import tinybvh_amd as tb
from custom_lib import bunny_verts, spheres_from_tris
from double_anim_lib import karras_tlas
from native_build import _i, _p, _u64, _vp

N_SPHERES = 2048
N_RAYS = 4096
FAR = np.array([1.0e7, -1.0e7, 1.0e7])

_BOX_DTYPE = np.dtype([("aabbMin", "<f8", 3), ("aabbMax", "<f8", 3)])


class _Blas(C.Structure):
    _fields_ = [("kind", _u64), ("nodes", _vp), ("idx", _vp), ("prims", _vp)]


class OracleCustomDouble:
    """oracle_custom_double.c.  rule 0 = the reference's, 1 = the library's."""

    def __init__(self, so):
        self.lib = C.CDLL(so)
        L = self.lib
        L.ocd_blas.argtypes = [_vp, _vp, _vp, _vp, _u64, _i, _vp]
        L.ocd_blas.restype = _u64
        L.ocd_brute.argtypes = [_vp, _u64, _vp, _u64, _i]
        L.ocd_tlas.argtypes = [_vp, _vp, _vp, _vp, _vp, _u64, _i, _vp]
        L.ocd_tlas.restype = _u64

    @staticmethod
    def _blob(nodes, idx, sph):
        return np.ascontiguousarray(nodes), np.ascontiguousarray(idx, np.uint64), np.ascontiguousarray(sph, np.float64).reshape(-1, 4)

    def intersect(self, nodes, idx, sph, rays, rule=1, depth=False):
        nodes, idx, sph = self._blob(nodes, idx, sph)
        out = np.ascontiguousarray(rays).copy()
        d = self.lib.ocd_blas(_p(nodes), _p(idx), _p(sph), _p(out), out.shape[0], rule, None)
        return (out, int(d)) if depth else out

    def occluded(self, nodes, idx, sph, rays, rule=1):
        nodes, idx, sph = self._blob(nodes, idx, sph)
        rays = np.ascontiguousarray(rays)
        out = np.zeros(rays.shape[0], np.uint8)
        self.lib.ocd_blas(_p(nodes), _p(idx), _p(sph), _p(rays), rays.shape[0], rule, _p(out))
        return out

    def brute(self, sph, rays, rule=1):
        sph = np.ascontiguousarray(sph, np.float64).reshape(-1, 4)
        out = np.ascontiguousarray(rays).copy()
        self.lib.ocd_brute(_p(sph), sph.shape[0], _p(out), out.shape[0], rule)
        return out

    def _tlas(self, tnodes, tidx, inst, blas, rays, rule, occ):
        """blas: list of ("sph", nodes, prim_idx, spheres) / ("tri", nodes, prim_idx, verts)"""
        keep = []
        descs = (_Blas * len(blas))()
        for i, (kind, nodes, idx, prims) in enumerate(blas):
            nodes = np.ascontiguousarray(nodes); idx = np.ascontiguousarray(idx, np.uint64); prims = np.ascontiguousarray(prims, np.float64)
            keep += [nodes, idx, prims]
            descs[i] = _Blas(0 if kind == "sph" else 1, nodes.ctypes.data, idx.ctypes.data, prims.ctypes.data)
        tnodes = np.ascontiguousarray(tnodes); tidx = np.ascontiguousarray(tidx, np.uint64); inst = np.ascontiguousarray(inst)
        return int(self.lib.ocd_tlas(_p(tnodes), _p(tidx), _p(inst), C.cast(descs, _vp), _p(rays), rays.shape[0], rule, _p(occ) if occ is not None else None))

    def tlas_intersect(self, tnodes, tidx, inst, blas, rays, rule=1):
        out = np.ascontiguousarray(rays).copy()
        self._tlas(tnodes, tidx, inst, blas, out, rule, None)
        return out

    def tlas_occluded(self, tnodes, tidx, inst, blas, rays, rule=1):
        rays = np.ascontiguousarray(rays)
        out = np.zeros(rays.shape[0], np.uint8)
        self._tlas(tnodes, tidx, inst, blas, rays, rule, out)
        return out


def compile_oracle(d):
    return OracleCustomDouble(nb.compile_c_oracle(d, "oracle_custom_double"))


ocd = nb.oracle_fixture("oracle_custom_double", compile_oracle)


class RefCustomDouble:
    """The real reference (custom_double_ref_shim.cpp)."""

    def __init__(self, so):
        self.lib = C.CDLL(so)
        L = self.lib
        L.cdref_build_spheres.argtypes = [_vp, _u64]; L.cdref_build_spheres.restype = _vp
        L.cdref_build_tris.argtypes = [_vp, _u64]; L.cdref_build_tris.restype = _vp
        L.cdref_free.argtypes = [_vp]
        L.cdref_blob.argtypes = [_vp, _i, C.POINTER(_vp)]; L.cdref_blob.restype = _u64
        L.cdref_intersect.argtypes = [_vp, _vp, _u64]
        L.cdref_tlas_build.argtypes = [_vp, _u64, _vp, _u64]; L.cdref_tlas_build.restype = _vp
        L.cdref_tlas_free.argtypes = [_vp]
        L.cdref_tlas_blob.argtypes = [_vp, _i, C.POINTER(_vp)]; L.cdref_tlas_blob.restype = _u64
        L.cdref_tlas_intersect.argtypes = [_vp, _vp, _u64]
        L.cdref_occluded.argtypes = [_vp, _vp, _u64, _vp]
        L.cdref_tlas_occluded.argtypes = [_vp, _vp, _u64, _vp]

    def build_spheres(self, sph):
        s = np.ascontiguousarray(sph, np.float64).reshape(-1, 4)
        h = self.lib.cdref_build_spheres(_p(s), s.shape[0])
        assert h, "every sphere slot of the shim is taken"
        return h

    def build_tris(self, verts):
        v = np.ascontiguousarray(verts, np.float64)
        return self.lib.cdref_build_tris(_p(v), v.size // 9)

    def free(self, h):
        self.lib.cdref_free(h)

    @staticmethod
    def _view(p, n, dtype):
        return np.frombuffer((C.c_char * (n * dtype.itemsize)).from_address(p.value), dtype=dtype).copy()

    def blob(self, h, tlas=False):
        """(bvhNode as NODE_DBL_DTYPE, primIdx)"""
        f = self.lib.cdref_tlas_blob if tlas else self.lib.cdref_blob
        p = _vp(); n = f(h, 0, C.byref(p)); nodes = self._view(p, n, tb.NODE_DBL_DTYPE)
        p = _vp(); n = f(h, 1, C.byref(p))
        return nodes, self._view(p, n, np.dtype("<u8"))

    def intersect(self, h, rays, tlas=False):
        r = np.ascontiguousarray(rays).copy()
        (self.lib.cdref_tlas_intersect if tlas else self.lib.cdref_intersect)(h, _p(r), r.shape[0])
        return r

    def occluded(self, h, rays, tlas=False):
        """IsOccluded of a triangle BLAS or of a TLAS over triangle BLASes (the custom branch discards its callback's answer)"""
        r = np.ascontiguousarray(rays)
        out = np.zeros(r.shape[0], np.uint8)
        (self.lib.cdref_tlas_occluded if tlas else self.lib.cdref_occluded)(h, _p(r), r.shape[0], _p(out))
        return out

    def tlas_build(self, inst, blas_handles):
        """inst is updated in place, as BVH_Double::Build( BLASInstanceEx*, ... ) does"""
        arr = (_vp * len(blas_handles))(*blas_handles)
        return self.lib.cdref_tlas_build(_p(inst), inst.shape[0], arr, len(blas_handles))

    def tlas_free(self, h):
        self.lib.cdref_tlas_free(h)


def compile_ref_shim(d):
    """the reference, rounding once per operation; None when the reference is absent"""
    so = nb.compile_ref_shim(d, "custom_double_ref_shim.cpp", extra=("-ffp-contract=off",))
    return so and RefCustomDouble(so)


cd_ref = nb.ref_fixture("custom_double_ref", compile_ref_shim)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "custom_double")
GOLDEN_SETS = ("bunny", "soup")


def golden_rays(name, ocd):
    """the two batches a golden records (tools/make_custom_double_golden.py), every second ray of the GPU tests' batches"""
    sph = sphere_set(name)
    h = tb.host_build_custom_spheres_double(sph)
    cam = camera_rays(sph)
    return {"camera": decorate(cam, 3)[::2].copy(), "bounce": decorate(bounce_rays(sph, ocd.intersect(h.nodes(), h.prim_idx(), sph, cam, rule=1)), 4)[::2].copy()}


# ---- sphere sets ------------------------------------------------------------------------------------------------------------------------
def sphere_set(name):
    """(n, 4) float64 {x, y, z, r}"""
    if name == "bunny":      # the demos' sphere bunny, from the bunny's first triangles (float-exact values)
        return spheres_from_tris(bunny_verts()[: 3 * N_SPHERES], 1.2, 0.55).astype(np.float64)
    if name == "soup":       # a random cloud, overlapping spheres included
        rng = np.random.default_rng(7)
        return np.concatenate([rng.uniform(-10, 10, (N_SPHERES, 3)), rng.uniform(0.05, 0.8, (N_SPHERES, 1))], 1)
    if name == "small":      # the soup with r in [1e-3, 5e-2]: what is moved 1e7 units away
        rng = np.random.default_rng(11)
        return np.concatenate([rng.uniform(-1, 1, (N_SPHERES, 3)), rng.uniform(1e-3, 5e-2, (N_SPHERES, 1))], 1)
    if name == "dups":       # 64 exact duplicates: ties at equal distance, the smaller prim wins
        return np.tile([[0.5, 0.25, -0.5, 0.75]], (64, 1))
    if name == "one":
        return np.array([[0.5, 0.25, -0.5, 0.75]])
    raise KeyError(name)


def sphere_boxes(sph):
    sph = np.asarray(sph, np.float64).reshape(-1, 4)
    return sph[:, :3] - sph[:, 3:4], sph[:, :3] + sph[:, 3:4]


def camera_rays(sph, n=N_RAYS, seed=1):
    """constructor-made rays as the demos make them: a float-normalised D handed to RayEx( O, D ), which normalises again in double"""
    rng = np.random.default_rng(seed)
    lo, hi = sphere_boxes(sph)
    lo, hi = lo.min(0), hi.max(0)
    c, ext = (lo + hi) * 0.5, float((hi - lo).max())
    eye = (c + np.array([0.2, 0.35, 1.6]) * ext).astype(np.float32)
    k = rng.integers(0, len(sph), n)   # aimed at the spheres, a radius and a half around their centres: hits, grazing rays and near misses
    tgt = (np.asarray(sph)[k, :3] + rng.uniform(-1.5, 1.5, (n, 3)) * np.asarray(sph)[k, 3:4]).astype(np.float32)
    D = tgt - eye
    D = (D / np.sqrt((D * D).sum(1, dtype=np.float32))[:, None]).astype(np.float32)
    return tb.make_rays_ex(np.broadcast_to(eye.astype(np.float64), (n, 3)), D.astype(np.float64))


def bounce_rays(sph, traced, seed=5):
    """diffuse rays from the hit points (misses: a point in the set's box), pushed 1e-6 off the surface along the new direction"""
    rng = np.random.default_rng(seed)
    n = traced.shape[0]
    lo, hi = sphere_boxes(sph)
    hit = traced["t"] < 1e299
    P = np.where(hit[:, None], traced["O"] + np.where(hit, traced["t"], 0.0)[:, None] * traced["D"], rng.uniform(lo.min(0), hi.max(0), (n, 3)))
    Dn = rng.normal(size=(n, 3))
    Dn = np.where(((Dn * traced["D"]).sum(1) > 0)[:, None], -Dn, Dn)
    Dn /= np.linalg.norm(Dn, axis=1, keepdims=True)
    return tb.make_rays_ex(P + 1e-6 * Dn, Dn)


def decorate(rays, seed):
    """non-zero incoming u, v, inst, prim and instIdx, a quarter with a finite tmax: a hit must leave u, v alone and pass instIdx through"""
    rng = np.random.default_rng(seed)
    r = rays.copy()
    r["u"] = rng.uniform(0, 1, r.shape[0]); r["v"] = rng.uniform(0, 1, r.shape[0])
    r["instIdx"] = rng.integers(0, 1 << 40, r.shape[0]).astype(np.uint64)
    r["inst"] = 0xDEADBEEF; r["prim"] = 0xFFFFFFFFFF
    fin = rng.random(r.shape[0]) < 0.25
    r["t"][fin] = rng.uniform(0.5, 30, int(fin.sum()))
    return r


def translated(rays, offset):
    r = rays.copy()
    r["O"] = r["O"] + np.asarray(offset, np.float64)
    return r


# ---- trees ------------------------------------------------------------------------------------------------------------------------------
def karras_spheres(sph):
    """(nodes, prim_idx) over the sphere boxes exactly as the device builds them (double_anim_lib.karras_tlas fed the boxes pos -/+ r)"""
    boxes = np.zeros(np.asarray(sph).reshape(-1, 4).shape[0], _BOX_DTYPE)
    boxes["aabbMin"], boxes["aabbMax"] = sphere_boxes(sph)
    return karras_tlas(boxes)


def chain_tree(lo, hi):
    """A chain over len(lo) primitives with boxes [lo, hi]: interior k at 2 k (the root at 0), its leaf (primitive k) at 2 k + 1, the rest of the
    chain at 2 k + 2: len(lo) - 1 levels deep."""
    n = lo.shape[0]
    nodes = np.zeros(2 * n - 1, tb.NODE_DBL_DTYPE)
    for k in range(n - 1):
        nodes[2 * k + 1]["aabbMin"], nodes[2 * k + 1]["aabbMax"], nodes[2 * k + 1]["leftFirst"], nodes[2 * k + 1]["triCount"] = lo[k], hi[k], k, 1
        nodes[2 * k]["leftFirst"] = 2 * k + 1
    nodes[2 * n - 2]["aabbMin"], nodes[2 * n - 2]["aabbMax"], nodes[2 * n - 2]["leftFirst"], nodes[2 * n - 2]["triCount"] = lo[n - 1], hi[n - 1], n - 1, 1
    for k in reversed(range(n - 1)):
        c = 2 * k + 1
        nodes[2 * k]["aabbMin"] = np.minimum(nodes[c]["aabbMin"], nodes[c + 1]["aabbMin"])
        nodes[2 * k]["aabbMax"] = np.maximum(nodes[c]["aabbMax"], nodes[c + 1]["aabbMax"])
    return nodes


def chain_spheres(depth):
    """depth + 1 unit spheres on the z axis, 3 apart, under a chain `depth` levels deep: sphere k at z = 3 k, so a ray travelling in -z from above
    finds the chain's LAST sphere first and has pushed every leaf on the way"""
    sph = np.zeros((depth + 1, 4))
    sph[:, 2] = 3.0 * np.arange(depth + 1); sph[:, 3] = 1.0
    lo, hi = sphere_boxes(sph)
    return chain_tree(lo, hi), np.arange(depth + 1, dtype=np.uint64), sph


def check_tree(nodes, idx, sph):
    """every sphere in exactly one leaf, leaf boxes the union of pos -/+ r, interior boxes the union of the children's, in all bits"""
    lo, hi = sphere_boxes(sph)
    seen = np.zeros(len(nodes), bool); covered = np.zeros(len(lo), np.int64)
    stack = [0]
    while stack:
        i = stack.pop()
        assert not seen[i], i
        seen[i] = True
        f, c = int(nodes[i]["leftFirst"]), int(nodes[i]["triCount"])
        if c:
            p = np.asarray(idx[f:f + c]).astype(np.int64)
            covered[p] += 1
            assert np.array_equal(nodes[i]["aabbMin"], lo[p].min(0)) and np.array_equal(nodes[i]["aabbMax"], hi[p].max(0)), i
        else:
            assert 0 < f and f + 1 < len(nodes), (i, f)
            assert np.array_equal(nodes[i]["aabbMin"], np.minimum(nodes[f]["aabbMin"], nodes[f + 1]["aabbMin"])), i
            assert np.array_equal(nodes[i]["aabbMax"], np.maximum(nodes[f]["aabbMax"], nodes[f + 1]["aabbMax"])), i
            stack += [f, f + 1]
    assert (covered == 1).all()


def mismatches(a, b):
    x = np.ascontiguousarray(a).view(np.uint8).reshape(-1, 128); y = np.ascontiguousarray(b).view(np.uint8).reshape(-1, 128)
    return int((x != y).any(1).sum())


def same_records(got, want, what):
    a = np.ascontiguousarray(got).view(np.uint8).reshape(-1, 128); b = np.ascontiguousarray(want).view(np.uint8).reshape(-1, 128)
    bad = np.nonzero((a != b).any(1))[0]
    assert bad.size == 0, f"{what}: {bad.size} of {got.shape[0]} records differ, first {bad[:5].tolist()}: got {got[bad[:2]]} want {want[bad[:2]]}"


# ---- a two-level scene: one sphere BLAS and one triangle BLAS under six instances ---------------------------------------------------------
def tlas_scene():
    """(sph, verts, inst): the sphere soup scaled to a box of ~4 units, a triangle soup of the same size, and six instances: identity (spheres),
    translated by 1e7 (spheres), scaled x 2.5 (triangles), non-uniformly scaled (spheres), mirrored (triangles, placed inside the first
    instance), and one with mask = 0 (spheres)"""
    from double_lib import rotated_soup
    sph = sphere_set("soup")[:512] * 0.2
    verts = rotated_soup(600, seed=13) * 0.2
    T = np.tile(np.eye(4), (6, 1, 1))
    T[1, :3, 3] = FAR
    T[2, :3, :3] *= 2.5; T[2, :3, 3] = [9.0, 0.0, 0.0]
    T[3, :3, :3] = np.diag([0.5, 2.0, 1.25]); T[3, :3, 3] = [0.0, 9.0, 0.0]
    T[4, :3, :3] = np.diag([-1.0, 1.0, 1.0]); T[4, :3, 3] = [0.5, 0.0, 0.0]   # (inside instance 0: triangles in front of and behind spheres)
    T[5, :3, 3] = [0.0, -9.0, 0.0]
    inst = tb.make_instances_ex(T, [0, 0, 1, 0, 1, 0])
    inst["mask"] = [0x1, 0x2, 0x1, 0x2, 0x3, 0x0]   # a ray mask of 0x1 or 0x2 selects half of the instances
    return sph, verts, inst


def tlas_rays(inst, n=N_RAYS, seed=3):
    """rays aimed at the instances from around them, a sixth from inside each instance's box; half carry mask 0x1, half 0x2"""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, inst.shape[0], n)
    lo, hi = inst["aabbMin"][k], inst["aabbMax"][k]
    c, ext = 0.5 * (lo + hi), (hi - lo)
    inside = rng.random(n) < 0.3
    O = np.where(inside[:, None], c + rng.uniform(-0.45, 0.45, (n, 3)) * ext, c + rng.normal(size=(n, 3)) * ext.max(1, keepdims=True) * 1.5)
    tgt = c + rng.uniform(-0.5, 0.5, (n, 3)) * ext
    rays = tb.make_rays_ex(O, np.where(inside[:, None], rng.normal(size=(n, 3)), tgt - O))
    rays["mask"] = np.where(np.arange(n) % 2 == 0, 0x1, 0x2)
    return rays
