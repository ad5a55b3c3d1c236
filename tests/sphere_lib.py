"""Shared pieces of the sphere-query tests: the restatement (tests/oracle_sphere.c) and the real reference behind tests/sphere_ref_shim.cpp,
both compiled per session into a pytest temp dir, the meshes, the seeded sphere sets and the rounding class of DESIGN.md par. 11."""
import ctypes as C
import os

import numpy as np

import native_build as nb
from native_build import _i, _p, _u64, _vp
from tinybvh_amd import scenes

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "spheres")


class SphereOracle:
    """oracle_sphere.c.  Every call returns one uint8 per sphere."""

    def __init__(self, so):
        self.lib = C.CDLL(so)
        L = self.lib
        L.sph_flat.argtypes = [_vp, _vp, _u64, _vp, _u64, _vp, _u64, _vp]
        L.sph_wald.argtypes = [_vp, _u64, _vp, _u64, _vp, _u64, _vp, _u64, _i, _vp]
        L.sph_bvhgpu.argtypes = [_vp, _vp, _vp, _u64, _vp, _u64, _vp]
        L.sph_bvh4.argtypes = [_vp, _vp, _u64, _vp, _u64, _vp]
        L.sph_cwbvh.argtypes = [_vp, _vp, _vp, _u64, _vp, _u64, _vp]
        L.sph_last_max_stack.restype = C.c_uint32

    def last_max_stack(self):
        """the most node / leaf entries the last BVH4_GPU or CWBVH call held on its stack at once (leaf entries counted only as nodes push them)"""
        return int(self.lib.sph_last_max_stack())

    @staticmethod
    def _in(verts, spheres):
        verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 4)
        spheres = np.ascontiguousarray(spheres, np.float32).reshape(-1, 4)
        return verts, spheres, np.zeros(spheres.shape[0], np.uint8)

    def flat(self, box6, prim_idx, verts, spheres):
        verts, spheres, out = self._in(verts, spheres)
        box6 = np.ascontiguousarray(box6, np.float32).reshape(6)
        pi = np.ascontiguousarray(prim_idx, np.uint32).reshape(-1)
        self.lib.sph_flat(_p(box6), _p(pi), pi.size, _p(verts), verts.shape[0] // 3, _p(spheres), spheres.shape[0], _p(out))
        return out

    def wald(self, nodes32, prim_idx, verts, spheres, mode=1):
        """mode 0: the reference verbatim (0 / 1, | 4 once it took a leaf off the stack, 2 = undefined); 1: the library's walk"""
        verts, spheres, out = self._in(verts, spheres)
        n = np.ascontiguousarray(nodes32).view(np.uint32).reshape(-1, 8)
        pi = np.ascontiguousarray(prim_idx, np.uint32).reshape(-1)
        self.lib.sph_wald(_p(n), n.shape[0], _p(pi), pi.size, _p(verts), verts.shape[0] // 3, _p(spheres), spheres.shape[0], mode, _p(out))
        return out

    def bvhgpu(self, nodes64, prim_idx, verts, spheres):
        verts, spheres, out = self._in(verts, spheres)
        n = np.ascontiguousarray(nodes64).view(np.uint32)
        pi = np.ascontiguousarray(prim_idx, np.uint32).reshape(-1)
        self.lib.sph_bvhgpu(_p(n), _p(pi), _p(verts), verts.shape[0] // 3, _p(spheres), spheres.shape[0], _p(out))
        return out

    def bvh4(self, blocks16, verts, spheres):
        verts, spheres, out = self._in(verts, spheres)
        b = np.ascontiguousarray(blocks16).view(np.uint32)
        self.lib.sph_bvh4(_p(b), _p(verts), verts.shape[0] // 3, _p(spheres), spheres.shape[0], _p(out))
        return out

    def cwbvh(self, nodes16, tris16, verts, spheres):
        verts, spheres, out = self._in(verts, spheres)
        n, t = np.ascontiguousarray(nodes16).view(np.uint32), np.ascontiguousarray(tris16).view(np.uint32)
        self.lib.sph_cwbvh(_p(n), _p(t), _p(verts), verts.shape[0] // 3, _p(spheres), spheres.shape[0], _p(out))
        return out

    def layout(self, layout, blobs, verts, spheres):
        """the restatement of one GPU layout over its blobs: 5 = (nodes64, primIdx), 8 = (blocks16,), 10 = (nodes16, tris16)"""
        if layout == 5:
            return self.bvhgpu(blobs[0], blobs[1], verts, spheres)
        if layout == 8:
            return self.bvh4(blobs[0], verts, spheres)
        return self.cwbvh(blobs[0], blobs[1], verts, spheres)


class RefSpheres:
    """The real reference (sphere_ref_shim.cpp)."""

    def __init__(self, so):
        self.lib = C.CDLL(so)
        L = self.lib
        L.sref_build.argtypes = [_vp, C.c_uint32, _i]
        L.sref_build.restype = _vp
        L.sref_free.argtypes = [_vp]
        L.sref_blob.argtypes = [_vp, _i, C.POINTER(_vp)]
        L.sref_blob.restype = _u64
        L.sref_intersect_spheres.argtypes = [_vp, _vp, _u64, _vp]
        L.sref_intersect_spheres_flat.argtypes = [_vp, _vp, _u64, _vp]
        L.sref_used_indices.argtypes = [_vp]
        L.sref_used_indices.restype = C.c_uint32

    def build(self, verts, hq):
        verts = np.ascontiguousarray(verts, np.float32)
        return self.lib.sref_build(_p(verts), verts.shape[0] // 3, 1 if hq else 0)

    def free(self, h):
        self.lib.sref_free(h)

    def blob(self, h, which):
        """0 Wald nodes (n, 8) u32, 1 primIdx (n,) u32, 2 BVH_GPU nodes (n, 16) u32, 3 BVH4_GPU blocks (n, 4), 4 / 5 CWBVH nodes / tris (n, 4)"""
        p = _vp()
        n = self.lib.sref_blob(h, which, C.byref(p))
        if which == 1:
            n = self.lib.sref_used_indices(h)   # (BuildHQ: the entries past the leaves' extent are slack)
        width = {0: 8, 1: 1, 2: 16}.get(which, 4)
        a = np.ctypeslib.as_array((C.c_uint32 * (n * width)).from_address(p.value)).reshape(n, width).copy()
        return a.reshape(-1) if which == 1 else a

    def intersect(self, h, spheres):
        """BVH::IntersectSphere: only for spheres the verbatim restatement has shown to terminate"""
        spheres = np.ascontiguousarray(spheres, np.float32)
        out = np.zeros(spheres.shape[0], np.uint8)
        self.lib.sref_intersect_spheres(h, _p(spheres), spheres.shape[0], _p(out))
        return out

    def intersect_flat(self, h, spheres):
        spheres = np.ascontiguousarray(spheres, np.float32)
        out = np.zeros(spheres.shape[0], np.uint8)
        self.lib.sref_intersect_spheres_flat(h, _p(spheres), spheres.shape[0], _p(out))
        return out


def compile_oracle(d):
    return SphereOracle(nb.compile_c_oracle(d, "oracle_sphere"))


def compile_ref_shim(d):
    """the reference with oracle/Makefile's flags; None when the reference is absent"""
    so = nb.compile_ref_shim(d, "sphere_ref_shim.cpp")
    return so and RefSpheres(so)


sph_oracle = nb.oracle_fixture("oracle_sphere", compile_oracle)
sph_ref = nb.ref_fixture("sphere_ref", compile_ref_shim)


# ---- meshes ---------------------------------------------------------------------------------------------------------------------------
def bunny():
    """the reference's testdata/bunny.bin, bit for bit (tests/golden/meshes/bunny.npz)"""
    g = np.load(os.path.join(HERE, "golden", "meshes", "bunny.npz"))
    verts = np.empty((g["indices"].size, 4), np.float32)
    verts[:, :3] = g["positions"][g["indices"].ravel()]
    verts[:, 3] = g["w_bits"].view(np.float32)[0]
    return verts


def with_degenerate(verts, seed=5):
    """the mesh plus a few zero-area triangles (a repeated vertex, three equal vertices, collinear vertices)"""
    rng = np.random.default_rng(seed)
    t = verts.reshape(-1, 3, 4)
    extra = []
    for k in rng.choice(t.shape[0], 6, replace=False):
        a, b = t[k, 0].copy(), t[k, 1].copy()
        extra += [np.stack([a, a, b]), np.stack([a, a, a]), np.stack([a, b, a + np.float32(2.0) * (b - a)])]
    return np.ascontiguousarray(np.concatenate([t, np.stack(extra)]).reshape(-1, 4), np.float32)


def mesh(name):
    if name == "bunny":
        return bunny()
    if name == "atrium":
        return with_degenerate(scenes.atrium(6_000, seed=1))
    if name == "soup":
        return with_degenerate(scenes.soup(3_000, seed=7))
    if name == "tri1":
        return np.array([[0, 0, 0, 0], [1, 0, 0, 0], [0, 1, 0.25, 0]], np.float32)
    if name == "tri2":
        return np.array([[0, 0, 0, 0], [1, 0, 0, 0], [0, 1, 0.25, 0], [2, 2, 1, 0], [3, 2, 1, 0], [2, 3, 1.5, 0]], np.float32)
    raise KeyError(name)


MESHES = ["bunny", "atrium", "soup", "tri1", "tri2"]


# ---- sphere sets ----------------------------------------------------------------------------------------------------------------------
def point_tri_dist(p, tris):
    """exact-enough fp64 distance from points p (n, 3) to the nearest of triangles tris (m, 3, 3) (Ericson, Real-Time Collision Detection 5.1.5)"""
    p = np.asarray(p, np.float64)[:, None, :]
    a, b, c = (np.asarray(tris[:, k, :3], np.float64)[None] for k in range(3))
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = (ab * ap).sum(-1), (ac * ap).sum(-1)
    bp = p - b
    d3, d4 = (ab * bp).sum(-1), (ac * bp).sum(-1)
    cp = p - c
    d5, d6 = (ab * cp).sum(-1), (ac * cp).sum(-1)
    va, vb, vc = d3 * d6 - d5 * d4, d5 * d2 - d1 * d6, d1 * d4 - d3 * d2
    with np.errstate(divide="ignore", invalid="ignore"):
        denom = va + vb + vc
        v = np.where(denom != 0, vb / denom, 0.0)
        w = np.where(denom != 0, vc / denom, 0.0)
        q = a + ab * v[..., None] + ac * w[..., None]   # interior
        # edges and vertices
        cand = [a, b, c]
        for s0, s1 in ((a, b), (b, c), (c, a)):
            e = s1 - s0
            ee = (e * e).sum(-1)
            t = np.clip(np.where(ee > 0, ((p - s0) * e).sum(-1) / np.where(ee > 0, ee, 1), 0.0), 0, 1)
            cand.append(s0 + e * t[..., None])
        inside = (va >= 0) & (vb >= 0) & (vc >= 0) & (denom > 0)
        dist = np.min(np.stack([np.sqrt(((p - x) ** 2).sum(-1)) for x in cand]), 0)
        di = np.sqrt(((p - q) ** 2).sum(-1))
        dist = np.where(inside, np.minimum(dist, di), dist)
    return dist.min(1)


def nearest_dist(verts, pos, chunk=64):
    tris = np.asarray(verts, np.float32).reshape(-1, 3, 4)
    out = []
    for k in range(0, len(pos), chunk):
        out.append(point_tri_dist(pos[k:k + chunk], tris))
    return np.concatenate(out) if out else np.zeros(0)


def random_spheres(verts, n, seed):
    """centres around the mesh's box, radii across scales (1e-4 .. 0.3 of the box diagonal)"""
    rng = np.random.default_rng(seed)
    v = verts[:, :3]
    lo, hi = v.min(0), v.max(0)
    diag = float(np.linalg.norm(hi - lo))
    pos = lo - 0.05 * (hi - lo) + rng.random((n, 3)) * 1.1 * (hi - lo)
    r = diag * 10.0 ** rng.uniform(-4, np.log10(0.3), n)
    return np.ascontiguousarray(np.concatenate([pos, r[:, None]], 1), np.float32)


def knife_edge_spheres(verts, n, seed):
    """r = the fp64 distance from the centre to a chosen triangle, then -4 .. +4 ulps of it"""
    rng = np.random.default_rng(seed)
    tris = verts.reshape(-1, 3, 4)
    v = verts[:, :3]
    scale = float(np.linalg.norm(v.max(0) - v.min(0)))
    k = rng.choice(tris.shape[0], n)
    w = rng.dirichlet(np.ones(3), n)
    onto = (tris[k, :, :3].astype(np.float64) * w[:, :, None]).sum(1)
    pos = (onto + rng.normal(0, 1, (n, 3)) * scale * 10.0 ** rng.uniform(-4, -1.5, (n, 1))).astype(np.float32)
    d = np.array([point_tri_dist(pos[i:i + 1], tris[k[i]:k[i] + 1])[0] for i in range(n)])
    r = d.astype(np.float32)
    out = []
    for ulps in range(-4, 5):
        rr = r.copy()
        step = np.float32(np.inf) if ulps > 0 else np.float32(-np.inf)
        for _ in range(abs(ulps)):
            rr = np.nextafter(rr, step).astype(np.float32)
        out.append(np.concatenate([pos, rr[:, None]], 1))
    return np.ascontiguousarray(np.concatenate(out), np.float32)


def wall_spheres(nodes32, n, seed):
    """spheres whose box touches a Wald node box face exactly (pos = face -/+ r with r a power of two, so the subtraction is exact)"""
    rng = np.random.default_rng(seed)
    f = np.ascontiguousarray(nodes32).view(np.float32).reshape(-1, 8)
    leaf = np.ascontiguousarray(nodes32).view(np.uint32).reshape(-1, 8)[:, 7] > 0
    boxes = f[np.flatnonzero(leaf)]
    pick = boxes[rng.choice(boxes.shape[0], n)]
    axis = rng.integers(0, 3, n)
    side = rng.integers(0, 2, n)
    ext = np.maximum(pick[:, 4:7] - pick[:, 0:3], 1e-6)
    r = np.exp2(np.round(np.log2(ext.max(1) * rng.uniform(0.3, 2.0, n)))).astype(np.float32)
    pos = (pick[:, 0:3] + pick[:, 4:7]) * np.float32(0.5)
    for i in range(n):
        a = axis[i]
        # side 0: bmax.a = pos + r lands on the box's min face; side 1: bmin.a = pos - r lands on its max face
        pos[i, a] = pick[i, a] - r[i] if side[i] == 0 else pick[i, 4 + a] + r[i]
    return np.ascontiguousarray(np.concatenate([pos, r[:, None]], 1), np.float32)


def degenerate_spheres(verts, seed):
    """r = 0 and r < 0 (on and near the surface), NaN / inf components, one sphere containing the scene, spheres far away"""
    rng = np.random.default_rng(seed)
    tris = verts.reshape(-1, 3, 4)
    v = verts[:, :3]
    lo, hi = v.min(0), v.max(0)
    ctr, diag = (lo + hi) * np.float32(0.5), float(np.linalg.norm(hi - lo))
    on = tris[rng.choice(tris.shape[0], 16), 0, :3]
    s = []
    for p in on:
        s += [[*p, 0.0], [*p, -0.0], [*p, -diag * 0.01], [*p, -diag]]
    s += [[*ctr, 0.0], [*ctr, -1e-3], [*ctr, diag], [*ctr, 2 * diag], [*ctr, np.inf], [*ctr, -np.inf], [*ctr, np.nan]]
    s += [[np.nan, ctr[1], ctr[2], diag], [ctr[0], np.inf, ctr[2], 1.0], [ctr[0], ctr[1], -np.inf, 1.0], [np.inf, np.inf, np.inf, np.inf]]
    s += [[*(ctr + np.float32(10 * diag)), diag], [*(ctr - np.float32(1e6)), 1.0], [1e30, 1e30, 1e30, 1e29], [*ctr, 1e30]]
    return np.ascontiguousarray(np.array(s, np.float32))


def sphere_sets(verts, nodes32, seed, n=1500):
    return {
        "random": random_spheres(verts, n, seed),
        "knife": knife_edge_spheres(verts, max(n // 9, 40), seed + 1),
        "wall": wall_spheres(nodes32, max(n // 3, 64), seed + 2),
        "degenerate": degenerate_spheres(verts, seed + 3),
    }


# ---- the rounding class (DESIGN.md par. 11) -------------------------------------------------------------------------------------------
def box_faces(layout, blobs):
    """per axis, every box face (min and max planes) of the layout's child boxes, dequantised as the kernels do it"""
    faces = [set(), set(), set()]
    if layout == 1:
        f = np.ascontiguousarray(blobs[0]).view(np.float32).reshape(-1, 8)
        for a in range(3):
            faces[a].update(f[:, a].tolist()); faces[a].update(f[:, 4 + a].tolist())
    elif layout == 5:
        f = np.ascontiguousarray(blobs[0]).view(np.float32).reshape(-1, 16)
        for a in range(3):
            for o in (0, 4, 8, 12):
                faces[a].update(f[:, o + a].tolist())
    elif layout == 8:
        b = np.ascontiguousarray(blobs[0]).view(np.uint32).reshape(-1, 4)
        f = b.view(np.float32)
        off = 0
        nb = b.shape[0]
        stack = [0]
        while stack:
            off = stack.pop()
            d0, d1, d2, d3 = f[off], f[off + 1], b[off + 2], b[off + 3]
            q = [(int(b[off, 3]), int(b[off + 1, 3])), (int(d2[0]), int(d2[1])), (int(d2[2]), int(d2[3]))]
            for i in range(4):
                if d3[i] == 0:
                    continue
                for a in range(3):
                    for w in q[a]:
                        faces[a].add(float(np.float32(d0[a]) + np.float32((w >> (8 * i)) & 255) * np.float32(d1[a])))
                if not d3[i] & 0x80000000:
                    stack.append(int(d3[i]))
        assert off < nb
    else:
        n = np.ascontiguousarray(blobs[0]).view(np.uint32).reshape(-1, 20)
        f = n.view(np.float32)
        for node in range(n.shape[0]):
            ew = int(n[node, 3])
            for a in range(3):
                e = ((ew >> (8 * a)) & 255)
                e = e - 256 if e >= 128 else e
                sc = np.ldexp(np.float32(1.0), e).astype(np.float32)
                for word in (8 + 2 * a, 9 + 2 * a, 14 + 2 * a, 15 + 2 * a):
                    w = int(n[node, word])
                    for i in range(4):
                        faces[a].add(float(np.float32(f[node, a]) + np.float32((w >> (8 * i)) & 255) * sc))
    return faces


def zero_area_prims(verts):
    """the triangles whose edge cross product is exactly zero: the reference's test has no plane axis for them and answers yes for some
    spheres that do not reach them (defect 2 of DESIGN.md par. 11)"""
    t = np.asarray(verts, np.float64).reshape(-1, 3, 4)[:, :, :3]
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    return np.flatnonzero((n * n).sum(1) == 0).astype(np.uint32)


def zero_area_yes(oracle, spheres, verts):
    """bool per sphere: the reference's triangle test answers yes for one of the mesh's zero-area triangles"""
    deg = zero_area_prims(verts)
    if deg.size == 0:
        return np.zeros(np.asarray(spheres).shape[0], bool)
    return oracle.flat(np.array([-np.inf] * 3 + [np.inf] * 3, np.float32), deg, verts, spheres) == 1


def in_rounding_class(spheres, verts, faces_list, rel=1e-5):
    """bool per sphere: the exact distance to the nearest triangle is within rel * max(r, 1) of r, or a face of the sphere's box equals a box
    face (of any of the given face sets) exactly"""
    s = np.asarray(spheres, np.float32)
    if s.shape[0] == 0:
        return np.zeros(0, bool)
    d = nearest_dist(verts, s[:, :3])
    r = s[:, 3].astype(np.float64)
    near = np.abs(d - r) <= rel * np.maximum(np.abs(r), 1.0)
    bmin, bmax = s[:, :3] - s[:, 3:4], s[:, :3] + s[:, 3:4]
    face = np.zeros(s.shape[0], bool)
    for faces in faces_list:
        for a in range(3):
            fa = faces[a]
            face |= np.array([float(x) in fa or float(y) in fa for x, y in zip(bmin[:, a], bmax[:, a])])
    return near | face
