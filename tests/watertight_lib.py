"""Shared by the watertight-mode tests (test_watertight_host.py, test_watertight_gpu.py), tools/make_watertight_golden.py and tools/watertight_bench.py (so:
NumPy and the compilers only, no GPU library): the closed star meshes and the rays aimed at their vertices and edges, the real reference behind
tests/watertight_ref_shim.cpp in its three builds (compiled per session into a pytest temp dir when the reference checkout is present; nothing of it is kept),
the session fixtures over them, and the goldens under tests/golden/watertight (DESIGN.md par. 4.6).

The star mesh: the surface lattice of a cube with N cells per edge, every vertex a pure function of its integer lattice coordinates — direction from the cube's
centre, radius 1 + 0.15 hash, a non-uniform scale, an offset — looked up in ONE table, so the vertices two triangles share are the same bits.  2 * 6 * N^2
triangles.  Star-shaped about its centre: from an eye near the centre every ray hits it."""
import ctypes as C
import os

import numpy as np

import native_build as nb
from native_build import _p, _u32, _u64

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "watertight")
F = np.float32
SCALE = np.array([1.3, 0.8, 1.1], F)
OFFSET = np.array([0.37, -1.21, 2.6], F)
EYES = np.array([[0.0, 0.0, 0.0], [0.21, -0.13, 0.17], [-0.3, 0.22, -0.11]], F)   # relative to the centre, before scale: well inside radius 0.85
N_RANDOM = 4096
RAY_DTYPE = np.dtype([("O", "<f4", 3), ("mask", "<u4"), ("D", "<f4", 3), ("instIdx", "<u4"), ("rD", "<f4", 3), ("inst", "<u4"),
                      ("t", "<f4"), ("u", "<f4"), ("v", "<f4"), ("prim", "<u4")])
BVH_FAR = F(1e30)


# ---- meshes --------------------------------------------------------------------------------------------------------------------------------------------
def _hash01(i, j, k, salt):
    h = (i.astype(np.uint64) * 73856093) ^ (j.astype(np.uint64) * 19349663) ^ (k.astype(np.uint64) * 83492791) ^ np.uint64(salt * 2654435761 & 0xFFFFFFFF)
    h = (h ^ (h >> np.uint64(13))) * np.uint64(1274126177) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(16)
    return ((h & np.uint64(0xFFFF)).astype(F) / F(65535.0)).astype(F)


def vertex_table(N, salt=0, displace=0.0):
    """(N + 1, N + 1, N + 1, 3) float32: the vertex of every lattice point (only the surface ones are used).  displace: a second per-vertex radius term, for
    the meshes that move — the moved mesh is again a pure function of the lattice coordinates."""
    g = np.arange(N + 1)
    i, j, k = np.meshgrid(g, g, g, indexing="ij")
    p = np.stack([i, j, k], -1).astype(F) * F(2.0 / N) - F(1.0)
    l = np.sqrt((p * p).sum(-1, dtype=F)).astype(F)
    l = np.where(l == 0, F(1), l)
    r = (F(1.0) + F(0.15) * _hash01(i, j, k, salt) + F(displace) * _hash01(i, j, k, salt + 77)).astype(F)
    return ((p / l[..., None]) * r[..., None] * SCALE + OFFSET).astype(F)


def quads(N):
    """(6 N^2, 4, 3) int: the lattice coordinates of each surface quad's corners c00, c10, c11, c01"""
    out = []
    a, b = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    a, b = a.reshape(-1), b.reshape(-1)
    for axis in range(3):
        for side in (0, N):
            q = np.zeros((a.size, 4, 3), np.int64)
            u, v = (axis + 1) % 3, (axis + 2) % 3
            for c, (da, db) in enumerate(((0, 0), (1, 0), (1, 1), (0, 1))):
                q[:, c, axis] = side; q[:, c, u] = a + da; q[:, c, v] = b + db
            out.append(q)
    return np.concatenate(out)


def star(N, salt=0, displace=0.0):
    """(3 n, 4) float32 vertices, 3 per triangle (w = 0): the quads' two triangles (c00, c10, c11) and (c00, c11, c01)"""
    tab = vertex_table(N, salt, displace)
    q = quads(N)
    P = tab[q[..., 0], q[..., 1], q[..., 2]]                        # (nq, 4, 3)
    tris = np.stack([P[:, [0, 1, 2]], P[:, [0, 2, 3]]], 1).reshape(-1, 3)   # (nq * 2 * 3, 3)
    v = np.zeros((tris.shape[0], 4), F)
    v[:, :3] = tris
    return np.ascontiguousarray(v)


def make_rays(O, D, tmax=BVH_FAR):
    """ray records as the tinybvh::Ray constructor makes them (normalised D, rD = tinybvh_safercp( D ))"""
    O = np.ascontiguousarray(O, F).reshape(-1, 3); D = np.ascontiguousarray(D, F).reshape(-1, 3)
    l = np.sqrt((D * D).sum(1, dtype=F)).astype(F)
    D = (D * (F(1) / np.where(l == 0, F(1), l))[:, None]).astype(F)
    big = np.abs(D) > F(1e-12)
    with np.errstate(divide="ignore"):
        rD = np.where(big, F(1) / np.where(big, D, F(1)), np.where(D >= 0, BVH_FAR, -BVH_FAR)).astype(F)
    r = np.zeros(O.shape[0], RAY_DTYPE)
    r["O"] = O; r["D"] = D; r["rD"] = rD; r["mask"] = 0xFFFF; r["t"] = tmax
    return r


def eyes():
    return (EYES * SCALE + OFFSET).astype(F)


def aimed_rays(N, salt=0, displace=0.0):
    """Per quad six targets — the corner c00, the midpoints of its edges c00-c10 and c00-c01 and of the diagonal c00-c11 (all three are triangle edges), the
    points 0.75 along c00-c10 and 0.7 along c10-c11 — from each of the three eyes: 108 N^2 rays, every one of which must hit the closed mesh."""
    tab = vertex_table(N, salt, displace)
    q = quads(N)
    P = tab[q[..., 0], q[..., 1], q[..., 2]]
    c00, c10, c11, c01 = P[:, 0], P[:, 1], P[:, 2], P[:, 3]
    tg = np.stack([c00, (c00 + c10) * F(0.5), (c00 + c01) * F(0.5), (c00 + c11) * F(0.5), c00 + (c10 - c00) * F(0.75), c10 + (c11 - c10) * F(0.7)], 1).astype(F)
    tg = tg.reshape(-1, 3)
    E = eyes()
    O = np.repeat(E, tg.shape[0], 0)
    T = np.tile(tg, (E.shape[0], 1))
    return make_rays(O, T - O)


def random_rays(seed):
    rng = np.random.default_rng(seed)
    E = eyes()
    O = E[rng.integers(0, E.shape[0], N_RANDOM)]
    return make_rays(O, rng.normal(size=(N_RANDOM, 3)).astype(F))


def checker_map(n_tris, N=4):
    """an opacity micromap of N x N bits per triangle: micro-triangle k is opaque iff (k + triangle) is even"""
    wpt = (N * N + 31) // 32
    m = np.zeros((n_tris, wpt), np.uint32)
    for k in range(N * N):
        on = ((np.arange(n_tris) + k) % 2 == 0)
        m[on, k >> 5] |= np.uint32(1 << (k & 31))
    return m


def interior_edges(N):
    """every edge two triangles of star(N) share, as (triangle a, its edge, triangle b, its edge, same direction?): edge k of a triangle runs from corner k to
    corner (k + 1) % 3; found by the vertices' bits"""
    v = star(N)[:, :3].reshape(-1, 3, 3)
    key = np.ascontiguousarray(v).view(np.uint32).reshape(-1, 3, 3)
    seen, out = {}, []
    for t in range(key.shape[0]):
        for a, b in ((0, 1), (1, 2), (2, 0)):
            ka, kb = tuple(key[t, a]), tuple(key[t, b])
            e = (ka, kb) if ka < kb else (kb, ka)
            if e in seen:
                t0, a0, fwd0 = seen[e]
                out.append((t0, a0, t, a, fwd0 == (ka < kb)))
            else:
                seen[e] = (t, a, ka < kb)
    return out


# ---- the real reference --------------------------------------------------------------------------------------------------------------------------------
TRI_OCCLUDES_GAP = b"if (t < 0 || t > ray.hit.t) return false;"
TRI_OCCLUDES_FIX = b"\tconst float u = U * invDet, v = V * invDet;"


def patched_header(d):
    """Under WATERTIGHT_TRITEST the reference's TriOccludes never declares the u, v its micromap lookup reads, so the define does not compile as shipped.
    Writes a copy of tiny_bvh.h with that one line inserted behind the watertight branch's range test, and nothing else touched, into d; d then goes FIRST on
    the include path.  Nothing of it is kept."""
    with open(os.path.join(nb.reference_dir(), "tiny_bvh.h"), "rb") as f:
        lines = f.read().split(b"\n")
    at = [k for k, line in enumerate(lines) if line.strip() == TRI_OCCLUDES_GAP]
    assert len(at) == 1, "the watertight branch of TriOccludes is not where it was"
    lines.insert(at[0] + 1, TRI_OCCLUDES_FIX)
    with open(os.path.join(str(d), "tiny_bvh.h"), "wb") as f:
        f.write(b"\n".join(lines))
    return str(d)


class Ref:
    def __init__(self, so):
        self.lib = L = C.CDLL(so)
        L.wref_watertight.restype = C.c_int
        for f in (L.wref_pairs, L.wref_brute, L.wref_bvh, L.wref_edge, L.wref_brute_tlas):
            f.restype = None
        self.watertight = bool(L.wref_watertight())

    def pairs(self, rays, tris9):
        """(accept, tuv, occ) of ray i against triangle i"""
        rays = np.ascontiguousarray(rays); tris9 = np.ascontiguousarray(tris9, F).reshape(-1, 9)
        n = rays.shape[0]
        acc, tuv, occ = np.zeros(n, np.uint8), np.zeros((n, 3), F), np.zeros(n, np.uint8)
        self.lib.wref_pairs(_p(rays), _p(tris9), _u64(n), _p(acc), _p(tuv), _p(occ))
        return acc, tuv, occ

    def edge(self, rays, pq6):
        """the edge function of the directed edge P -> Q of pair i as ray i sees it, as THIS build contracts the expression Px * Qy - Py * Qx; the sheared
        coordinates are computed here, every operation rounded once (numpy float32), with the ray's precalculation as device_common.h: wt_precalc states it"""
        pq6 = np.ascontiguousarray(pq6, F).reshape(-1, 6)
        D, rD, O = rays["D"], rays["rD"], rays["O"]
        n = np.arange(D.shape[0])
        aD = np.abs(D)
        r = np.where(aD[:, 0] > aD[:, 1], 0, 1)
        kz = np.where(aD[:, 2] > aD[n, r], 2, r)
        kx = (1 << kz) & 3; ky = (1 << kx) & 3
        neg = D[n, kz] < 0
        kx, ky = np.where(neg, ky, kx), np.where(neg, kx, ky)
        Sz = rD[n, kz]; Sx = (D[n, kx] * Sz).astype(F); Sy = (D[n, ky] * Sz).astype(F)
        out = []
        for v in (pq6[:, :3], pq6[:, 3:]):
            A = (v - O).astype(F)
            out += [(A[n, kx] - (Sx * A[n, kz]).astype(F)).astype(F), (A[n, ky] - (Sy * A[n, kz]).astype(F)).astype(F)]
        pq4 = np.ascontiguousarray(np.stack(out, 1), F)
        e = np.zeros(pq4.shape[0], F)
        self.lib.wref_edge(_p(pq4), _u64(pq4.shape[0]), _p(e))
        return e

    def brute(self, verts, rays, opmap=None, N=0):
        """(records, occlusion flags): every triangle in index order"""
        verts = np.ascontiguousarray(verts, F); out = np.ascontiguousarray(rays).copy()
        occ = np.zeros(out.shape[0], np.uint8)
        m = None if opmap is None else np.ascontiguousarray(opmap, np.uint32)
        self.lib.wref_brute(_p(verts), _u32(verts.shape[0] // 3), _p(out), _u64(out.shape[0]), _p(occ), None if m is None else _p(m), _u32(N))
        return out, occ

    def brute_tlas(self, blas_verts, inv_transforms, inst_blas, rays):
        """(records with the winning instance in "inst", occlusion flags): every instance in index order, every triangle of its BLAS in index order"""
        vs = [np.ascontiguousarray(v, F) for v in blas_verts]
        ptrs = (C.c_void_p * len(vs))(*[v.ctypes.data for v in vs])
        nt = np.array([v.shape[0] // 3 for v in vs], np.uint32)
        inv = np.ascontiguousarray(inv_transforms, F).reshape(-1, 16); ib = np.ascontiguousarray(inst_blas, np.uint32)
        out = np.ascontiguousarray(rays).copy()
        occ = np.zeros(out.shape[0], np.uint8)
        self.lib.wref_brute_tlas(ptrs, _p(nt), _p(inv), _p(ib), _u32(ib.size), _p(out), _u64(out.shape[0]), _p(occ))
        return out, occ

    def bvh(self, verts, rays, hq=False):
        verts = np.ascontiguousarray(verts, F); out = np.ascontiguousarray(rays).copy()
        occ = np.zeros(out.shape[0], np.uint8)
        self.lib.wref_bvh(_p(verts), _u32(verts.shape[0] // 3), C.c_int(1 if hq else 0), _p(out), _u64(out.shape[0]), _p(occ))
        return out, occ


def compile_ref_shims(d):
    """{"wt": uncontracted watertight, "wt_fma": watertight as the usual flags build it, "mt": Moeller-Trumbore}, or None when the reference is absent"""
    if not nb.have_reference():
        return None
    inc = ("-iquote", patched_header(d))   # (quote includes look there before any -I directory, the reference's own included)
    out = {}
    for name, defines, extra in (("wt", ("WATERTIGHT_TRITEST",), ("-ffp-contract=off",)), ("wt_fma", ("WATERTIGHT_TRITEST",), ()), ("mt", (), ())):
        so = nb.compile_ref_shim(d, "watertight_ref_shim.cpp", out="watertight_ref_" + name, defines=defines, extra=inc + extra)
        out[name] = Ref(so)
    assert out["wt"].watertight and out["wt_fma"].watertight and not out["mt"].watertight
    return out


watertight_refs = nb.ref_fixture("watertight_ref", compile_ref_shims)


# ---- the two-level fixture ----------------------------------------------------------------------------------------------------------------------------------
TLAS_BLAS = (4, 12)            # BLAS 0 = star4, BLAS 1 = star12
TLAS_INST_BLAS = (0, 1, 1)
TLAS_RANDOM = 2048


def tlas_transforms():
    """(3, 4, 4) float32, row-major: the identity; a rotation about (1, 2, 3) by 0.7 with the scale (1.5, 0.6, 1.1), moved to (7, 1, -2); and a mirrored one
    (x scaled by -0.8: negative determinant) rotated about z by 0.4, moved to (-6, 2, 3)"""
    def rot(axis, a):
        x, y, z = np.asarray(axis, np.float64) / np.linalg.norm(axis)
        c, s = np.cos(a), np.sin(a)
        return np.array([[c + x * x * (1 - c), x * y * (1 - c) - z * s, x * z * (1 - c) + y * s], [y * x * (1 - c) + z * s, c + y * y * (1 - c), y * z * (1 - c) - x * s],
                         [z * x * (1 - c) - y * s, z * y * (1 - c) + x * s, c + z * z * (1 - c)]])
    T = np.tile(np.eye(4), (3, 1, 1))
    T[1, :3, :3] = rot((1, 2, 3), 0.7) @ np.diag([1.5, 0.6, 1.1]); T[1, :3, 3] = (7, 1, -2)
    T[2, :3, :3] = rot((0, 0, 1), 0.4) @ np.diag([-0.8, 1.0, 1.2]); T[2, :3, 3] = (-6, 2, 3)
    return T.astype(F)


def tlas_instances():
    """(INSTANCE_DTYPE records with invTransform and bounds as the library's host TLAS builder leaves them — BLASInstance::Update —, the BLASes' vertices)"""
    import ctypes
    import tinybvh_amd as tb
    verts = [star(n) for n in TLAS_BLAS]
    inst = tb.make_instances(tlas_transforms(), list(TLAS_INST_BLAS))
    bounds = np.array([np.concatenate([v[:, :3].min(0), v[:, :3].max(0)]) for v in verts], F)
    h = ctypes.c_void_p()
    tb.check(tb.lib.tbvh_host_build_tlas(_p(inst), inst.shape[0], _p(bounds), len(verts), ctypes.byref(h)), "tbvh_host_build_tlas")
    tb.lib.tbvh_host_free(h)
    return inst, verts


def tlas_rays():
    """per instance: the aimed rays of its BLAS from the first eye, eye and targets taken through the instance's transform (fp32), so every one starts inside a
    closed mesh and must hit it; then TLAS_RANDOM random directions from those three eyes"""
    T = tlas_transforms()
    out = []
    eyes_w = []
    for k, b in enumerate(TLAS_INST_BLAS):
        N = TLAS_BLAS[b]
        r = aimed_rays(N)[:36 * N * N]                      # the first eye's
        P0 = r["O"]; P1 = (r["O"] + r["D"] * F(0.5)).astype(F)
        M = T[k]
        W0 = (P0 @ M[:3, :3].T + M[:3, 3]).astype(F); W1 = (P1 @ M[:3, :3].T + M[:3, 3]).astype(F)
        out.append(make_rays(W0, W1 - W0))
        eyes_w.append(W0[0])
    rng = np.random.default_rng(321)
    E = np.array(eyes_w, F)
    out.append(make_rays(E[rng.integers(0, 3, TLAS_RANDOM)], rng.normal(size=(TLAS_RANDOM, 3)).astype(F)))
    return np.concatenate(out)


def hit_fields_inst(r):
    """(n, 5) uint32: t, u, v bits, prim, and the instance (0 where the ray hit nothing)"""
    hit = r["t"] < BVH_FAR
    return np.ascontiguousarray(np.concatenate([hit_fields(r), np.where(hit, r["inst"], 0).astype(np.uint32)[:, None]], 1))


def make_tlas_golden(refs, out_dir=GOLDEN):
    inst, verts = tlas_instances()
    rays = tlas_rays()
    wt, occ = refs["wt"].brute_tlas(verts, inst["invTransform"], inst["blasIdx"], rays)
    mt, _ = refs["mt"].brute_tlas(verts, inst["invTransform"], inst["blasIdx"], rays)
    n_aimed = rays.shape[0] - TLAS_RANDOM
    assert misses(wt[:n_aimed]) == 0, ("the uncontracted watertight brute force leaks through the instances", misses(wt[:n_aimed]))
    assert misses(mt[:n_aimed]) > 0
    np.savez_compressed(os.path.join(out_dir, "tlas.npz"), n_aimed=np.int64(n_aimed), ray_sum=np.uint64(rays.view(np.uint32).astype(np.uint64).sum()),
                        inst_sum=np.uint64(np.ascontiguousarray(inst["invTransform"]).view(np.uint32).astype(np.uint64).sum()), wt=hit_fields_inst(wt), wt_occ=np.packbits(occ),
                        mt_misses=np.int64(misses(mt[:n_aimed])))


def tlas_fixture_inputs():
    g = golden("tlas")
    inst, verts = tlas_instances()
    rays = tlas_rays()
    assert int(rays.view(np.uint32).astype(np.uint64).sum()) == int(g["ray_sum"]) and \
        int(np.ascontiguousarray(inst["invTransform"]).view(np.uint32).astype(np.uint64).sum()) == int(g["inst_sum"]), "the generators no longer make the golden's inputs"
    return inst, verts, rays, g


# ---- goldens -------------------------------------------------------------------------------------------------------------------------------------------
GOLDEN_N = (4, 12)
DISPLACE = 0.08


def misses(records):
    return int((records["t"] >= BVH_FAR).sum())


def golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def hit_fields(r):
    """a record array's hit part as (n, 4) uint32: t, u, v bits and prim"""
    return np.ascontiguousarray(np.stack([r["t"].view(np.uint32), r["u"].view(np.uint32), r["v"].view(np.uint32), r["prim"]], 1))


def make_golden(refs, out_dir=GOLDEN):
    """Per mesh: the vertices are regenerated by the tests (star is deterministic; the file keeps a checksum), the rays likewise; stored are the watertight
    brute-force records and occlusion flags (bit-packed), the four miss counts on the aimed rays, and for the unmoved meshes the records of Moeller-Trumbore's
    brute force and of the reference's own BVH::Intersect under either test (the tests compare records with the watertight brute force only).  The watertight brute force must
    miss NOTHING on the aimed sets: that is the condition the fixtures have to meet."""
    os.makedirs(out_dir, exist_ok=True)
    for N in GOLDEN_N:
        for tag, disp in (("", 0.0), ("_moved", DISPLACE)):
            if tag and N != 12:
                continue
            verts = star(N, displace=disp)
            rays = np.concatenate([aimed_rays(N, displace=disp), random_rays(100 + N)])
            n_aimed = rays.shape[0] - N_RANDOM
            wt, wt_occ = refs["wt"].brute(verts, rays)
            mt, mt_occ = refs["mt"].brute(verts, rays)
            wt_bvh, _ = refs["wt"].bvh(verts, rays)
            mt_bvh, _ = refs["mt"].bvh(verts, rays)
            fma, _ = refs["wt_fma"].brute(verts, rays)
            counts = (misses(mt_bvh[:n_aimed]), misses(mt[:n_aimed]), misses(wt_bvh[:n_aimed]), misses(wt[:n_aimed]))
            assert counts[3] == 0, ("the uncontracted watertight brute force leaks", N, tag, counts)
            assert counts[1] > 0 and counts[0] >= counts[1], ("the aimed set has no teeth: Moeller-Trumbore loses none of it", N, tag, counts)
            save = dict(n_aimed=np.int64(n_aimed), vert_sum=np.uint64(verts.view(np.uint32).astype(np.uint64).sum()),
                        ray_sum=np.uint64(rays.view(np.uint32).astype(np.uint64).sum()), wt=hit_fields(wt), wt_occ=np.packbits(wt_occ), counts=np.array(counts, np.int64), fma_misses=np.int64(misses(fma[:n_aimed])))
            if not tag:   # for whoever asks later WHICH rays each test and each traversal loses: Moeller-Trumbore's brute force, and the reference's own BVH::Intersect under either test
                save.update(mt=hit_fields(mt), mt_bvh=hit_fields(mt_bvh), wt_bvh=hit_fields(wt_bvh))
            if N == 4 and not tag:
                m = checker_map(verts.shape[0] // 3, 4)
                omm, omm_occ = refs["wt"].brute(verts, rays, m, 4)
                save.update(omm=hit_fields(omm), omm_occ=np.packbits(omm_occ))
            np.savez_compressed(os.path.join(out_dir, f"star{N}{tag}.npz"), **save)


def fixture_inputs(N, moved=False):
    """(verts, rays, golden) with the checksums verified: the generators still make what the golden was recorded over"""
    g = golden(f"star{N}" + ("_moved" if moved else ""))
    verts = star(N, displace=DISPLACE if moved else 0.0)
    rays = np.concatenate([aimed_rays(N, displace=DISPLACE if moved else 0.0), random_rays(100 + N)])
    assert int(verts.view(np.uint32).astype(np.uint64).sum()) == int(g["vert_sum"]) and int(rays.view(np.uint32).astype(np.uint64).sum()) == int(g["ray_sum"]), \
        "the generators no longer make the golden's inputs"
    return verts, rays, g
