"""Shared by the viewer tests (test_viewer_host.py, test_viewer_gpu.py): NumPy and the compilers only.  The plain-C restatement of the reference's two CPU
viewers with libm's atan2f / acosf (tests/oracle_viewer.c), the real SampleSky of tiny_bvh_gltf.cpp behind tests/viewer_ref_shim.cpp (compiled per session
into a pytest temp dir when the reference checkout is present), and the SKY_EDGE margin (DESIGN.md par. 22) from the measurement in profiles/viewer.txt."""
import ctypes as C
import os
import re

import numpy as np

import native_build as nb
from native_build import _p, _u32, _u64, _vp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SKY_EDGE_U, SKY_EDGE_V, SKY_CLAMPED_Y, SKY_NAN = 1, 2, 4, 8
_f64 = C.c_double


def measured_ulps():
    """(vw_atan2f, vw_acosf): the largest errors tools/viewer_math_error.c found, as profiles/viewer.txt records them"""
    with open(os.path.join(ROOT, "profiles", "viewer.txt")) as f:
        text = f.read()
    a = re.search(r"vw_atan2f\s+max ([0-9.]+) ulp", text)
    c = re.search(r"vw_acosf\s+max ([0-9.]+) ulp", text)
    return float(a.group(1)), float(c.group(1))


def margins():
    """The margin, in ulps of the texel coordinate, within which this library's sky and a libm sky may read different texels (DESIGN.md par. 22): the
    measured error of the library's function, glibc's 1 ulp, the three roundings of the product chain (the sum p + 2 pi, the product with the width, the
    fused multiply-add), and for atan2 one more because its sweep is not exhaustive."""
    atan2_ulp, acos_ulp = measured_ulps()
    return atan2_ulp + 1 + 3 + 1, acos_ulp + 1 + 3


class Restatement:
    def __init__(self, so):
        self.lib = C.CDLL(so)
        for name in ("ovw_generate", "ovw_sky", "ovw_continue", "ovw_shadow_rays", "ovw_light", "ovw_pack"):
            getattr(self.lib, name).restype = None
        self.lib.ovw_generate.argtypes = [_vp, _vp, _vp, _vp, _u32, _u32, _u64, _u64, _vp]
        self.lib.ovw_sky.argtypes = [_vp, _u32, _u32, _vp, _u64, _f64, _vp, _vp, _vp, _vp]
        self.lib.ovw_continue.argtypes = [_vp, _u32, _u32, _vp, _u32, _vp, _u64, _vp]
        self.lib.ovw_shadow_rays.argtypes = [_vp, _u32, _u64, _vp, _vp]
        self.lib.ovw_light.argtypes = [_u32, _vp, _u32, _u32, _vp, _u32, _vp, _vp, _u64, _vp, _f64, _vp, _vp]
        self.lib.ovw_pack.argtypes = [_vp, _u64, _vp]

    def generate(self, cam, first=0, n=None):
        n = cam.width * cam.height - first if n is None else n
        rays = np.zeros((n, 16), np.float32)
        v = [np.array(list(getattr(cam, k)), np.float32) for k in ("eye", "p1", "p2", "p3")]
        self.lib.ovw_generate(_p(v[0]), _p(v[1]), _p(v[2]), _p(v[3]), cam.width, cam.height, first, n, _p(rays))
        return rays

    def sky(self, pixels, dirs, margin_ulps):
        """(out (n, 4) float32, flags, ku, kv): margin_ulps = (u, v) margins; the flags of both calls are merged"""
        p = np.ascontiguousarray(pixels, np.float32)
        d = np.zeros((np.asarray(dirs).shape[0], 4), np.float32); d[:, :3] = np.asarray(dirs, np.float32)[:, :3]
        n = d.shape[0]
        out = np.zeros((n, 4), np.float32); ku = np.zeros(n, np.int64); kv = np.zeros(n, np.int64)
        fu = np.zeros(n, np.uint32); fv = np.zeros(n, np.uint32)
        self.lib.ovw_sky(_p(p), p.shape[1], p.shape[0], _p(d), n, margin_ulps[0], _p(out), _p(fu), _p(ku), _p(kv))
        self.lib.ovw_sky(_p(p), p.shape[1], p.shape[0], _p(d), n, margin_ulps[1], _p(out), _p(fv), _p(ku), _p(kv))
        flags = (fu & ~np.uint32(SKY_EDGE_V)) | (fv & np.uint32(SKY_EDGE_V))
        return out, flags, ku, kv

    def continue_(self, materials, n_textures, rays, out48):
        r = np.array(rays).view(np.float32).reshape(rays.shape[0], -1)
        m = np.ascontiguousarray(materials).view(np.uint32).reshape(-1, 5)
        o = np.ascontiguousarray(out48, np.float32).reshape(-1, 12)
        went = np.zeros(r.shape[0], np.uint8)
        self.lib.ovw_continue(_p(m), m.shape[0], n_textures, _p(r), r.shape[1], _p(o), r.shape[0], _p(went))
        return r, went.astype(bool)

    def shadow_rays(self, rays, L):
        r = np.ascontiguousarray(rays).view(np.float32).reshape(rays.shape[0], -1)
        l = np.ascontiguousarray(L, np.float32)
        out = np.zeros((r.shape[0], 16), np.float32)
        self.lib.ovw_shadow_rays(_p(r), r.shape[1], r.shape[0], _p(l), _p(out))
        return out

    def light(self, mode, pixels, rays, out48, occ, L, margin_ulps):
        """(rgb (n, 4), edge flags of every sky sample the record took)"""
        r = np.ascontiguousarray(rays).view(np.float32).reshape(rays.shape[0], -1)
        o = np.ascontiguousarray(out48, np.float32).reshape(-1, 12)
        l = np.ascontiguousarray(L, np.float32)
        p = None if pixels is None else np.ascontiguousarray(pixels, np.float32)
        oc = None if occ is None else np.ascontiguousarray(occ, np.uint8)
        n = r.shape[0]
        rgb = np.zeros((n, 4), np.float32)
        edge = np.zeros(n, np.uint32); e2 = np.zeros(n, np.uint32)
        args = (mode, None if p is None else _p(p), 0 if p is None else p.shape[1], 0 if p is None else p.shape[0], _p(r), r.shape[1], _p(o), None if oc is None else _p(oc), n, _p(l))
        self.lib.ovw_light(*args, margin_ulps[0], _p(rgb), _p(edge))
        self.lib.ovw_light(*args, margin_ulps[1], _p(rgb), _p(e2))
        return rgb, (edge & ~np.uint32(SKY_EDGE_V)) | (e2 & np.uint32(SKY_EDGE_V))

    def pack(self, rgb):
        c = np.ascontiguousarray(rgb, np.float32).reshape(-1, 4)
        out = np.zeros(c.shape[0], np.uint32)
        self.lib.ovw_pack(_p(c), c.shape[0], _p(out))
        return out


GOLDEN = os.path.join(HERE, "golden", "viewer")
GOLDEN_STEP = 131            # the per-ray sets of the goldens: every 131st pixel of the 800 x 600 frame


def golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def cpu_frame(trace, occluded, sc, fat, inst, cam, mode, sky, max_rounds=8):
    """A viewer frame through the library's host twins, with the caller's traversal for every Intersect (trace( rays ) -> traced copy) and IsOccluded
    (occluded( rays ) -> bytes): host generate -> { trace, tbvh_host_shade_hits, tbvh_host_viewer_continue } x rounds -> host shadow rays -> host light ->
    host pack.  fat: the FatTri arrays per BLAS slot; inst: the instance records, or None for a single BLAS.  Returns a dict: pix, rgb, rays (final),
    out (final shading records), occ, per_round (rays traced per round), history (per round: pixel indices, their records after the trace)."""
    import tinybvh_amd as tb
    rays = tb._aligned(trace(tb.host_viewer_generate(cam)))
    n = rays.shape[0]
    out = np.array(tb.host_shade_hits(sc.materials, sc.textures, fat, rays, inst))
    per_round, history = [n], [(np.arange(n), rays.copy())]
    if mode == tb.VIEWER_GLTF:
        live = np.arange(n)
        for _ in range(1, max_rounds):
            sub = tb._aligned(rays[live].copy())
            went = tb.host_viewer_continue(sc.materials, sc.n_textures, sub, out[live])
            if not went.any():
                break
            live = live[went]
            sub = tb._aligned(trace(np.ascontiguousarray(sub[went])))
            rays[live] = sub
            out[live] = np.array(tb.host_shade_hits(sc.materials, sc.textures, fat, sub, inst))
            per_round.append(int(live.size))
            history.append((live.copy(), sub.copy()))
    occ = None
    if mode == tb.VIEWER_FOLIAGE:
        occ = np.asarray(occluded(tb.host_viewer_shadow_rays(rays)), np.uint8)
    rgb = tb.host_viewer_light(mode, sky, rays, out, occ)
    return dict(pix=tb.host_viewer_pack(rgb), rgb=rgb, rays=rays, out=out, occ=occ, per_round=per_round, history=history)


def reference_tracers(reference, verts, inst, kind):
    """(trace, occluded) through oracle/_ref, the real tiny_bvh.h built by the recipe under oracle/: BVH::Build per BLAS and, for "tlas", BVH::Build over the
    instances + IntersectTLAS (oracle_lib.RefTlas); "blas": BVH::Intersect / IsOccluded of the one BLAS.  oracle/_ref has no IsOccluded for a TLAS: a shadow
    ray is occluded exactly when Intersect finds a hit below its tmax (both accept t < hit.t of the same triangle test), so that is what is asked.  The objects
    are kept alive by the closures."""
    from oracle_lib import RefTlas
    scenes = [reference.build(v) for v in verts]
    if kind == "blas":
        return (lambda r: scenes[0].intersect(1, r)), (lambda r: scenes[0].occluded(1, r))
    tlas = RefTlas(reference, inst, scenes)

    def occluded(r):
        return (tlas.intersect(r)["t"] < r["t"]).astype(np.uint8)
    return tlas.intersect, occluded


def same_through_the_rounds(a, b, n):
    """per pixel: the records of two frames' histories (cpu_frame's, or a staged device frame's) are bit-equal in every round, and the pixel is traced in the
    same rounds by both"""
    ok = np.ones(n, bool)
    for r in range(max(len(a), len(b))):
        if r >= len(a) or r >= len(b):
            ok[(a if r < len(a) else b)[r][0]] = False
            continue
        (ia, ra), (ib, rb) = a[r], b[r]
        ma, mb = np.zeros(n, bool), np.zeros(n, bool)
        ma[ia] = True; mb[ib] = True
        ok[ma != mb] = False
        fa, fb = np.zeros((n, 16), np.uint32), np.zeros((n, 16), np.uint32)
        fa[ia] = np.ascontiguousarray(ra).view(np.uint32).reshape(-1, 16); fb[ib] = np.ascontiguousarray(rb).view(np.uint32).reshape(-1, 16)
        ok[(fa != fb).any(1)] = False
    return ok


def compile_oracle(d):
    return Restatement(nb.compile_c_oracle(d, "oracle_viewer"))


# ---- the real reference ---------------------------------------------------------------------------------------------------------------------------
REF_FILES = ("tiny_bvh.h", "tiny_scene.h", "tiny_bvh_gltf.cpp", "tiny_bvh_foliage.cpp")   # what the shim needs of the reference checkout


class RealReference:
    """tests/viewer_ref_shim.cpp: the viewer file's own SampleSky, Trace and WorkerThread, and Scene::tlas's Intersect / IsOccluded, over a scene handed in once
    (scene(): the arrays are kept alive here)"""

    def __init__(self, so):
        self.lib = C.CDLL(so)
        for name in ("vref_scene", "vref_release", "vref_intersect", "vref_occluded", "vref_trace", "vref_sky", "vref_frame"):
            getattr(self.lib, name).restype = None
        self.lib.vref_scene.argtypes = [_vp, _u32, _vp, _vp, _vp, _u32, _vp, _u32, _vp, _vp, _vp, _u32, _vp, _u32, _u32]
        self.lib.vref_intersect.argtypes = [_vp, _u32]
        self.lib.vref_occluded.argtypes = [_vp, _u32, _vp]
        self.lib.vref_trace.argtypes = [_vp, _u32, _vp]
        self.lib.vref_sky.argtypes = [_vp, _u32, _u32, _vp, _u32, _vp]
        self.lib.vref_frame.argtypes = [_vp, _vp, _vp, _vp, _vp]
        self.keep = None

    def scene(self, instances, verts, fat_tris, materials, textures, sky):
        assert self.keep is None, "one scene per shim"
        inst = np.ascontiguousarray(instances)
        v = [np.ascontiguousarray(x, np.float32) for x in verts]
        f = [np.ascontiguousarray(x) for x in fat_tris]
        counts = np.array([x.shape[0] // 3 for x in v], np.uint32)
        assert all(fi.size == c for fi, c in zip(f, counts))
        mats = np.ascontiguousarray(materials).view(np.uint32).reshape(-1, 5)
        tex = [np.ascontiguousarray(t, np.uint32) for t in textures]
        widths = np.array([t.shape[1] for t in tex], np.uint32); heights = np.array([t.shape[0] for t in tex], np.uint32)
        vp = (C.c_void_p * len(v))(*[x.ctypes.data for x in v])
        fp = (C.c_void_p * len(f))(*[x.ctypes.data for x in f])
        tp = (C.c_void_p * len(tex))(*[t.ctypes.data for t in tex])
        sk = None if sky is None else np.ascontiguousarray(sky, np.float32)
        self.keep = (inst, v, f, mats, tex, sk)
        self.lib.vref_scene(_p(inst), inst.nbytes // 192, vp, fp, _p(counts), len(v), _p(mats), mats.shape[0], tp, _p(widths), _p(heights), len(tex),
                            None if sk is None else _p(sk), 0 if sk is None else sk.shape[1], 0 if sk is None else sk.shape[0])
        return self

    def release(self):
        if self.keep is not None:
            self.lib.vref_release()
            self.keep = None

    def intersect(self, rays):
        r = np.array(rays)
        self.lib.vref_intersect(_p(r), r.shape[0])
        return r

    def occluded(self, rays):
        r = np.ascontiguousarray(rays)
        out = np.zeros(r.shape[0], np.uint8)
        self.lib.vref_occluded(_p(r), r.shape[0], _p(out))
        return out

    def trace(self, rays):
        """(rgb (n, 3), the records as Trace leaves them)"""
        r = np.array(rays)
        rgb = np.zeros((r.shape[0], 3), np.float32)
        self.lib.vref_trace(_p(r), r.shape[0], _p(rgb))
        return rgb, r

    def sky(self, pixels, dirs):
        p = np.ascontiguousarray(pixels, np.float32)
        d = np.ascontiguousarray(np.asarray(dirs, np.float32)[:, :3])
        out = np.zeros((d.shape[0], 3), np.float32)
        self.lib.vref_sky(_p(p), p.shape[1], p.shape[0], _p(d), d.shape[0], _p(out))
        return out

    def frame(self, cam):
        """WorkerThread's 800 x 600 buf for this view pyramid"""
        v = [np.array(list(getattr(cam, k)), np.float32) for k in ("eye", "p1", "p2", "p3")]
        buf = np.zeros((600, 800), np.uint32)
        self.lib.vref_frame(_p(v[0]), _p(v[1]), _p(v[2]), _p(v[3]), _p(buf))
        return buf


def compile_ref_shim(d, foliage=False):
    """The real viewer file (tiny_bvh_gltf.cpp, or tiny_bvh_foliage.cpp) with oracle/Makefile's flags; None when the reference is absent"""
    so = nb.compile_ref_shim(d, "viewer_ref_shim.cpp", out="viewer_ref_foliage" if foliage else None, defines=("VIEWER_REF_FOLIAGE",) if foliage else (),
                             scene_header=True, need=REF_FILES)
    return so and RealReference(so)
