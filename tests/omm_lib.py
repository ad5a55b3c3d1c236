"""Shared by the opacity-micromap bake tests (test_omm_host.py, test_omm_gpu.py), tools/make_omm_golden.py and tools/omm_bake_bench.py (so: NumPy and the
compilers only, no GPU library): deterministic alpha textures and UV meshes, the
plain-C restatement of CreateOpacityMicroMap (tests/oracle_omm.c), the real reference behind tests/omm_ref_shim.cpp (compiled per session into a pytest temp
dir when the reference checkout is present), the two session fixtures over them, and the goldens under tests/golden/omm (DESIGN.md par. 15)."""
import ctypes as C
import os

import numpy as np

import native_build as nb
from native_build import _p, _u32

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "omm")
GOLDEN_N = (4, 32)
GOLDEN_TRIS = 301
NO_TEXTURE = 0xFFFFFFFF
ALPHAS = np.array([0, 1, 2, 3, 128, 255], np.uint32)   # the reference's test is alpha > 2: hit from both sides
ALL_N = (1, 2, 4, 8, 32, 64)


def words_per_tri(N):
    return (N * N + 31) // 32


# ---- the restatement and the real reference ------------------------------------------------------------------------------------------------
class _BakeFns:
    """bake(uv (3 n, 2) flat corners, tri_texture (n,), textures [(h, w) uint32], N): (n, words) uint32"""

    def __init__(self, so, prefix):
        self.lib = L = C.CDLL(so)
        self._bake = getattr(L, prefix + "_bake")
        self._bake.restype = None
        if prefix == "oorc":
            L.oorc_clamped.restype = _u32

    @staticmethod
    def _args(uv, tri_texture, textures):
        uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 6)
        tt = np.ascontiguousarray(tri_texture, np.uint32).reshape(-1)
        tex = [np.ascontiguousarray(t, np.uint32) for t in textures]
        assert uv.shape[0] == tt.size and all(t.ndim == 2 for t in tex)
        assert all(int(k) == NO_TEXTURE or int(k) < len(tex) for k in np.unique(tt))
        ptrs = (C.c_void_p * max(len(tex), 1))(*[t.ctypes.data for t in tex])
        widths = np.array([t.shape[1] for t in tex] or [0], np.uint32)
        heights = np.array([t.shape[0] for t in tex] or [0], np.uint32)
        return uv, tt, tex, ptrs, widths, heights

    def bake(self, uv, tri_texture, textures, N):
        uv, tt, tex, ptrs, widths, heights = self._args(uv, tri_texture, textures)
        out = np.full((uv.shape[0], words_per_tri(N)), 0xA5A5A5A5, np.uint32)
        self._bake(_p(uv), _u32(uv.shape[0]), _p(tt), ptrs, _p(widths), _p(heights), _u32(len(tex)), C.c_int(N), _p(out))
        return out

    def clamped(self, uv, tri_texture, textures, N):
        """how many samples take the clamp to the last texel column / row (restatement only)"""
        uv, tt, tex, ptrs, widths, heights = self._args(uv, tri_texture, textures)
        return int(self.lib.oorc_clamped(_p(uv), _u32(uv.shape[0]), _p(tt), _p(widths), _p(heights), C.c_int(N)))


def compile_oracle(d):
    return _BakeFns(nb.compile_c_oracle(d, "oracle_omm"), "oorc")


def compile_ref_shim(d):
    """The real CreateOpacityMicroMap with oracle/Makefile's flags; None when the reference is absent"""
    so = nb.compile_ref_shim(d, "omm_ref_shim.cpp", scene_header=True, need=("tiny_bvh.h", "tiny_scene.h"))
    return so and _BakeFns(so, "oref")


omm_oracle = nb.oracle_fixture("oracle_omm", compile_oracle)
omm_ref = nb.ref_fixture("omm_ref", compile_ref_shim)


# ---- generators ----------------------------------------------------------------------------------------------------------------------------
ALPHA_P = (0.2, 0.2, 0.2, 0.1, 0.15, 0.15)   # 40 % of the blobs opaque: a bit is the OR of its samples, so maps come out fuller than the texture


def texture(w, h, seed, blobs=5):
    """(h, w) uint32 texels: alpha drawn from ALPHAS per blob — about `blobs` blobs across each side, several texels wide —, random colour bits below"""
    rng = np.random.default_rng(seed)
    cw, ch = max(1, w // blobs), max(1, h // blobs)
    a = rng.choice(ALPHAS, size=(-(-h // ch), -(-w // cw)), p=ALPHA_P)
    a = np.repeat(np.repeat(a, ch, 0), cw, 1)[:h, :w]
    rgb = rng.integers(0, 1 << 24, (h, w)).astype(np.uint32)
    return np.ascontiguousarray((a.astype(np.uint32) << 24) | rgb)


def textures():
    """the two textures of the test meshes: 64 x 64, and 37 x 19 (neither square nor a power of two)"""
    return [texture(64, 64, 11), texture(37, 19, 12)]


SPECIALS = {   # triangle -> its three corners (the slots are ones that keep a texture, see mesh())
    0: [(0, 0), (1, 0), (0, 1)],                                   # corners exactly on integers
    1: [(-1, 2), (2, -1), (3, 3)],
    3: [(0.3, 0.7), (0.3, 0.7), (0.3, 0.7)],                       # degenerate: all corners equal
    4: [(-1e-9, 0.5), (-1e-9, 0.25), (-1e-9, 0.75)],               # a tiny negative u: the fraction rounds to 1.0, the clamp to w - 1 is taken
    6: [(3 / 64, 5 / 64), (17 / 64, 5 / 64), (3 / 64, 40 / 64)],   # on texel boundaries k / w of the 64 x 64 texture (triangle 6 uses texture 0)
    7: [(-37.3, -20.1), (41.9, 3.3), (2.2, 55.5)],                 # many texture repeats
    9: [(5 / 37, 2 / 19), (30 / 37, 2 / 19), (5 / 37, 17 / 19)],   # on texel boundaries of the 37 x 19 texture (triangle 9 uses texture 1)
    10: [(0.5, -1e-9), (0.25, -1e-9), (0.75, -1e-9)],              # the clamp in v
}


def mesh(n_tris=GOLDEN_TRIS, seed=5):
    """(uv (3 n, 2) float32: corners of triangle i at 3i .. 3i + 2; tri_texture (n,) uint32).  Every third triangle (i % 3 == 2) has no texture, the others
    alternate between textures 0 and 1.  Every twelfth triangle has its corners anywhere in [-2, 3]^2 (many repeats: at a small N every bit of it sees an opaque
    texel), every twelfth is about a texel wide (inside one blob: a fully clear or fully set map), the others are a blob or two wide around a centre in
    [-2, 3]^2 (wrap, negatives; mixed maps); SPECIALS overwrite the first few."""
    rng = np.random.default_rng(seed)
    uv = np.zeros((n_tris, 3, 2), np.float32)
    for i in range(n_tris):
        if i % 12 == 0:
            uv[i] = rng.uniform(-2, 3, (3, 2))
        else:
            ext = 0.008 if i % 12 == 4 else (0.2, 0.3, 0.25)[i % 3]
            uv[i] = rng.uniform(-2, 3, (1, 2)) + rng.uniform(-ext, ext, (3, 2))
    for i, c in SPECIALS.items():
        if i < n_tris:
            uv[i] = np.array(c, np.float32)
    tt = np.where(np.arange(n_tris) % 3 == 2, NO_TEXTURE, (np.arange(n_tris) // 3) % 2).astype(np.uint32)
    return np.ascontiguousarray(uv.reshape(-1, 2)), tt


def indexed(uv_flat):
    """the same triangles over shared UVs: (uv (n_uv, 2), indices (n, 3))"""
    u, inv = np.unique(uv_flat, axis=0, return_inverse=True)
    return np.ascontiguousarray(u, np.float32), np.ascontiguousarray(inv.reshape(-1, 3).astype(np.uint32))


def leaf_texture(size=1024):
    """a procedural leaf: opaque inside a pointed oval with a serrated edge, a few holes, transparent outside (tools/omm_bake_bench.py, the end-to-end test)"""
    y, x = np.mgrid[0:size, 0:size].astype(np.float32) / np.float32(size)
    cx, cy = x - 0.5, y - 0.5
    half = 0.42 * np.sin(np.pi * np.clip(y, 0, 1)) ** 0.8 * (1 + 0.08 * np.sin(40 * y))
    inside = (np.abs(cx) < half) & (np.abs(cy) < 0.48)
    holes = ((cx - 0.1) ** 2 + (cy + 0.15) ** 2 < 0.003) | ((cx + 0.12) ** 2 + (cy - 0.1) ** 2 < 0.002)
    a = np.where(inside & ~holes, 255, 0).astype(np.uint32)
    return np.ascontiguousarray((a << 24) | np.uint32(0x2E8B57))


def map_stats(words, tri_texture, N):
    """over the TEXTURED triangles: (share of their N * N bits that are set, share of them that are mixed, how many fully clear, how many fully set)"""
    w = np.ascontiguousarray(words, np.uint32)[np.asarray(tri_texture) != NO_TEXTURE]
    bits = np.unpackbits(w.view(np.uint8), axis=1, bitorder="little")[:, :N * N].sum(1)
    clear, full = int((bits == 0).sum()), int((bits == N * N).sum())
    return float(bits.sum()) / (w.shape[0] * N * N), 1.0 - (clear + full) / w.shape[0], clear, full


def check_not_vacuous(words, tri_texture, N):
    share, mixed, clear, full = map_stats(words, tri_texture, N)
    assert 0.2 <= share <= 0.8 and mixed >= 0.5 and clear >= 1 and full >= 1, (N, share, mixed, clear, full)


# ---- goldens -------------------------------------------------------------------------------------------------------------------------------
def golden(N):
    return np.load(os.path.join(GOLDEN, f"mixed_n{N}.npz"))


def make_golden(ref, out_dir=GOLDEN):
    """Inputs and the REAL reference's words (ref: compile_ref_shim's), one file per N of GOLDEN_N: the flat UVs, the shared UVs and indices of the same mesh,
    the per-triangle texture indices, the two textures, N, and `words`.  The reference alone must meet the cap against a vacuous golden."""
    os.makedirs(out_dir, exist_ok=True)
    uv, tt = mesh()
    tex = textures()
    uvi, idx = indexed(uv)
    for N in GOLDEN_N:
        words = ref.bake(uv, tt, tex, N)
        check_not_vacuous(words, tt, N)
        np.savez_compressed(os.path.join(out_dir, f"mixed_n{N}.npz"), uv=uv, uv_shared=uvi, indices=idx, tri_texture=tt, tex0=tex[0], tex1=tex[1],
                            N=np.int32(N), words=words)
