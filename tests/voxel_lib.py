"""Shared pieces of the VoxelSet tests: the restatement (tests/oracle_voxel.c) and the real reference behind tests/voxel_ref_shim.cpp, both
compiled per session into a pytest temp dir, the fixtures' scenes and the seeded ray sets."""
import ctypes as C
import os

import numpy as np

import native_build as nb
import tinybvh_amd as tb
from native_build import _i, _p, _u32, _u64, _vp

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "voxels")
GRID_WORDS, BRICK_WORDS, TOP_WORDS = 32 * 32 * 32, 512, 16


def dense_to_xyzv(dense):
    """the set voxels of dense[z, y, x] as {x, y, z, v} records in the order of tiny_bvh_voxel.cpp's loop (x outermost, z innermost)"""
    v = np.ascontiguousarray(dense, np.uint32).transpose(2, 1, 0)
    x, y, z = np.nonzero(v)
    return np.ascontiguousarray(np.stack([x, y, z, v[x, y, z]], 1).astype(np.uint32))


class VoxelOracle:
    """oracle_voxel.c: Set / UpdateTopGrid and the traversals; rule 0 = the reference verbatim, rule 1 = the library's acceptance."""

    def __init__(self, so):
        self.lib = C.CDLL(so)
        L = self.lib
        L.vx_set_voxels.argtypes = [_vp, _vp, _u32, _vp, _vp, _u64]
        L.vx_update_top_grid.argtypes = [_vp, _vp]
        L.vx_intersect.argtypes = [_vp, _vp, _vp, _vp, _u64, _i]
        L.vx_occluded.argtypes = [_vp, _vp, _vp, _vp, _u64, _vp]
        L.vx_intersect_tlas.argtypes = [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _u32, _vp, _u64, _i]
        L.vx_occluded_tlas.argtypes = [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _u32, _vp, _u64, _i, _vp]

    def build(self, dense):
        """(grid, bricks[:used], top) of a set filled in the reference demo's order"""
        recs = dense_to_xyzv(dense)
        cap = 2 + recs.shape[0]
        grid = np.zeros(GRID_WORDS, np.uint32)
        bricks = np.zeros(min(cap, GRID_WORDS + 1) * BRICK_WORDS, np.uint32)
        used = C.c_uint32(1)
        assert self.lib.vx_set_voxels(_p(grid), _p(bricks), min(cap, GRID_WORDS + 1), C.byref(used), _p(recs), recs.shape[0]) == 0
        top = np.zeros(TOP_WORDS, np.uint32)
        self.lib.vx_update_top_grid(_p(grid), _p(top))
        return grid, bricks[: used.value * BRICK_WORDS].copy(), top

    def intersect(self, s, rays, rule):
        out = np.ascontiguousarray(rays).copy()
        self.lib.vx_intersect(_p(s[0]), _p(s[1]), _p(s[2]), _p(out), out.shape[0], rule)
        return out

    def occluded(self, s, rays):
        rays = np.ascontiguousarray(rays)
        out = np.zeros(rays.shape[0], np.uint8)
        self.lib.vx_occluded(_p(s[0]), _p(s[1]), _p(s[2]), _p(rays), rays.shape[0], _p(out))
        return out

    def _sets(self, sets):
        arrs = [(C.c_void_p * len(sets))(*[s[k].ctypes.data for s in sets]) for k in range(3)]
        return [C.cast(a, _vp) for a in arrs], arrs

    def intersect_tlas(self, nodes32, idx, inst, sets, rays, rule):
        """nodes32 / idx: the Wald-format TLAS (rule 0 only; rule 1 visits every instance)"""
        (g, b, t), keep = self._sets(sets)
        nodes32 = np.zeros(8, np.uint32) if nodes32 is None else np.ascontiguousarray(nodes32)
        idx = np.zeros(1, np.uint32) if idx is None else np.ascontiguousarray(idx, np.uint32)
        inst = np.ascontiguousarray(inst)
        out = np.ascontiguousarray(rays).copy()
        self.lib.vx_intersect_tlas(_p(nodes32), _p(idx), _p(inst), inst.shape[0], g, b, t, len(sets), _p(out), out.shape[0], rule)
        return out

    def occluded_tlas(self, nodes32, idx, inst, sets, rays, rule):
        (g, b, t), keep = self._sets(sets)
        nodes32 = np.zeros(8, np.uint32) if nodes32 is None else np.ascontiguousarray(nodes32)
        idx = np.zeros(1, np.uint32) if idx is None else np.ascontiguousarray(idx, np.uint32)
        inst = np.ascontiguousarray(inst)
        rays = np.ascontiguousarray(rays)
        out = np.zeros(rays.shape[0], np.uint8)
        self.lib.vx_occluded_tlas(_p(nodes32), _p(idx), _p(inst), inst.shape[0], g, b, t, len(sets), _p(rays), rays.shape[0], rule, _p(out))
        return out


class RefVoxels:
    """The real reference (voxel_ref_shim.cpp)."""

    def __init__(self, so):
        self.lib = C.CDLL(so)
        L = self.lib
        L.vref_new.restype = _vp
        L.vref_free.argtypes = [_vp]
        L.vref_set.argtypes = [_vp, _vp, _u64]
        L.vref_update_top_grid.argtypes = [_vp]
        L.vref_arrays.argtypes = [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]
        L.vref_arrays.restype = _u32
        L.vref_intersect.argtypes = [_vp, _vp, _u64]
        L.vref_occluded.argtypes = [_vp, _vp, _u64, _vp]
        L.vref_tlas_build.argtypes = [_vp, _u32, _vp, _u32]
        L.vref_tlas_build.restype = _vp
        L.vref_tlas_free.argtypes = [_vp]
        L.vref_tlas_blob.argtypes = [_vp, _i, C.POINTER(_vp)]
        L.vref_tlas_blob.restype = _u64
        L.vref_tlas_intersect.argtypes = [_vp, _vp, _u64]
        L.vref_tlas_occluded.argtypes = [_vp, _vp, _u64, _vp]

    def new_set(self, dense):
        h = self.lib.vref_new()
        recs = dense_to_xyzv(dense)
        self.lib.vref_set(h, _p(recs), recs.shape[0])
        self.lib.vref_update_top_grid(h)
        return h

    def arrays(self, h):
        g, b, t = _vp(), _vp(), _vp()
        used = self.lib.vref_arrays(h, C.byref(g), C.byref(b), C.byref(t))
        grid = np.ctypeslib.as_array((C.c_uint32 * GRID_WORDS).from_address(g.value)).copy()
        bricks = np.ctypeslib.as_array((C.c_uint32 * (used * BRICK_WORDS)).from_address(b.value)).copy()
        top = np.ctypeslib.as_array((C.c_uint32 * TOP_WORDS).from_address(t.value)).copy()
        return grid, bricks, top

    def intersect(self, h, rays):
        out = np.ascontiguousarray(rays).copy()
        self.lib.vref_intersect(h, _p(out), out.shape[0])
        return out

    def occluded(self, h, rays):
        rays = np.ascontiguousarray(rays)
        out = np.zeros(rays.shape[0], np.uint8)
        self.lib.vref_occluded(h, _p(rays), rays.shape[0], _p(out))
        return out

    def tlas(self, inst, set_handles):
        """BVH::Build over the instances (updated in place); returns (handle, BVH_GPU nodes (n, 16) u32, idx, Wald nodes (n, 8) u32)"""
        arr = (C.c_void_p * len(set_handles))(*set_handles)
        h = self.lib.vref_tlas_build(_p(inst), inst.shape[0], C.cast(arr, _vp), len(set_handles))
        blobs = []
        for which, width in ((0, 16), (1, 1), (2, 8)):
            p = _vp()
            n = self.lib.vref_tlas_blob(h, which, C.byref(p))
            blobs.append(np.ctypeslib.as_array((C.c_uint32 * (n * width)).from_address(p.value)).reshape(n, width).copy())
        return h, blobs[0], blobs[1].reshape(-1), blobs[2]

    def tlas_intersect(self, h, rays):
        out = np.ascontiguousarray(rays).copy()
        self.lib.vref_tlas_intersect(h, _p(out), out.shape[0])
        return out

    def tlas_occluded(self, h, rays):
        rays = np.ascontiguousarray(rays)
        out = np.zeros(rays.shape[0], np.uint8)
        self.lib.vref_tlas_occluded(h, _p(rays), rays.shape[0], _p(out))
        return out


def compile_oracle(d):
    return VoxelOracle(nb.compile_c_oracle(d, "oracle_voxel"))


def compile_ref_shim(d):
    """the reference with oracle/Makefile's flags plus -DNDEBUG; None when the reference is absent"""
    so = nb.compile_ref_shim(d, "voxel_ref_shim.cpp", defines=("NDEBUG",))
    return so and RefVoxels(so)


vox_oracle = nb.oracle_fixture("oracle_voxel", compile_oracle)
vox_ref = nb.ref_fixture("voxel_ref", compile_ref_shim)


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
def load_fixture(name):
    """a dense (z, y, x) uint32 array from a voxel file of the reference's format (tb.load_voxel_file)"""
    return tb.load_voxel_file(os.path.join(GOLDEN, name + ".bin"))


def scene_dense(name, seed=0):
    """dense (z, y, x) arrays of the test scenes, within 256^3"""
    rng = np.random.default_rng(seed)
    if name in ("legocar", "rock"):
        return load_fixture(name)
    if name == "sparse":
        d = np.zeros((256, 256, 256), np.uint32)
        n = 20000
        z, y, x = rng.integers(0, 256, n), rng.integers(0, 256, n), rng.integers(0, 256, n)
        d[z, y, x] = rng.integers(1, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        return d
    if name == "block64":
        d = np.zeros((96, 96, 96), np.uint32)
        d[16:80, 16:80, 16:80] = (np.arange(64 ** 3, dtype=np.uint32) + 1).reshape(64, 64, 64)
        return d
    if name == "terrain":
        xs = np.arange(256, dtype=np.float32)
        h = (96 + 40 * np.sin(xs[None, :] * 0.05) * np.cos(xs[:, None] * 0.037) + 20 * np.sin((xs[None, :] + xs[:, None]) * 0.11)).astype(np.int32)
        zz = np.arange(256)[:, None, None]
        d = np.where(np.arange(256)[None, :, None] < h[:, None, :], (zz * 65536 + h[:, None, :] + 1).astype(np.uint32), np.uint32(0))
        return np.ascontiguousarray(d.astype(np.uint32))   # (z, y, x): height along y
    raise KeyError(name)


# ---- rays -----------------------------------------------------------------------------------------------------------------------------
def voxel_rays(n, seed, dense=None, lo=(0.0, 0.0, 0.0), hi=(1.0, 1.0, 1.0)):
    """a seeded mix over the box [lo, hi]: rays from outside at the box, rays starting inside (also inside filled voxels when `dense`
    is given), origins on cell planes of all three levels, axis-parallel rays with +-0 components, grazing rays along the faces, and a
    quarter with a finite tmax"""
    rng = np.random.default_rng(seed)
    lo = np.asarray(lo, np.float32); hi = np.asarray(hi, np.float32)
    ext = hi - lo
    k = n // 8
    O = np.zeros((n, 3), np.float32); D = np.zeros((n, 3), np.float32)
    # 1: from a sphere around the box towards a point in it
    c = (lo + hi) * 0.5
    u = rng.normal(size=(n, 3)).astype(np.float32); u /= np.linalg.norm(u, axis=1, keepdims=True)
    O[:] = c + u * np.float32(1.2) * ext.max()
    D[:] = lo + rng.random((n, 3), dtype=np.float32) * ext - O
    # 2: inside the box, random directions
    O[k:2 * k] = lo + rng.random((k, 3), dtype=np.float32) * ext
    D[k:2 * k] = rng.normal(size=(k, 3))
    # 3: inside filled voxels
    if dense is not None:
        zz, yy, xx = np.nonzero(dense)
        pick = rng.integers(0, xx.size, k)
        vox = np.stack([xx[pick], yy[pick], zz[pick]], 1).astype(np.float32) + rng.random((k, 3), dtype=np.float32)
        O[2 * k:3 * k] = lo + vox / np.float32(256) * ext
        D[2 * k:3 * k] = rng.normal(size=(k, 3))
    # 4: origins on cell planes (1/8, 1/32, 1/256) inside and just outside
    res = rng.choice([8, 32, 256], size=(k, 1)).astype(np.float32)
    O[3 * k:4 * k] = lo + np.floor(rng.uniform(-0.25, 1.25, (k, 3)).astype(np.float32) * res) / res * ext
    D[3 * k:4 * k] = rng.normal(size=(k, 3))
    # 5: axis-parallel and +-0 components
    Dp = rng.normal(size=(k, 3)).astype(np.float32)
    for j in range(k):
        m = rng.integers(1, 7)
        for a in range(3):
            if m >> a & 1:
                Dp[j, a] = np.float32(-0.0) if rng.random() < 0.5 else np.float32(0.0)
    O[4 * k:5 * k] = lo + rng.uniform(-0.5, 1.5, (k, 3)).astype(np.float32) * ext
    D[4 * k:5 * k] = Dp
    # 6: grazing: on a face of the box, direction within that face (or nearly)
    Og = lo + rng.random((k, 3), dtype=np.float32) * ext
    Dg = rng.normal(size=(k, 3)).astype(np.float32)
    ax = rng.integers(0, 3, k)
    side = rng.integers(0, 2, k)
    for j in range(k):
        Og[j, ax[j]] = lo[ax[j]] if side[j] == 0 else hi[ax[j]]
        Dg[j, ax[j]] = rng.choice([0.0, -0.0, 1e-7, -1e-7]) if rng.random() < 0.8 else Dg[j, ax[j]] * np.float32(1e-3)
    O[5 * k:6 * k] = Og; D[5 * k:6 * k] = Dg
    # 7: edges / corners: through cell edges exactly (diagonal directions)
    O[6 * k:7 * k] = lo + np.floor(rng.random((k, 3), dtype=np.float32) * 32) / np.float32(32) * ext
    D[6 * k:7 * k] = rng.choice([-1.0, 1.0], size=(k, 3)) * rng.choice([1.0, 0.5, 2.0], size=(k, 1))
    tmax = np.full(n, np.float32(1e30))
    fin = rng.random(n) < 0.25
    tmax[fin] = rng.uniform(0.0, 2.0, fin.sum()).astype(np.float32) * ext.max()
    rays = tb.make_rays(O, D, tmax=tmax)
    rays["instIdx"] = rng.integers(0, 1 << 20, n).astype(np.uint32)
    rays["mask"] = rng.choice([0xFFFF, 0x1, 0x2, 0xFF00], n).astype(np.uint32)
    return rays


def hit_bytes(rays):
    """the 20 hit bytes of every record (inst, t, u, v, prim) as (n, 5) uint32"""
    return np.ascontiguousarray(rays).view(np.uint32).reshape(-1, 16)[:, 11:16].copy()
