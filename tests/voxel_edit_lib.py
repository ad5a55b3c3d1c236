"""Shared pieces of the voxel editing tests: the real reference behind tests/voxel_edit_ref_shim.cpp (compiled per session into a pytest temp
dir), the Set cases, the rays of the normals tests and the goldens under tests/golden/voxeledit (tools/make_voxel_edit_golden.py)."""
import ctypes as C
import os

import numpy as np

import native_build as nb
import tinybvh_amd as tb
from native_build import _p, _u32, _u64, _vp
from voxel_lib import GRID_WORDS, BRICK_WORDS, TOP_WORDS, dense_to_xyzv, scene_dense

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_EDIT = os.path.join(HERE, "golden", "voxeledit")


class RefVoxelEdit:
    """The real reference's VoxelSet::Set / UpdateTopGrid / GetNormal (voxel_edit_ref_shim.cpp)."""

    def __init__(self, so):
        self.lib = C.CDLL(so)
        L = self.lib
        L.vedit_new.restype = _vp
        L.vedit_free.argtypes = [_vp]
        L.vedit_set.argtypes = [_vp, _vp, _u64]
        L.vedit_update_top_grid.argtypes = [_vp]
        L.vedit_arrays.argtypes = [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]
        L.vedit_arrays.restype = _u32
        L.vedit_normals.argtypes = [_vp, _vp, _u32, _u64, _vp]

    def run(self, batches, top=True):
        """(grid, bricks[:used], top) after Set on every record of every batch in turn, then UpdateTopGrid"""
        h = self.lib.vedit_new()
        try:
            for b in batches:
                b = np.ascontiguousarray(b, np.uint32).reshape(-1, 4)
                self.lib.vedit_set(h, _p(b), b.shape[0])
            if top:
                self.lib.vedit_update_top_grid(h)
            g, b, t = _vp(), _vp(), _vp()
            used = self.lib.vedit_arrays(h, C.byref(g), C.byref(b), C.byref(t))
            grid = np.ctypeslib.as_array((C.c_uint32 * GRID_WORDS).from_address(g.value)).copy()
            bricks = np.ctypeslib.as_array((C.c_uint32 * (used * BRICK_WORDS)).from_address(b.value)).copy()
            topg = np.ctypeslib.as_array((C.c_uint32 * TOP_WORDS).from_address(t.value)).copy() if top else np.zeros(TOP_WORDS, np.uint32)
            return grid, bricks, topg
        finally:
            self.lib.vedit_free(h)

    def normals(self, rays):
        rays = np.ascontiguousarray(rays)
        out = np.zeros((rays.shape[0], 4), np.float32)
        h = self.lib.vedit_new()
        try:
            self.lib.vedit_normals(h, _p(rays), rays.dtype.itemsize, rays.shape[0], _p(out))
        finally:
            self.lib.vedit_free(h)
        return out


def compile_edit_ref_shim(d):
    """the reference with oracle/Makefile's flags plus -DNDEBUG; None when the reference is absent"""
    so = nb.compile_ref_shim(d, "voxel_edit_ref_shim.cpp", defines=("NDEBUG",))
    return so and RefVoxelEdit(so)


edit_ref = nb.ref_fixture("voxel_edit_ref", compile_edit_ref_shim)


def host_twin(batches, top=True):
    """(grid, bricks[:used], top) of the library's CPU twin after the same calls"""
    h = tb.HostVoxelEdit()
    for b in batches:
        h.Set(b)
    if top:
        h.UpdateTopGrid()
    return h.arrays()


def same_arrays(got, want, what):
    for name, a, b in zip(("grid", "bricks", "top"), got, want):
        assert a.size == b.size, f"{what}: {name}: {a.size} words, want {b.size}"
        bad = np.nonzero(a != b)[0]
        assert bad.size == 0, f"{what}: {name}: {bad.size} words differ, first at {bad[:4].tolist()}: got {a[bad[:4]]} want {b[bad[:4]]}"


# ---- Set cases: name -> list of batches, each an (n, 4) uint32 array of {x, y, z, v} -----------------------------------------------------
def _recs(rows):
    return np.ascontiguousarray(np.asarray(rows, np.uint32).reshape(-1, 4))


_LEGOCAR = {}


def legocar_records():
    if "r" not in _LEGOCAR:
        _LEGOCAR["r"] = dense_to_xyzv(scene_dense("legocar"))
    return _LEGOCAR["r"]


def set_case(name):
    rng = np.random.default_rng(sum(name.encode()))
    if name == "one_record":
        return [_recs([[200, 3, 77, 0xDEADBEEF]])]
    if name == "one_voxel_1000":
        r = np.zeros((1000, 4), np.uint32)
        r[:, 0], r[:, 1], r[:, 2] = 17, 250, 9
        r[:, 3] = rng.integers(0, 1 << 32, 1000, dtype=np.uint64).astype(np.uint32)
        return [r]
    if name == "brick_reverse":
        i = np.arange(511, -1, -1, dtype=np.uint32)
        return [_recs(np.stack([40 + (i & 7), 96 + ((i >> 3) & 7), 8 + (i >> 6), i + 1], 1))]
    if name == "bricks_65_out_of_order":
        cells = rng.permutation(32768)[:65].astype(np.uint32)      # not cell order; each touched three times, interleaved
        order = np.concatenate([cells, cells[::-1], rng.permutation(cells)])
        off = rng.integers(0, 8, (order.size, 3)).astype(np.uint32)
        xyz = np.stack([(order & 31) * 8, ((order >> 5) & 31) * 8, (order >> 10) * 8], 1).astype(np.uint32) + off
        return [_recs(np.concatenate([xyz, rng.integers(1, 1 << 32, (order.size, 1), dtype=np.uint64).astype(np.uint32)], 1))]
    if name == "mixed_new_existing_zero":
        first = _recs(np.concatenate([rng.integers(0, 64, (300, 3)), rng.integers(1, 1 << 32, (300, 1), dtype=np.uint64)], 1).astype(np.uint32))
        xyz = np.concatenate([first[rng.integers(0, 300, 200), :3], rng.integers(0, 256, (200, 3)).astype(np.uint32)])   # existing voxels and new bricks
        v = rng.integers(1, 1 << 32, 400, dtype=np.uint64).astype(np.uint32)
        v[rng.random(400) < 0.3] = 0                               # v = 0 is written like any value, and allocates
        second = np.concatenate([xyz, v[:, None]], 1)[rng.permutation(400)]
        return [first, _recs(second)]
    if name == "two_batches":
        a = rng.integers(0, 256, (500, 4)).astype(np.uint32); b = rng.integers(0, 256, (500, 4)).astype(np.uint32)
        b[:100, :3] = a[:100, :3]
        return [_recs(a), _recs(b)]
    if name == "legocar_100k":
        r = rng.integers(0, 256, (100000, 4)).astype(np.uint32)
        r[:, 3] = rng.integers(0, 1 << 32, 100000, dtype=np.uint64).astype(np.uint32)
        r[50000:, :3] = r[rng.integers(0, 50000, 50000), :3]       # duplicates
        r[::7, :3] = legocar_records()[rng.integers(0, legocar_records().shape[0], r[::7].shape[0]), :3]   # voxels the car holds
        return [legocar_records(), _recs(r)]
    raise KeyError(name)


SET_CASES = ["one_record", "one_voxel_1000", "brick_reverse", "bricks_65_out_of_order", "mixed_new_existing_zero", "two_batches", "legocar_100k"]


# ---- rays of the normals tests --------------------------------------------------------------------------------------------------------
def normal_rays(n, seed):
    """hit records whose point O + t D lies in cells, on cell planes and edges of all three levels (exactly: dyadic O, D and t), with zero,
    negative-zero and negative direction components, and misses (t = 1e30)"""
    rng = np.random.default_rng(seed)
    k = n // 4
    O = rng.random((n, 3), dtype=np.float32)
    D = rng.normal(size=(n, 3)).astype(np.float32)
    t = rng.uniform(0, 1.5, n).astype(np.float32)
    # exact points on planes / edges / corners: O on a 1/1024 grid, D small integers over a power of two, t a multiple of 1/256
    res = rng.choice([8, 32, 256, 1024], (k, 1)).astype(np.float32)
    O[:k] = np.floor(rng.random((k, 3), dtype=np.float32) * res) / res
    D[:k] = rng.integers(-4, 5, (k, 3)).astype(np.float32) / np.float32(4)
    t[:k] = rng.integers(0, 64, k).astype(np.float32) / np.float32(256)
    # a plane in one axis, an edge in two, anything in the third
    O[k:2 * k] = rng.random((k, 3), dtype=np.float32)
    ax = rng.integers(0, 3, k); ax2 = (ax + rng.integers(1, 3, k)) % 3
    res = rng.choice([8, 32, 256], k).astype(np.float32)
    j = np.arange(k)
    O[k + j, ax] = np.floor(O[k + j, ax] * res) / res
    edge = rng.random(k) < 0.5
    O[k + j[edge], ax2[edge]] = np.floor(O[k + j[edge], ax2[edge]] * res[edge]) / res[edge]
    t[k:2 * k] = 0
    # zero, negative-zero and negative components
    z = rng.integers(0, 4, (k, 3))
    Dz = D[2 * k:3 * k].copy()
    Dz[z == 0] = np.float32(0.0); Dz[z == 1] = np.float32(-0.0); Dz[z == 2] = -np.abs(Dz[z == 2])
    D[2 * k:3 * k] = Dz
    rays = tb.make_rays(O, D, tmax=t)
    rays["D"] = D                                                  # as drawn: GetNormal does not ask for a unit vector
    miss = rng.random(n) < 0.1
    rays["t"][miss] = np.float32(1e30)
    rays["prim"] = rng.integers(1, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    return rays


def exact_instances(n, seed):
    """instances whose transforms are exact in fp32 whatever the contraction: a signed axis permutation (a rotation by quarter turns, or its
    mirror image), power-of-two scales, translations on a 1/8 grid"""
    rng = np.random.default_rng(seed)
    T = np.zeros((n, 4, 4), np.float32)
    for i in range(n):
        P = np.eye(3)[rng.permutation(3)] * rng.choice([-1.0, 1.0], 3)[:, None]
        T[i, :3, :3] = P * rng.choice([0.5, 1.0, 2.0, 4.0], 3)[None, :]
        T[i, :3, 3] = rng.integers(-32, 33, 3) / 8.0
        T[i, 3, 3] = 1
    inst = tb.make_instances(T, np.zeros(n, np.uint32))
    inst["invTransform"] = np.linalg.inv(T.astype(np.float64)).astype(np.float32).reshape(n, 16)   # exact: every entry is dyadic
    return inst


def exact_world_rays(rays, inst, seed):
    """object-space hit records taken into world space through instance hit.inst, exactly: O, D on coarse dyadic grids so that every product and
    sum of the transform and of its inverse is exact"""
    rng = np.random.default_rng(seed)
    n = rays.shape[0]
    out = rays.copy()
    which = rng.integers(0, inst.shape[0], n).astype(np.uint32)
    O = np.floor(rays["O"] * np.float32(1024)) / np.float32(1024)
    D = np.round(rays["D"] * np.float32(16)) / np.float32(16)
    t = np.floor(rays["t"] * np.float32(64)) / np.float32(64)
    M = inst["transform"].reshape(-1, 4, 4)[which].astype(np.float32)
    out["O"] = np.einsum("nij,nj->ni", M[:, :3, :3], O) + M[:, :3, 3]
    out["D"] = np.einsum("nij,nj->ni", M[:, :3, :3], D)
    out["t"] = np.where(rays["t"] < np.float32(1e30), t, rays["t"])
    out["inst"] = which
    obj = rays.copy()
    obj["O"], obj["D"], obj["t"] = O, D, out["t"]
    return out, obj


# ---- voxelising a traced scene: the goldens' scene, and the reference's loop (voxel_edit_ref_shim.cpp) finished with the CPU shading twin --------
VOXELIZE_CASES = ["table", "colour", "tlas", "ugly"]
VOXELIZE_MAX_HITS = 64
VOXELIZE_COLOUR = 0x00C08040


def _quad(p0, p1, p2, p3):
    return [p0, p1, p2, p0, p2, p3]


def voxelize_scene():
    """(verts (3 n, 4) float32, FatTri records, materials, textures): a closed box (12 triangles), three tilted interior quads and one quad with an
    alpha-cut texture, coordinates within +-10.  An axis ray crosses at most 2 box faces and 4 quads."""
    lo, hi = np.array([-6.3, -5.1, -4.7]), np.array([7.9, 6.2, 5.3])
    c = [np.array([hi[0] if i & 1 else lo[0], hi[1] if i & 2 else lo[1], hi[2] if i & 4 else lo[2]]) for i in range(8)]
    tris, mat, uv = [], [], []
    for q in ((0, 2, 6, 4), (1, 5, 7, 3), (0, 4, 5, 1), (2, 3, 7, 6), (0, 1, 3, 2), (4, 6, 7, 5)):
        tris += _quad(*[c[k] for k in q]); mat += [0, 0]; uv += [[(0, 0), (1, 0), (1, 1)], [(0, 0), (1, 1), (0, 1)]]
    quads = [((-5.2, -4.1, -3.3), (6.1, -3.7, -2.2), (5.7, 5.0, 1.9), (-4.9, 4.4, 0.6)),
             ((-3.9, -4.6, 3.8), (-2.7, 5.3, 4.4), (4.8, 4.9, -3.1), (3.5, -4.2, -3.9)),
             ((-5.6, 1.2, -4.1), (6.9, 2.3, -3.6), (6.2, 0.4, 4.7), (-5.1, -0.9, 4.2))]
    for k, q in enumerate(quads):
        tris += _quad(*[np.array(p) for p in q]); mat += [1 + k, 1 + k]; uv += [[(0, 0), (1, 0), (1, 1)], [(0, 0), (1, 1), (0, 1)]]
    leaf = ((-4.4, -2.9, 2.6), (5.3, -3.4, 3.1), (5.8, 3.9, 2.2), (-4.0, 4.6, 1.4))
    tris += _quad(*[np.array(p) for p in leaf]); mat += [4, 4]; uv += [[(0.1, 0.2), (3.1, 0.2), (3.1, 3.2)], [(0.1, 0.2), (3.1, 3.2), (0.1, 3.2)]]
    verts = np.zeros((len(tris), 4), np.float32)
    verts[:, :3] = np.array(tris, np.float32)
    fat = np.zeros(len(mat), tb.FATTRI_DTYPE)
    fat["material"] = mat
    for k in range(3):
        fat["u%d" % k] = [t[k][0] for t in uv]; fat["v%d" % k] = [t[k][1] for t in uv]
    for k in range(3):
        fat["vertex%d" % k] = verts[k::3, :3]
    mats = np.zeros(5, tb.MATERIAL_DTYPE)
    mats["color"] = [(0.8, 0.7, 0.6), (0.9, 0.1, 0.2), (0.15, 0.85, 0.3), (0.2, 0.3, 0.95), (1, 1, 1)]
    mats["color_texture"] = [tb.NO_TEXTURE] * 4 + [0]
    mats["normal_texture"] = tb.NO_TEXTURE
    rng = np.random.default_rng(61)
    tex = rng.integers(0, 1 << 24, (32, 32), dtype=np.uint64).astype(np.uint32)
    yy, xx = np.mgrid[0:32, 0:32]
    alpha = np.where(((xx // 4 + yy // 4) & 1) == 0, 255, rng.integers(0, 3, (32, 32))).astype(np.uint32)   # cut: alpha 0, 1 or 2
    tex |= alpha << 24
    return verts, fat, mats, [tex]


def voxelize_instances():
    """the scene twice: as it is, and halved, turned a quarter about z and lifted — both within +-10"""
    T = np.tile(np.eye(4, dtype=np.float32), (2, 1, 1))
    T[1, :3, :3] = np.array([[0, -0.5, 0], [0.5, 0, 0], [0, 0, 0.5]], np.float32)
    T[1, :3, 3] = (1.25, -0.75, 6.5)
    return tb.make_instances(T, np.zeros(2, np.uint32))


def voxelize_params(case, bounds6):
    """(bmin, maxSize, ext): dyadic ones for which the ray origins are exact whatever is contracted, or the demo's cube of the scene's bounds"""
    if case in ("table", "colour"):
        return np.full(3, -8.5, np.float32), np.float32(17.0), np.array([16, 16, 16], np.float32)
    return tb.voxelize_bounds(bounds6)


def reference_voxelize(ref, case):
    """the reference's loop over the case's scene: dict of the set's arrays after it, the records made, the most hits a ray had and the rays with
    more than two"""
    verts, fat, mats, texs = voxelize_scene()
    L = ref.lib
    L.vscene_blas.restype = _vp; L.vscene_blas.argtypes = [_vp, _u32]
    L.vscene_tlas.restype = _vp; L.vscene_tlas.argtypes = [_vp, _u32, _vp, _u32]
    L.vscene_free.argtypes = [_vp]; L.vscene_bounds.argtypes = [_vp, _vp]
    L.vedit_voxelize_hits.restype = _u64
    L.vedit_voxelize_hits.argtypes = [_vp, _vp, C.c_float, _vp, _u32, _u64, _vp, _vp, _vp]
    blas = L.vscene_blas(_p(verts), verts.shape[0] // 3)
    inst, scene = None, blas
    if case == "tlas":
        inst = voxelize_instances()
        arr = (C.c_void_p * 1)(blas)
        scene = L.vscene_tlas(_p(inst), inst.shape[0], C.cast(arr, _vp), 1)
    try:
        b6 = np.zeros(6, np.float32)
        L.vscene_bounds(scene, _p(b6))
        bmin, max_size, ext = voxelize_params(case, b6)
        bmin = np.ascontiguousarray(bmin, np.float32); ext = np.ascontiguousarray(ext, np.float32)
        per_ray = np.zeros(3 * 65536, np.uint32)
        n = L.vedit_voxelize_hits(scene, _p(bmin), float(max_size), _p(ext), 100000, 0, None, None, _p(per_ray))
        rays = np.zeros(n, tb.RAY_DTYPE); meta = np.zeros((n, 4), np.uint32)
        assert L.vedit_voxelize_hits(scene, _p(bmin), float(max_size), _p(ext), 100000, n, _p(rays), _p(meta), _p(per_ray)) == n
    finally:
        if scene != blas:
            L.vscene_free(scene)
        L.vscene_free(blas)
    a, x, y = meta[:, 0].astype(np.int64), meta[:, 1], meta[:, 2]
    P = np.zeros((n, 3), np.int64)
    idx = np.arange(n)
    P[idx, (a + 1) % 3] = x; P[idx, (a + 2) % 3] = y; P[idx, a] = meta[:, 3].view(np.int32)
    P = np.clip(P, 0, 255).astype(np.uint32)
    if case == "colour":
        v = np.full(n, VOXELIZE_COLOUR, np.uint32); keep = np.ones(n, bool)
    else:
        sh = tb.host_shade_hits(mats, texs, [fat], rays, inst)
        rgb = (sh.albedo * np.float32(255)).astype(np.int32).astype(np.int64)        # (int)( albedo * 255 ): one fp32 product, truncated
        v = ((rgb[:, 0] << 16) + (rgb[:, 1] << 8) + rgb[:, 2]).astype(np.uint32)
        keep = sh.alpha != 0
    recs = np.ascontiguousarray(np.concatenate([P, v[:, None]], 1)[keep])
    grid, bricks, top = ref.run([recs])
    return {"grid": grid, "bricks": bricks, "top": top, "records": np.uint64(recs.shape[0]), "max_hits": np.uint32(per_ray.max()),
            "rays_over_2": np.uint64((per_ray > 2).sum()), "hits": np.uint64(n),
            "bmin": bmin, "max_size": np.float32(max_size), "ext": ext}
