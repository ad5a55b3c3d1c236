"""The scene and the hit records of the shading tests (test_shade_host.py, test_shade_gpu.py, tools/make_shade_golden.py): the smallest at which the kernel can
still go wrong.  Two BLAS slots (the committed bunny cut, every 16th triangle; a two-triangle quad), five instances (identity; rotated with a non-uniform
scale; mirrored; translated only; one over the quad), four materials (untextured; a 7 x 3 colour texture with texels of alpha 0, 2 and 3; colour 5 x 4 plus a
3 x 6 normal map; a normal map only), one FatTri with a zero geometric normal and one with zero vertex normals.  Everything is made from seeds; nothing
here needs a GPU."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import native_build as nb
import shade_lib as _L
import tinybvh_amd as tb
from custom_lib import bunny_verts
from shade_lib import FATTRI_DTYPE, MATERIAL_DTYPE, NO_TEXTURE, REF_OUT_OF_BOUNDS, TU_INTEGER, WRAPPED

BUNNY_STEP = 16
N_SYNTHETIC = 4096 + 37          # the last wave is partial
CAMERA_SIDE = 64
# the special triangles of slot 0 (all textured)
TRI_INTEGER_UV, TRI_WRAP_U, TRI_WRAP_V, TRI_WRAP_U_LAST_ROW, TRI_ZERO_N, TRI_ZERO_VN = 5, 6, 7, 8, 9, 10
TINY = np.float32(-1e-9)


def _unit(v):
    l = np.sqrt((v * v).sum(-1, keepdims=True))
    return (v / np.where(l == 0, 1, l)).astype(np.float32)


def textures():
    rng = np.random.default_rng(21)
    shapes = [(3, 7), (4, 5), (6, 3), (5, 2)]     # (h, w): colour 7 x 3, colour 5 x 4, normal map 3 x 6, normal map 2 x 5
    out = []
    for h, w in shapes:
        rgb = rng.integers(0, 1 << 24, (h, w)).astype(np.uint32)
        a = rng.choice(np.array([0, 2, 3, 255], np.uint32), size=(h, w))
        out.append(np.ascontiguousarray((a << 24) | rgb))
    out[0].reshape(-1)[:3] = (out[0].reshape(-1)[:3] & 0xFFFFFF) | (np.array([0, 2, 3], np.uint32) << 24)
    return out


def materials():
    m = np.zeros(4, MATERIAL_DTYPE)
    m["color"] = [(0.8, 0.5, 0.25), (0.1, 0.2, 0.3), (0.9, 0.9, 0.1), (0.33, 0.66, 0.99)]
    m["color_texture"] = [NO_TEXTURE, 0, 1, NO_TEXTURE]
    m["normal_texture"] = [NO_TEXTURE, NO_TEXTURE, 2, 3]
    return m


def fat_tris(verts, seed):
    """FatTri records for a (3 n, 4) triangle soup: vertices and the geometric normal from the soup, vertex normals the geometric normal bent a little,
    random UVs in [-2, 3], T and B a random frame, every field the shading does not read filled with a pattern (it must come back untouched)."""
    rng = np.random.default_rng(seed)
    t = verts.reshape(-1, 3, 4)[:, :, :3]
    n = t.shape[0]
    f = np.zeros(n, FATTRI_DTYPE)
    f.view(np.uint32).reshape(n, 48)[:] = (0x7F000000 + np.arange(n * 48, dtype=np.uint32).reshape(n, 48) % 0xFFFF)
    N = _unit(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]))
    f["Nx"], f["Ny"], f["Nz"] = N[:, 0], N[:, 1], N[:, 2]
    for k in range(3):
        f[f"vertex{k}"] = t[:, k]
        f[f"vN{k}"] = _unit(N + rng.normal(0, 0.2, (n, 3)).astype(np.float32))
        f[f"u{k}"] = rng.uniform(-2, 3, n).astype(np.float32)
        f[f"v{k}"] = rng.uniform(-2, 3, n).astype(np.float32)
    f["T"] = _unit(rng.normal(size=(n, 3)).astype(np.float32))
    f["B"] = _unit(rng.normal(size=(n, 3)).astype(np.float32))
    f["material"] = rng.integers(0, 4, n).astype(np.uint32)
    f["ltriIdx"] = -1
    return f


class ShadeScene:
    """verts[s], fat[s]: the two BLAS slots; instances: INSTANCE_DTYPE with transform and blasIdx set (the bounds and the inverse are filled when a TLAS is
    built over them); materials, textures."""

    def __init__(self):
        bunny = np.ascontiguousarray(bunny_verts().reshape(-1, 3, 4)[::BUNNY_STEP].reshape(-1, 4))
        quad = np.array([[-1, -1, 0, 0], [1, -1, 0, 0], [1, 1, 0, 0], [-1, -1, 0, 0], [1, 1, 0, 0], [-1, 1, 0, 0]], np.float32)
        self.verts = [bunny, quad]
        self.materials, self.textures = materials(), textures()
        f0, f1 = fat_tris(bunny, 31), fat_tris(quad, 32)
        # the quad: UVs its corners, material 1 (the 7 x 3 texture)
        uvq = (quad[:, :2] * 0.5 + 0.5).reshape(2, 3, 2)
        for k in range(3):
            f1[f"u{k}"], f1[f"v{k}"] = uvq[:, k, 0], uvq[:, k, 1]
        f1["material"] = 1
        f0["material"][[TRI_INTEGER_UV, TRI_WRAP_U, TRI_WRAP_V, TRI_WRAP_U_LAST_ROW]] = [2, 1, 1, 2]
        for k, (u, v) in enumerate([(1.0, -2.0), (2.0, 3.0), (3.0, 0.0)]):                        # corners on integers: tu an exact integer at the corners
            f0[f"u{k}"][TRI_INTEGER_UV], f0[f"v{k}"][TRI_INTEGER_UV] = u, v
        for k in range(3):
            f0[f"u{k}"][TRI_WRAP_U], f0[f"v{k}"][TRI_WRAP_U] = TINY, 0.5                          # tu wraps to 1.0, a middle row: the next row's first texel
            f0[f"u{k}"][TRI_WRAP_V], f0[f"v{k}"][TRI_WRAP_V] = 0.4, TINY                          # tv wraps to 1.0: row `height`, outside the texture
            f0[f"u{k}"][TRI_WRAP_U_LAST_ROW], f0[f"v{k}"][TRI_WRAP_U_LAST_ROW] = TINY, 0.99       # tu wraps in the last row: texel width * height
        f0["Nx"][TRI_ZERO_N] = f0["Ny"][TRI_ZERO_N] = f0["Nz"][TRI_ZERO_N] = 0
        for k in range(3):
            f0[f"vN{k}"][TRI_ZERO_VN] = 0
        f0["material"][[TRI_ZERO_N, TRI_ZERO_VN]] = [0, 1]                                        # (no normal map: the zero vector stays zero)
        self.fat = [f0, f1]
        lo, hi = bunny[:, :3].min(0), bunny[:, :3].max(0)
        ext = float((hi - lo).max())
        a, b = 0.7, 0.4
        rot = (np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]) @ np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]]))
        T = np.tile(np.eye(4), (5, 1, 1))
        T[1, :3, :3] = rot @ np.diag([0.6, 1.3, 0.9]); T[1, :3, 3] = [1.3 * ext, 0, 0]
        T[2, :3, :3] = np.diag([-1.0, 1.0, 1.0]); T[2, :3, 3] = [0, 1.3 * ext, 0]
        T[3, :3, 3] = [1.3 * ext, 1.3 * ext, 0.1 * ext]
        T[4, :3, :3] = np.diag([0.25 * ext] * 3); T[4, :3, 3] = [0.65 * ext + float(lo[0] + hi[0]) / 2, 0.65 * ext + float(lo[1] + hi[1]) / 2, float(hi[2]) + 0.2 * ext]
        self.instances = tb.make_instances(T.astype(np.float32), [0, 0, 0, 0, 1])
        self.slot_of_inst = np.array([0, 0, 0, 0, 1])
        c = np.array([0.65 * ext + (lo[0] + hi[0]) / 2, 0.65 * ext + (lo[1] + hi[1]) / 2, (lo[2] + hi[2]) / 2], np.float32)
        self.centre, self.extent = c, ext

    def camera_rays(self):
        """64 x 64 rays from a pinhole in front of the scene (+z side), a little wider than the scene: misses included"""
        s = CAMERA_SIDE
        eye = self.centre + np.array([0.1, 0.2, 4.0], np.float32) * self.extent
        g = (np.arange(s, dtype=np.float32) + 0.5) / s - 0.5
        gx, gy = np.meshgrid(g, g)
        target = self.centre + np.stack([gx.ravel() * 2.7 * self.extent, gy.ravel() * 2.7 * self.extent, np.zeros(s * s, np.float32)], 1)
        return tb.make_rays(np.tile(eye, (s * s, 1)), target - eye)

    def host_bvhs(self):
        return [tb.HostBVH(v, tb.LAYOUT_CWBVH) for v in self.verts]

    def synthetic_records(self):
        """4096 + 37 hit records with inst, prim, u, v and D set directly: random ones, then the classes the tests want present, written over the first ones"""
        rng = np.random.default_rng(77)
        n = N_SYNTHETIC
        r = tb.make_rays(rng.normal(size=(n, 3)).astype(np.float32), rng.normal(size=(n, 3)).astype(np.float32))
        inst = rng.integers(0, 5, n)
        r["inst"] = inst
        r["prim"] = [rng.integers(0, self.fat[self.slot_of_inst[i]].size) for i in inst]
        u = rng.random(n, dtype=np.float32); v = rng.random(n, dtype=np.float32)
        flip = u + v > 1
        u[flip], v[flip] = 1 - u[flip], 1 - v[flip]
        r["u"], r["v"], r["t"] = u, v, rng.uniform(0.5, 20, n).astype(np.float32)
        k = 0

        def put(inst_, prim, u_, v_):
            nonlocal k
            r["inst"][k], r["prim"][k], r["u"][k], r["v"][k] = inst_, prim, u_, v_
            k += 1
        for i in range(4):                                    # every bunny instance: the special triangles
            put(i, 0, 0.0, 0.0)                               # u = v = 0
            put(i, 1, 0.25, 0.75)                             # u + v = 1
            put(i, 2, 1.0, 0.0)
            for c in ((0.0, 0.0), (1.0, 0.0), (0.0, 1.0)):
                put(i, TRI_INTEGER_UV, *c)
            for tri in (TRI_WRAP_U, TRI_WRAP_V, TRI_WRAP_U_LAST_ROW, TRI_ZERO_N, TRI_ZERO_VN):
                put(i, tri, 0.3, 0.3)
        put(4, 0, 0.0, 0.0); put(4, 1, 0.5, 0.5)
        r[k:k + 200] = r[k + 200:k + 400]                     # D on both sides of the surface: 200 records twice, the second time with -D
        r["D"][k:k + 200] = -r["D"][k + 200:k + 400]
        self.n_special, self.pairs = k, (slice(k, k + 200), slice(k + 200, k + 400))
        r["t"][-3:] = 1e30                                    # and three misses at the end (the partial wave)
        return r

    @staticmethod
    def stride128(r):
        wide = np.zeros((r.shape[0], 128), np.uint8)
        wide[:, :64] = r.view(np.uint8).reshape(-1, 64)
        wide[:, 64:] = 0xCD
        return wide


@functools.lru_cache(maxsize=1)
def scene():
    return ShadeScene()


def host_tlas(instances, verts):
    """the library's host TLAS over the instances (their bounds and inverses are filled in place): (bvh2 nodes, instance indices) for the oracle"""
    bounds = np.array([np.concatenate([v[:, :3].min(0), v[:, :3].max(0)]) for v in verts], np.float32)
    h = C.c_void_p()
    tb.check(tb.lib.tbvh_host_build_tlas(C.c_void_p(instances.ctypes.data), instances.shape[0], C.c_void_p(bounds.ctypes.data), len(verts), C.byref(h)), "tbvh_host_build_tlas")
    host = tb.HostBVH.__new__(tb.HostBVH)
    host._h = h; host.layout = tb.LAYOUT_BVH_GPU; host.verts = None; host.n_tris = instances.shape[0]
    return host


def traced_on_the_cpu(oracle):
    """the camera rays through the oracle's TLAS traversal: 4096 records, misses included"""
    from oracle_lib import tlas_intersect
    sc = scene()
    inst = sc.instances.copy()
    h = host_tlas(inst, sc.verts)
    bl = [(b.bvh2_nodes(), b.bvh2_prim_idx(), v) for b, v in zip(sc.host_bvhs(), sc.verts)]
    return tlas_intersect(oracle, h.blob(2, np.uint32, 8), h.blob(1, np.uint32, 1), inst, bl, sc.camera_rays()), inst


def assert_classes_present(records, out, flags):
    """the record classes the issue lists are really in a synthetic set (out, flags: the restatement's)"""
    sc = scene()
    hit = records["t"] < 1e30
    assert (~hit).any() and hit.sum() > 4000
    assert ((records["u"] == 0) & (records["v"] == 0) & hit).any()
    assert ((records["u"] + records["v"] == 1) & (records["u"] > 0) & (records["v"] > 0) & hit).any()
    assert (flags & TU_INTEGER).astype(bool).sum() >= 4
    wrapped = (flags & WRAPPED).astype(bool)
    oob = (flags & REF_OUT_OF_BOUNDS).astype(bool)
    assert (wrapped & ~oob).any(), "a wrap whose reference read is inside the texture"
    assert (wrapped & oob).any(), "a wrap whose reference read is outside the texture"
    assert (wrapped & oob & (records["prim"] == TRI_WRAP_U_LAST_ROW)).any() and (wrapped & ~oob & (records["prim"] == TRI_WRAP_U)).any()   # the last row, and not
    a, b = sc.pairs                                           # both sides: the pair's geometric normals are opposite
    nz = np.abs(out[a, 4:7]).sum(1) > 0
    assert nz.sum() > 150 and np.array_equal(out[a, 4:7][nz], -out[b, 4:7][nz])
    assert (np.abs(out[hit, 4:7]).sum(1) == 0).any() and (np.abs(out[hit, 8:11]).sum(1) == 0).any()   # the zero normals stayed zero
    assert len(np.unique(out[hit, 7].view(np.uint32))) == 4 and set(np.unique(records["inst"][hit])) == {0, 1, 2, 3, 4}
    alphas = out[hit, 11].view(np.uint32) >> 24
    assert {0, 2, 3} <= set(alphas.tolist())


# ---- posed meshes: the bunny cut of slot 0 with tests/pose_lib.py's skeleton and morph targets ------------------------------------------------------
def pose_cases():
    """{"skin": ..., "skin_indexed": ..., "morph": ...}: the inputs of the FatTri half of SetPose over slot 0's records.  Rest normals are random unit
    vectors per vertex (per shared vertex for the indexed form, whose flat twin gathers them); the morph targets get normals of their own."""
    import pose_lib as P
    sc = scene()
    rng = np.random.default_rng(55)
    rest_i, joints_i, weights_i, jy, idx = P.skinned_bunny(indexed=True)
    nrm_i = _unit(rng.normal(size=(rest_i.shape[0], 3)).astype(np.float32))
    flat = idx.reshape(-1)
    mats = np.stack([P.joint_mats(jy, 1), P.joint_mats(jy, 2, scale=True)])
    skin_i = dict(rest=rest_i, joints=joints_i, weights=weights_i, normals=nrm_i, indices=idx, mats=mats)
    skin = dict(rest=np.ascontiguousarray(rest_i[flat]), joints=np.ascontiguousarray(joints_i[flat]), weights=np.ascontiguousarray(weights_i[flat]),
                normals=np.ascontiguousarray(nrm_i[flat]), indices=None, mats=mats)
    assert np.array_equal(skin["rest"][:, :3], sc.verts[0][:, :3]) and idx.shape[0] == sc.fat[0].size
    pos, w = P.morph_bunny()
    nrm = _unit(rng.normal(size=pos.shape).astype(np.float32))
    nrm[1:] *= np.float32(0.4)                                  # (targets bend the base normal; the sum is far from unit length)
    return dict(skin=skin, skin_indexed=skin_i, morph=dict(positions=pos, normals=np.ascontiguousarray(nrm), weights=w))


def host_posed(case, kind, frame):
    """the posed FatTri array of slot 0 through the library's host path: tbvh_host_pose_* + tbvh_host_pose_*_normals + tbvh_host_pose_update_fat_tris"""
    fat = scene().fat[0]
    if kind == "morph":
        v = tb.host_pose_morph(case["positions"], case["weights"][frame])
        return tb.host_pose_fat_tris(fat, v, tb.host_pose_morph_normals(case["normals"]), skin=False)
    v = tb.host_pose_skin(case["rest"], case["joints"], case["weights"], case["mats"][frame])
    n = tb.host_pose_skin_normals(case["normals"], case["joints"], case["weights"], case["mats"][frame])
    return tb.host_pose_fat_tris(fat, v, n, indices=case["indices"], skin=True)


# ---- session fixtures ----------------------------------------------------------------------------------------------------------------------------
shade_oracle = nb.oracle_fixture("oracle_shade", _L.compile_oracle)
shade_ref = nb.ref_fixture("shade_ref", _L.compile_ref_shim)


@pytest.fixture(scope="session")
def shade_sets(shade_oracle, oracle):
    """{name: (records, instances, the restatement's (n, 12) records, its flags)} for the traced and the synthetic set, computed once and never changed"""
    sc = scene()
    traced, inst = traced_on_the_cpu(oracle)
    syn = sc.synthetic_records()
    sets = {}
    for name, r in (("traced", traced), ("synthetic", syn)):
        out, flags = shade_oracle.shade(sc.materials, sc.textures, sc.fat, r, inst)
        for a in (r, out, flags):
            a.flags.writeable = False
        sets[name] = (r, inst, out, flags)
    assert_classes_present(syn, sets["synthetic"][2], sets["synthetic"][3])
    hit = traced["t"] < 1e30
    assert traced.shape[0] == CAMERA_SIDE ** 2 and hit.sum() > 300 and (~hit).sum() > 300 and set(np.unique(traced["inst"][hit])) == {0, 1, 2, 3, 4}
    return sets
