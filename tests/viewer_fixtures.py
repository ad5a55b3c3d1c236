"""The scenes, skies and directions of the viewer tests (test_viewer_host.py, test_viewer_gpu.py): the smallest at which the kernels can still go wrong.
The frame scene is the scene of tests/shade_fixtures.py plus a third BLAS slot of quads — a floor, a stack of 9 masked quads before an opaque one (the
8-round cap), 3 masked then opaque, masked then sky — with two more textures that the two alpha rules judge differently: texels ( 1, 1, 1, alpha 255 ) are
masked for tiny_bvh_gltf.cpp (x + y + z <= 5) and opaque for tiny_bvh_foliage.cpp (alpha > 2), texels ( 200, 100, 50, alpha 0 ) the other way round.
Everything is made from seeds; nothing here needs a GPU."""
import functools

import numpy as np

import native_build as nb
import tinybvh_amd as tb
import shade_fixtures as SF
import viewer_lib
from shade_lib import FATTRI_DTYPE, MATERIAL_DTYPE, NO_TEXTURE

SKY_SHAPES = [(1, 1), (5, 7), (8, 16)]          # (h, w): 1 x 1, 7 x 5, 16 x 8
FRAME_SKY = (32, 64)                             # the frames' sky: small enough that the SKY_EDGE pixels stay under 1 / 2000 (test_viewer_host.py checks it)
FRAME_SIZES = [(1, 1), (3, 5), (70, 3), (800, 600)]   # (w, h); 70 x 3 ends in a partial wave
MAT_FLOOR, MAT_GLTF_MASKED, MAT_FOLIAGE_MASKED = 4, 5, 6
TEXEL_GLTF_MASKED, TEXEL_FOLIAGE_MASKED = 0xFF010101, 0x003264C8
N_RANDOM_DIRS = 4096


def sky(shape, seed=5):
    h, w = shape
    return np.random.default_rng(seed + 100 * h + w).uniform(0.0, 2.5, (h, w, 3)).astype(np.float32)


def sky_directions():
    """(dirs (n, 3) float32, classes: name -> index array): the special directions first, then 4096 random unit and non-unit vectors"""
    up = np.nextafter(np.float32(1), np.float32(2))
    special = {
        "pole_up": [(0.0, 1.0, 0.0)], "pole_down": [(0.0, -1.0, 0.0)],
        "minus_x_plus_zero": [(-1.0, 0.0, 0.0), (-0.5, 0.3, 0.0)], "minus_x_minus_zero": [(-1.0, 0.0, -0.0), (-0.5, 0.3, -0.0)],
        "wrap": [(0.3, 0.1, -0.7), (-0.3, -0.2, -0.01), (1.0, 0.0, -1e-3)],
        "atan2_zero_zero": [(0.0, 1.0, 0.0), (0.0, -1.0, 0.0), (0.0, 1.0, -0.0), (-0.0, -1.0, 0.0)],
        "y_above_one": [(0.0, up, 0.0), (0.0, -up, 0.0), (0.1, 1.5, 0.1), (0.1, -2.0, -0.1)],
        "nan": [(np.nan, 0.0, 1.0), (0.0, np.nan, 1.0), (1.0, 0.0, np.nan)],
    }
    rows, classes = [], {}
    for name, vs in special.items():
        classes[name] = np.arange(len(rows), len(rows) + len(vs))
        rows += vs
    rng = np.random.default_rng(9)
    r = rng.normal(size=(N_RANDOM_DIRS, 3))
    r[: N_RANDOM_DIRS // 2] /= np.linalg.norm(r[: N_RANDOM_DIRS // 2], axis=1, keepdims=True)
    r[N_RANDOM_DIRS // 2:] *= rng.uniform(0.1, 1.2, (N_RANDOM_DIRS // 2, 1))
    classes["random"] = np.arange(len(rows), len(rows) + N_RANDOM_DIRS)
    d = np.concatenate([np.array(rows, np.float32), r.astype(np.float32)])
    return np.ascontiguousarray(d), classes


def defined_directions(dirs):
    """the directions for which the reference's SampleSky is defined: no NaN, |D.y| <= 1 (acosf of anything else is a NaN converted to an index)"""
    return ~np.isnan(dirs).any(1) & (np.abs(dirs[:, 1]) <= 1)


def _quad(cx, cy, z, half):
    """two triangles of an axis-aligned square in the plane z, facing +z"""
    a, b, c, d = (cx - half, cy - half, z), (cx + half, cy - half, z), (cx + half, cy + half, z), (cx - half, cy + half, z)
    return [a, b, c, a, c, d]


class ViewerScene:
    """verts[s], fat[s] for three BLAS slots, six instances, seven materials, six textures; camera(): the view pyramid the frames use"""

    def __init__(self):
        base = SF.scene()
        ext, c = base.extent, base.centre.astype(np.float64)
        self.extent, self.centre = ext, base.centre
        self.textures = [t.copy() for t in base.textures] + [np.full((2, 2), TEXEL_GLTF_MASKED, np.uint32), np.full((2, 2), TEXEL_FOLIAGE_MASKED, np.uint32)]
        m = np.zeros(7, MATERIAL_DTYPE)
        m[:4] = base.materials
        m["color"][4:] = [(0.6, 0.6, 0.6), (0.5, 0.5, 0.5), (0.5, 0.5, 0.5)]
        m["color_texture"][4:] = [NO_TEXTURE, 4, 5]
        m["normal_texture"][4:] = NO_TEXTURE
        self.materials = m
        # the third slot: quads in planes of constant z in front of the bunnies (the camera looks down -z), and a floor under everything
        z0, step, half = float(c[2]) + 1.6 * ext, 0.05 * ext, 0.16 * ext
        tris, mats = [], []

        def add(q, mat):
            tris.extend(q); mats.extend([mat, mat])
        self.stack_centres = {"cap": (c[0] - 1.5 * ext, c[1] - 0.2 * ext), "three": (c[0] - 1.5 * ext, c[1] + 0.5 * ext), "then_sky": (c[0] - 1.5 * ext, c[1] + 1.3 * ext),
                              "foliage_masked": (c[0] + 1.5 * ext, c[1] + 0.5 * ext)}
        for k in range(9):                                                       # 9 masked layers, nearest first for the camera, then an opaque one
            add(_quad(*self.stack_centres["cap"], z0 - k * step, half), MAT_GLTF_MASKED)
        add(_quad(*self.stack_centres["cap"], z0 - 9 * step, half), MAT_FLOOR)
        for k in range(3):
            add(_quad(*self.stack_centres["three"], z0 - k * step, half), MAT_GLTF_MASKED)
        add(_quad(*self.stack_centres["three"], z0 - 3 * step, half), MAT_FLOOR)
        add(_quad(*self.stack_centres["then_sky"], z0, half), MAT_GLTF_MASKED)
        add(_quad(*self.stack_centres["foliage_masked"], z0, half), MAT_FOLIAGE_MASKED)
        y_floor, big = float(c[1]) - 1.25 * ext, 3.0 * ext
        fl = [(c[0] - big, y_floor, c[2] + big), (c[0] + big, y_floor, c[2] + big), (c[0] + big, y_floor, c[2] - big), (c[0] - big, y_floor, c[2] - big)]
        add([fl[0], fl[1], fl[2], fl[0], fl[2], fl[3]], MAT_FLOOR)              # (faces +y)
        v = np.zeros((len(tris), 4), np.float32)
        v[:, :3] = np.array(tris, np.float64).astype(np.float32)
        f = SF.fat_tris(v, 33)
        f["material"] = np.array(mats, np.uint32)
        for k in range(3):
            f[f"vN{k}"] = np.stack([f["Nx"], f["Ny"], f["Nz"]], 1)              # flat shading: the vertex normals are the geometric one
        self.verts = [base.verts[0], base.verts[1], v]
        self.fat = [base.fat[0], base.fat[1], f]
        T = np.tile(np.eye(4, dtype=np.float32), (6, 1, 1))
        T[:5] = base.instances.view(np.float32).reshape(5, 48)[:, :16].reshape(5, 4, 4)
        self.instances = tb.make_instances(T, [0, 0, 0, 0, 1, 2])
        self.slot_of_inst = np.array([0, 0, 0, 0, 1, 2])
        self.n_textures = len(self.textures)

    def camera(self, width, height):
        """UpdateCamera's pyramid for an eye in front of the scene looking down -z, a little from above"""
        eye = (self.centre + np.array([0.1, 0.45, 4.0], np.float32) * np.float32(self.extent)).astype(np.float32)
        view = np.array([0.0, -0.08, -1.0], np.float32)
        view /= np.float32(np.sqrt((view * view).sum(dtype=np.float32)))
        right = np.cross(np.array([0, 1, 0], np.float32), view).astype(np.float32)
        right /= np.float32(np.sqrt((right * right).sum(dtype=np.float32)))
        up = (np.float32(0.8) * np.cross(view, right)).astype(np.float32)
        C = eye + np.float32(1.2) * view
        return tb.viewer_camera(eye, C - right + up, C + right + up, C - right - up, width, height)

    def host_bvhs(self):
        return [tb.HostBVH(v, tb.LAYOUT_CWBVH) for v in self.verts]


def default_light():
    """normalize( 2, 4, 5 ) as tinybvh_normalize computes it"""
    f = np.float32
    l = f(np.sqrt(f(f(5) * f(5) + f(f(2) * f(2) + f(4) * f(4)))))
    rl = f(1) / l
    return np.array([f(2) * rl, f(4) * rl, f(5) * rl], np.float32)


def scene_kind(sc, kind):
    """(verts, FatTri arrays, instance records with bounds and inverses filled, the instance records the LIBRARY's shading takes) for the fixture as a TLAS
    ("tlas") or its third BLAS alone ("blas": one identity instance for the reference's viewers, which always trace a TLAS; None for the library)"""
    if kind == "tlas":
        verts, fat, inst = sc.verts, sc.fat, sc.instances.copy()
    else:
        verts, fat = [sc.verts[2]], [sc.fat[2]]
        inst = tb.make_instances(np.eye(4, dtype=np.float32)[None], [0])
    SF.host_tlas(inst, verts)                                                # (fills the bounds and the inverses in place)
    return verts, fat, inst, (inst if kind == "tlas" else None)


@functools.lru_cache(maxsize=1)
def scene():
    return ViewerScene()


def synthetic_lighting_records(n=2048 + 37, seed=3):
    """(rays, out48 (n, 12) float32, occ): records whose D, hit.t, albedo, alpha, material, iN and texel are set directly — hits, hits beyond 10000, misses,
    "no surface", masked by either rule, NaN and zero normals — for the light, continue, shadow-ray and pack stages, which look at nothing else"""
    sc = scene()
    rng = np.random.default_rng(seed)
    r = tb.make_rays(rng.normal(size=(n, 3)).astype(np.float32) * 3, rng.normal(size=(n, 3)).astype(np.float32))
    r["t"] = rng.uniform(0.5, 40, n).astype(np.float32)
    r["t"][::13] = 1e30
    r["t"][5::17] = rng.uniform(10000, 50000, r["t"][5::17].size).astype(np.float32)
    r["t"][6::97] = 10000.0
    r["u"], r["v"], r["prim"], r["inst"] = 0.25, 0.25, rng.integers(0, 50, n), rng.integers(0, 6, n)
    o = np.zeros((n, 12), np.float32)
    o[:, 0:3] = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    o[:, 3] = rng.choice(np.array([0, 1], np.float32), n)
    iN = rng.normal(size=(n, 3)); iN /= np.linalg.norm(iN, axis=1, keepdims=True)
    o[:, 8:11] = iN.astype(np.float32)
    ow = o.view(np.uint32)
    ow[:, 7] = rng.integers(0, 7, n)
    texel = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    texel[::3] = rng.integers(0, 4, texel[::3].size).astype(np.uint32) * 0x010101 + (rng.integers(0, 256, texel[::3].size).astype(np.uint32) << 24)   # sums 0, 3, 6, 9
    ow[:, 11] = texel
    miss = r["t"] >= 1e30
    o[miss] = 0; o[miss, 3] = -1                                                  # "no surface"
    o[7::101] = 0; o[7::101, 3] = -1                                              # ... also on records that hit (a bad index, a sphere BLAS)
    ow[11::103, 7] = 0x80000001                                                   # a material index beyond the table
    o[12::107, 8:11] = 0                                                          # zero normals
    o[14::109, 8] = np.nan
    o[15::113, 0] = 7.5                                                           # a colour beyond 1
    occ = rng.integers(0, 2, n).astype(np.uint8)
    return r, o, occ


# ---- session fixtures -----------------------------------------------------------------------------------------------------------------------------
viewer_oracle = nb.oracle_fixture("oracle_viewer", viewer_lib.compile_oracle)
