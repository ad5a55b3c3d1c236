"""The small scenes of the per-path checks of the path tracer (tests/test_wavefront_paths_gpu.py, tests/test_wavefront_ref_host.py), their oracle
traversals, and the reference (tests/wavefront_ref.py) run as a complete path tracer on the CPU."""
import ctypes as C

import numpy as np

import tinybvh_amd as tb
import wavefront_ref as wr
from oracle_lib import tlas_intersect

DIFFUSE, LIGHT, MIRROR = tb.MATERIAL_DIFFUSE << 24, tb.MATERIAL_LIGHT << 24, tb.MATERIAL_SPECULAR << 24
W_A, H_A = 72, 52          # 3744 paths: 3 full Shade workgroups of 1024 and a partial one, 14 full Generate / Connect blocks of 256 and a partial one


def grid(p0, du, dv, nu, nv, material):
    """A parallelogram p0 + s du + t dv as nu x nv cells of two triangles, the material word in v0.w of each triangle."""
    p0, du, dv = (np.asarray(x, np.float64) for x in (p0, du, dv))
    s, t = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    a = p0 + s[..., None] * du / nu + t[..., None] * dv / nv
    b, c, d = a + du / nu, a + du / nu + dv / nv, a + dv / nv
    tris = np.stack([np.stack([a, b, c], -2), np.stack([a, c, d], -2)], -3).reshape(-1, 3, 3)
    return pack(tris, material)


def sphere(c, r, nu, nv, material, squash=(1.0, 1.0, 1.0)):
    th = np.linspace(0, 2 * np.pi, nu + 1); ph = np.linspace(0.02, np.pi - 0.02, nv + 1)
    P = lambda i, j: np.asarray(c) + r * np.asarray(squash) * np.array([np.cos(th[i]) * np.sin(ph[j]), np.cos(ph[j]), np.sin(th[i]) * np.sin(ph[j])])
    tris = []
    for i in range(nu):
        for j in range(nv):
            tris += [[P(i, j), P(i + 1, j), P(i + 1, j + 1)], [P(i, j), P(i + 1, j + 1), P(i, j + 1)]]
    return pack(np.array(tris), material)


def pack(tris, material):
    v = np.zeros((tris.shape[0] * 3, 4), np.float32)
    v[:, :3] = tris.reshape(-1, 3)
    v[0::3, 3] = np.array([material], np.uint32).view(np.float32)[0]
    return v


def camera(eye, target, up_hint, fov, W, H):
    """A pinhole whose screen is the rectangle p1 (top left), p2 (top right), p3 (bottom left) one unit in front of the eye."""
    e, t = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    f = (t - e) / np.linalg.norm(t - e)
    r = np.cross(np.asarray(up_hint, np.float64), f); r /= np.linalg.norm(r)
    u = np.cross(f, r)
    hw, hh = fov, fov * H / W
    cam = tb.Camera()
    cam.eye[:] = [float(x) for x in e]
    cam.p1[:] = [float(x) for x in e + f - hw * r + hh * u]
    cam.p2[:] = [float(x) for x in e + f + hw * r + hh * u]
    cam.p3[:] = [float(x) for x in e + f - hw * r - hh * u]
    cam.width, cam.height, cam.spp_x, cam.spp_y = W, H, 1, 1
    return cam


class SingleLevel:
    """A triangle soup with its host-built tree: what Extend and Connect must report, by the oracle on the BVH2 the device's layout was made from."""

    def __init__(self, verts, layout=tb.LAYOUT_CWBVH):
        self.verts = verts
        self.host = tb.HostBVH(verts, layout)
        self.geo = wr.Geometry(verts=verts)

    def intersect(self, orc, rays):
        return orc.bvh2_intersect(self.host.bvh2_nodes(), self.host.bvh2_prim_idx(), self.verts, rays)

    def occluded(self, orc, rays):
        return orc.bvh2_occluded(self.host.bvh2_nodes(), self.host.bvh2_prim_idx(), self.verts, rays)


class TwoLevel:
    """Instances over BLASes: the host TLAS as TLAS.Build makes it (which fills invTransform and the bounds of `instances`)."""

    def __init__(self, blas_verts, layouts, transforms, blas_idx):
        self.blas_verts = blas_verts
        self.blas_host = [tb.HostBVH(v, l) for v, l in zip(blas_verts, layouts)]
        self.layouts = layouts
        self.instances = tb.make_instances(np.asarray(transforms, np.float32), np.asarray(blas_idx, np.uint32))
        bounds = np.array([np.concatenate([v[:, :3].min(0), v[:, :3].max(0)]) for v in blas_verts], np.float32)
        h = C.c_void_p()
        tb.check(tb.lib.tbvh_host_build_tlas(C.c_void_p(self.instances.ctypes.data), self.instances.shape[0], C.c_void_p(bounds.ctypes.data), len(blas_verts), C.byref(h)),
                 "tbvh_host_build_tlas")
        host = tb.HostBVH.__new__(tb.HostBVH)
        host._h = h; host.layout = tb.LAYOUT_BVH_GPU; host.verts = None; host.n_tris = self.instances.shape[0]
        self.host = host
        self.geo = wr.Geometry(instances=self.instances, blas_verts=blas_verts)

    def intersect(self, orc, rays):
        bl = [(b.bvh2_nodes(), b.bvh2_prim_idx(), v) for b, v in zip(self.blas_host, self.blas_verts)]
        return tlas_intersect(orc, self.host.blob(2, np.uint32, 8), self.host.blob(1, np.uint32, 1), self.instances, bl, rays)

    def occluded(self, orc, rays):
        return (self.intersect(orc, rays)["t"] < rays["t"]).astype(np.uint8)


# ---- Scene A: a closed room with every material among the first hits ----------------------------------------------------------

LIGHT_A = dict(light_pos=(0.0, 7.5, 0.0), light_color=(22.0, 20.0, 17.0), light_size=(9.0, 5.0), sky_lo=(0.6, 0.7, 0.8), sky_hi=(0.2, 0.4, 0.9), eps=1e-3)


def scene_a_verts():
    """x -6 .. 6, y 0 .. 8, z -6 .. 6: a coloured floor, a 70 % grey back wall (RGB 0), two facing mirror walls (x = -6, x = 6: specular chains as deep as the
    frame allows), a coloured wall behind the camera, a ceiling that stops at z = 3 (the sky shows beyond), the 9 x 5 lamp facing down at y = 7.5, a squashed
    coloured ball and a tilted mirror on the floor, a small tilted diffuse panel.  About 2.3 k triangles."""
    parts = [
        grid((-6, 0, -6), (12, 0, 0), (0, 0, 12), 12, 12, DIFFUSE | 0xC08040),
        grid((-6, 0, 6), (12, 0, 0), (0, 8, 0), 10, 8, DIFFUSE | 0),
        grid((-6, 0, -6), (0, 0, 12), (0, 8, 0), 6, 4, MIRROR | 0xF0F0F0),
        grid((6, 0, -6), (0, 8, 0), (0, 0, 12), 4, 6, MIRROR | 0xE0F0FF),
        grid((-6, 0, -6), (0, 8, 0), (12, 0, 0), 8, 10, DIFFUSE | 0x4060C0),
        grid((-6, 8, -6), (0, 0, 9), (12, 0, 0), 9, 12, DIFFUSE | 0xB0B0A0),
        grid((-4.5, 7.5, -2.5), (0, 0, 5), (9, 0, 0), 2, 3, LIGHT | 0xFFFFFF),
        sphere((-2.0, 1.2, 2.0), 1.2, 24, 16, DIFFUSE | 0x30A040, squash=(1.0, 0.8, 1.3)),
        grid((1.5, 0.0, 3.5), (2.2, 0.4, -1.1), (-0.3, 2.6, 0.5), 3, 3, MIRROR | 0xFFE0C0),
        grid((2.5, 0.3, 0.0), (1.4, 0.2, 0.9), (-0.5, 1.9, 0.4), 4, 4, DIFFUSE | 0xD02020),
    ]
    return np.concatenate(parts)


def camera_a(W=W_A, H=H_A):
    return camera((0.3, 3.0, -5.5), (0.5, 3.6, 6.0), (0, 1, 0), 0.75, W, H)


# ---- Scene B: the same kinds of surfaces under instances -----------------------------------------------------------------------

def rot(axis, deg):
    a = np.deg2rad(deg); c, s = np.cos(a), np.sin(a)
    M = np.eye(4)
    i, j = {"x": (1, 2), "y": (2, 0), "z": (0, 1)}[axis]
    M[i, i] = c; M[i, j] = -s; M[j, i] = s; M[j, j] = c
    return M


def translate(x, y, z):
    M = np.eye(4); M[:3, 3] = (x, y, z)
    return M


LIGHT_B = dict(light_pos=(0.0, 6.0, 0.0), light_color=(14.0, 13.0, 12.0), light_size=(9.0, 5.0), sky_lo=(0.5, 0.6, 0.7), sky_hi=(0.1, 0.3, 0.8), eps=1e-3)


def scene_b():
    """A diffuse floor (unit grid scaled 14 x 1 x 10), a diffuse ball under a non-uniform scale and a rotation, the same ball MIRRORED (negative determinant),
    a mirror panel scaled non-uniformly and tilted, the lamp (a 5 x 9 rectangle turned 90 degrees about y and lifted): three BLAS layouts."""
    unit = grid((-0.5, 0, -0.5), (1, 0, 0), (0, 0, 1), 6, 6, DIFFUSE | 0xC0C060)
    ball = sphere((0, 0, 0), 1.0, 16, 10, DIFFUSE | 0x4080E0)
    panel = grid((-0.5, 0, -0.5), (1, 0, 0), (0, 0, 1), 2, 2, MIRROR | 0xF0E0D0)
    lamp = grid((-2.5, 0, -4.5), (0, 0, 9), (5, 0, 0), 2, 2, LIGHT | 0xFFFFFF)
    T = [np.diag([14.0, 1.0, 10.0, 1.0]),
         translate(-2.0, 1.3, 1.0) @ rot("z", 20.0) @ rot("x", -15.0) @ np.diag([1.6, 0.9, 1.2, 1.0]),
         translate(2.2, 1.1, 1.5) @ rot("y", 30.0) @ np.diag([-1.1, 1.0, 0.8, 1.0]),
         translate(0.0, 2.0, 4.0) @ rot("x", -70.0) @ rot("z", 8.0) @ np.diag([7.0, 1.0, 3.5, 1.0]),
         translate(0.0, 6.0, 0.0) @ rot("y", 90.0)]
    return TwoLevel([unit, ball, panel, lamp], [tb.LAYOUT_CWBVH, tb.LAYOUT_BVH4_GPU, tb.LAYOUT_BVH_GPU, tb.LAYOUT_CWBVH], np.array(T), [0, 1, 1, 2, 3])


def camera_b(W=64, H=64):
    return camera((0.2, 2.6, -6.0), (0.0, 1.4, 1.0), (0, 1, 0), 0.6, W, H)


# ---- two scripted edge scenes ----------------------------------------------------------------------------------------------------

def scene_grazing():
    """A floor 0.01 under the plane of the lamp's samples (the lamp itself is not modelled: next event estimation needs only its rectangle): from the floor
    most samples lie at grazing incidence (|L.y| small: the solid angle nears 0), and right under a sample the solid angle passes 2 pi (the clamp)."""
    return grid((-7, 0, -5), (14, 0, 0), (0, 0, 10), 4, 4, DIFFUSE | 0xC0C0C0)


GRAZING = dict(light_pos=(0.0, 0.01, 0.0), light_color=(3.0, 3.0, 3.0), light_size=(9.0, 5.0), sky_lo=(0.0, 0.0, 0.0), sky_hi=(0.0, 0.0, 0.0), eps=1e-3)


def camera_grazing(W=64, H=64):
    return camera((0.0, 3.0, -0.5), (0.0, 0.0, 0.0), (0, 0, 1), 1.6, W, H)


def scene_near_point_light():
    """A floor whose middle lies closer to the point light than 2 eps: no shadow ray from there (ldist <= 2 eps), ordinary ones further out."""
    return grid((-1, 0, -1), (2, 0, 0), (0, 0, 2), 3, 3, DIFFUSE | 0xFFFFFF)


NEAR = dict(light_pos=(0.0, 0.001, 0.0), light_color=(1e-4, 1e-4, 1e-4), light_size=(0.0, 0.0), sky_lo=(0.0, 0.0, 0.0), sky_hi=(0.0, 0.0, 0.0), eps=1e-3)


def camera_near(W=64, H=64):
    return camera((0.0, 0.5, 0.0), (0.0, 0.0, 0.0), (0, 0, 1), 0.012, W, H)


# ---- the cases both test files run: (scene, camera, parameters, max_depth, seed) ------------------------------------------------------

def blue_table(seed=77):
    """A seeded stand-in for the demos' 128 x 128 x 8 table: two 8-bit channels per word (bits 8 .. 23), the low byte unused."""
    return (np.random.default_rng(seed).integers(0, 1 << 24, 128 * 128 * 8, dtype=np.uint32)).astype(np.uint32)


CASES = {
    "scene_a": lambda: (SingleLevel(scene_a_verts()), camera_a(), dict(LIGHT_A), 4, 5),
    "scene_a_one_bounce": lambda: (SingleLevel(scene_a_verts()), camera_a(), dict(LIGHT_A, one_diffuse_bounce=True), 4, 5),
    "scene_a_chain": lambda: (SingleLevel(scene_a_verts()), camera_a(), dict(LIGHT_A), 8, 6),
    "scene_a_point_light": lambda: (SingleLevel(scene_a_verts()), camera_a(), dict(LIGHT_A, light_size=(0.0, 0.0)), 2, 7),
    "scene_a_letter": lambda: (SingleLevel(scene_a_verts()), camera_a(), dict(LIGHT_A, reference_letter=True), 3, 8),
    "scene_a_blue_0": lambda: (SingleLevel(scene_a_verts()), camera_a(), dict(LIGHT_A, sample_index=0, blue_noise=blue_table()), 2, 12),
    "scene_a_blue_3": lambda: (SingleLevel(scene_a_verts()), camera_a(), dict(LIGHT_A, sample_index=3, blue_noise=blue_table()), 2, 12),
    "scene_a_blue_4": lambda: (SingleLevel(scene_a_verts()), camera_a(), dict(LIGHT_A, sample_index=4, blue_noise=blue_table()), 2, 12),
    "scene_a_blue_off": lambda: (SingleLevel(scene_a_verts()), camera_a(), dict(LIGHT_A, sample_index=0xFFFFFFFF, blue_noise=blue_table()), 2, 12),
    "scene_b": lambda: (scene_b(), camera_b(), dict(LIGHT_B), 3, 9),
    "grazing": lambda: (SingleLevel(scene_grazing()), camera_grazing(), dict(GRAZING), 1, 10),
    "near_point_light": lambda: (SingleLevel(scene_near_point_light()), camera_near(), dict(NEAR), 1, 11),
}


# ---- the reference as a complete path tracer -------------------------------------------------------------------------------------

def trace_cpu(orc, scene, cam, seed, max_depth, first_row=0, band_rows=None, **kw):
    """Generate, { Extend (oracle), Shade (reference), Connect (oracle) } x depth on the CPU.  The queues between the stages are the reference's values rounded
    to float32, in path order.  Returns one dict per stage: the Shade input with hit records, the reference's output, the shadow queue and its flags."""
    W = int(cam.width)
    rows = int(cam.height) if band_rows is None else band_rows
    P = wr.Params(max_depth=max_depth, seed=seed, width=W, height=int(cam.height), pixel_offset=first_row * W, **kw)
    g = wr.generate(cam, seed, first_row, rows)
    D = np.stack([c.v for c in g["D"]], -1)
    rays, aux = wr.make_queue(tb.RAY_DTYPE, tb.PATH_AUX_DTYPE, g["O"], D, 1.0, 1e30, 1.0, g["word"])
    stages = []
    for d in range(P.max_depth):
        hit = scene.intersect(orc, rays) if rays.shape[0] else rays
        ref = wr.shade(hit, aux, scene.geo, P, d)
        ws = ref["want_shadow"]
        sh, sh_aux = wr.make_queue(tb.RAY_DTYPE, tb.PATH_AUX_DTYPE, ref["shadow_O"][0][ws], ref["shadow_D"][0][ws], 1.0, ref["shadow_tmax"][0][ws], ref["contrib"][0][ws],
                                   ref["pixel"][ws].astype(np.uint32))
        sh["instIdx"] = np.float32(1.0).view(np.uint32)
        occ = scene.occluded(orc, sh) if sh.shape[0] else np.zeros(0, np.uint8)
        stages.append({"rays": hit, "aux": aux, "ref": ref, "shadow": sh, "shadow_aux": sh_aux, "occ": occ, "P": P})
        wb = ref["want_bounce"]
        rays, aux = wr.make_queue(tb.RAY_DTYPE, tb.PATH_AUX_DTYPE, ref["bounce_O"][0][wb], ref["bounce_D"][0][wb], ref["bounce_pdf"][0][wb], 1e30, ref["bounce_T"][0][wb],
                                  ref["bounce_word"][wb])
    return stages


def classes(stages):
    """How often each branch of Shade was taken over the stages of one frame (so that no check of it passes on an empty set)."""
    c = dict.fromkeys(("emitter_from_camera", "emitter_after_mirror", "emitter_after_diffuse", "sky_after_diffuse", "sky_after_mirror", "diffuse_mirror_diffuse",
                       "one_bounce_stop", "nee_ndl_rejected", "nee_occluded"), 0)
    via_dmd = None
    for d, s in enumerate(stages):
        r = s["ref"]
        spec_in, diff_in = (r["flags"] & wr.PATH_LAST_SPECULAR) != 0, (r["flags"] & wr.PATH_VIA_DIFFUSE) != 0
        if d == 0:
            c["emitter_from_camera"] += int(r["emitter"].sum())
        else:
            c["emitter_after_mirror"] += int((r["emitter"] & spec_in).sum())
            c["sky_after_mirror"] += int((r["miss"] & spec_in).sum())
        c["emitter_after_diffuse"] += int(r["mis_light"].sum())
        c["sky_after_diffuse"] += int((r["miss"] & diff_in).sum())
        c["one_bounce_stop"] += int(r["stopped"].sum())
        c["nee_ndl_rejected"] += int(r["ndl_rejected"].sum())
        c["nee_occluded"] += int(np.asarray(s["occ"]).astype(bool).sum())
        # diffuse -> mirror -> diffuse: a path that was diffuse two stages ago, specular one stage ago and is diffuse now
        if via_dmd is not None:
            c["diffuse_mirror_diffuse"] += int((r["diffuse"] & np.isin(r["pixel"], via_dmd)).sum())
        via_dmd = r["pixel"][r["specular"] & diff_in]
    return c


def undecided_share(stages):
    """Per stage: undecided paths / live paths."""
    return [float((s["ref"]["undecided"] != 0).sum()) / max(1, s["ref"]["n"]) for s in stages]
