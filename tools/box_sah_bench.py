"""The SAH builder over boxes and its one-workgroup path (DESIGN.md par. 20), in one run: (1) the threshold sweep — build time of k_sah_one_group against the
per-level path (small-subtree threshold 64) over n boxes and soup(n) triangles, device-resident input and output; (2) sphere scenes: build and rebuild
time and rays per second through the LBVH, PLOC and SAH trees; (3) TLASes: device rebuild time and rays per second, LBVH against SAH (`tlas` as a second argument: that part alone).  Times: best of 4 after one warm-up, device time (tbvh_time_last_ms), wall in brackets.
Writes profiles/box_sah_build.txt.
    python tools/box_sah_bench.py [out.txt] [tlas]"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tinybvh_amd as tb  # noqa: E402
from tinybvh_amd import scenes  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "box_sah_build.txt")
lines = []
lib = tb.lib


def say(s):
    print(s, flush=True)
    lines.append(s)


def best(ctx, fn, reps=4):
    """(best device ms, best wall ms) of reps calls after one warm-up"""
    dev, wall = [], []
    for it in range(reps + 1):
        ctx.synchronize()
        t0 = time.perf_counter(); fn(); ctx.synchronize(); t = (time.perf_counter() - t0) * 1e3
        if it:
            dev.append(ctx.time_last_ms()); wall.append(t)
    return min(dev), min(wall)


def mixed_boxes(n):
    """tests/boxbuild_lib.py: mixed — small boxes with every 50th a large one"""
    rng = np.random.default_rng(7)
    c = rng.uniform(0, 1, (n, 3)) * np.array([100, 20, 100])
    h = 0.2 + rng.uniform(0, 1, (n, 3))
    big = 5 + 20 * rng.uniform(0, 1, (n, 3))
    h[::50] = big[::50]
    a = np.zeros((n, 8), np.float32)
    a[:, 0:3] = c - h; a[:, 4:7] = c + h
    return a


def set_paths(ctx, one_group, small=64):
    tb.check(lib.tbvh_debug_set_sah_one_group(ctx._h, one_group), "tbvh_debug_set_sah_one_group")
    tb.check(lib.tbvh_debug_set_sah_small_subtree(ctx._h, small), "tbvh_debug_set_sah_small_subtree")


def sweep(ctx):
    global DEFAULTS
    saved = (C.c_uint32 * 2)()
    tb.check(lib.tbvh_debug_get_sah_thresholds(ctx._h, saved), "tbvh_debug_get_sah_thresholds")
    DEFAULTS = (saved[0], saved[1])
    say("== threshold sweep: ms on the device (wall), one workgroup | per-level path T = 64 | one wave (T >= n) ==")
    for n in (256, 1024, 3000, 8192, 16384, 65536):
        row = {}
        for kind in ("boxes", "soup"):
            if kind == "boxes":
                data = mixed_boxes(n)
            else:
                data = scenes.soup(n, seed=5)
            d_in = ctx.malloc(data.nbytes); ctx.to_device(d_in, data)
            d_n = ctx.malloc(2 * n * 32); d_i = ctx.malloc(n * 4)
            nn = C.c_uint64(0)
            mesh = tb.device_mesh(d_in, data.shape[0], n) if kind == "soup" else None

            def build():
                if kind == "boxes":
                    tb.check(lib.tbvh_build_bvh2_sah_device_aabbs(ctx._h, C.c_void_p(d_in), n, 1, 0, C.c_void_p(d_n), 2 * n, C.c_void_p(d_i), n, 1, C.byref(nn)), "aabbs")
                else:
                    tb.check(lib.tbvh_build_bvh2_sah_device(ctx._h, C.byref(mesh), 0, C.c_void_p(d_n), 2 * n, C.c_void_p(d_i), n, 1, C.byref(nn)), "tris")
            for name, (og, small) in (("group", (1 << 14, 64)), ("levels", (0, 64)), ("wave", (0, 1 << 30))):
                if (name == "wave" and n > 8192) or (name == "group" and n > 1 << 14):   # (beyond 2^14 the library takes the level path whatever the threshold says)
                    continue
                set_paths(ctx, og, small)
                row[(kind, name)] = best(ctx, build)
            for d in (d_in, d_n, d_i):
                ctx.free(d)
        set_paths(ctx, DEFAULTS[1], DEFAULTS[0])
        fmt = lambda k: f"{row[k][0]:7.3f} ({row[k][1]:.3f})" if k in row else "      -"
        say(f"n = {n:6d}  boxes: {fmt(('boxes', 'group'))} | {fmt(('boxes', 'levels'))} | {fmt(('boxes', 'wave'))}    soup: {fmt(('soup', 'group'))} | {fmt(('soup', 'levels'))} | {fmt(('soup', 'wave'))}")


def sphere_set(n):
    """tools/sphere_anim_bench.py's random set (its first n spheres)"""
    rng = np.random.default_rng(21)
    s = np.empty((1_000_000, 4), np.float32)
    s[:, :3] = rng.uniform(-10, 10, (s.shape[0], 3))
    s[:, 3] = rng.uniform(0.002, 0.01, s.shape[0]) * 20.0
    return np.ascontiguousarray(s[:n])


def ray_batches(sph, n):
    lo, hi = sph[:, :3].min(0), sph[:, :3].max(0)
    rng = np.random.default_rng(9)
    c, ext = (lo + hi) * 0.5, float((hi - lo).max())
    eye = (c + np.array([0.2, 0.35, 1.6], np.float32) * ext).astype(np.float32)
    tgt = c + rng.uniform(-0.45, 0.45, (n, 3)).astype(np.float32) * (hi - lo)
    cam = tb.make_rays(np.broadcast_to(eye, (n, 3)), tgt - eye)
    inc = tb.make_rays((lo + rng.random((n, 3)).astype(np.float32) * (hi - lo)).astype(np.float32), rng.normal(size=(n, 3)).astype(np.float32))
    return {"camera": cam, "incoherent": inc}


def spheres(ctx, n_rays=1 << 20):
    say("== sphere scenes: build / rebuild ms on the device (wall); G rays/s camera, incoherent ==")
    d_rays = ctx.malloc(n_rays * 64)
    for n in (10_000, 1_000_000):
        sph = sphere_set(n)
        d_s = ctx.malloc(sph.nbytes); ctx.to_device(d_s, sph)
        batches = ray_batches(sph, n_rays)
        for label, kw in (("LBVH", dict(builder="lbvh")), ("PLOC r16", dict(builder="ploc")), ("SAH", dict(builder="sah"))):
            holder = {}

            def build():
                if "sc" in holder:
                    holder["sc"].free()
                holder["sc"] = tb.SphereBVH(ctx).BuildOnDevice((d_s, n), **kw)
            b = best(ctx, build)
            sc = holder["sc"]
            r = best(ctx, lambda: sc.RebuildOnDevice((d_s, n)))
            rate = []
            for kind, rays in batches.items():
                ctx.to_device(d_rays, rays)
                ms = []
                for k in range(4):
                    sc.intersect_device_fresh(d_rays, n_rays, 1e30); ctx.synchronize()
                    if k:
                        ms.append(ctx.time_last_ms())
                rate.append(n_rays / min(ms) / 1e6)
            say(f"n = {n:8d}  {label:9s} build {b[0]:8.3f} ({b[1]:.3f})  rebuild {r[0]:8.3f} ({r[1]:.3f})  camera {rate[0]:6.3f}  incoherent {rate[1]:6.3f}  {sc.device_bytes / 1e6:.1f} MB")
            sc.free()
        ctx.free(d_s)
    ctx.free(d_rays)


def tlas_scene(side, mixed):
    """(a) config 5's layout (DESIGN.md par. 3.5): side^3 equal instances on a grid, scale 0.7, seeded rotation; (b) mixed sizes: the same grid with scales from
    0.05 to 1 and instance 0 scaled to span the whole scene (terrain + props)"""
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    n = g.shape[0]
    ang = (np.arange(n) * 0.37).astype(np.float32)
    scale = np.full(n, 0.7, np.float32)
    if mixed:
        scale = (0.05 * 20.0 ** np.random.default_rng(3).uniform(0, 1, n)).astype(np.float32)
    c_, s_ = np.cos(ang) * scale, np.sin(ang) * scale
    T = np.zeros((n, 4, 4), np.float32)
    T[:, 0, 0] = c_; T[:, 0, 2] = s_; T[:, 1, 1] = scale; T[:, 2, 0] = -s_; T[:, 2, 2] = c_; T[:, 3, 3] = 1
    T[:, :3, 3] = g * 2.0
    if mixed:
        T[0] = np.diag([float(side), 0.05, float(side), 1.0]).astype(np.float32); T[0, :3, 3] = (side - 1.0, -1.0, side - 1.0)   # a flat slab under everything
    return T


def tree_cost(nodes64):
    """sum of area( child box ) / area( root box ) over every child box of the Aila-Laine tree: the expected number of node visits of a random line that
    meets the root box (the SAH's own estimate; the oracle counts no visits)"""
    f = nodes64.view(np.float32)
    inner = nodes64[:, 11] == 0
    def area(lo, hi):
        e = np.maximum(hi - lo, 0).astype(np.float64)
        return e[:, 0] * e[:, 1] + e[:, 1] * e[:, 2] + e[:, 2] * e[:, 0]
    if not inner.any():
        return 1.0
    la, ra = area(f[inner, 0:3], f[inner, 4:7]), area(f[inner, 8:11], f[inner, 12:15])
    lo = np.minimum(f[0, 0:3], f[0, 8:11])[None]; hi = np.maximum(f[0, 4:7], f[0, 12:15])[None]
    return 1.0 + float((la.sum() + ra.sum()) / area(lo, hi)[0])


def tlas(ctx, W=1920, H=1080):
    from tinybvh_amd import rays as R
    say("== TLAS: rebuild ms on the device (wall); G rays/s camera, shadow, random; expected node visits of a random line (SAH estimate) ==")
    blas = tb.BVH8_CWBVH(ctx).Build(scenes.blob(20000, seed=3))
    n_rays = W * H
    d_r = ctx.malloc(n_rays * 64); d_s = ctx.malloc(n_rays * 64); d_o = ctx.malloc(n_rays)
    for side in (10, 20, 40):
        for mixed in (False, True):
            T = tlas_scene(side, mixed)
            n = T.shape[0]
            inst = tb.make_instances(T, np.zeros(n, np.uint32))
            t = tb.TLAS(ctx).Build(inst, [blas])
            ext = 2.0 * side
            cam = R.camera((-0.6 * ext, 0.8 * ext, -0.9 * ext), (0.62, -0.38, 0.68), W, H, 1, 1)
            rnd = R.random_rays(n_rays, (-2, -2, -2), (ext, ext, ext), seed=6)
            for builder in ("lbvh", "sah"):
                t.SetBuilder(builder)
                b = best(ctx, lambda: t.RebuildOnDevice())
                nodes = t.Download()[0]
                rate = {}
                for kind in ("camera", "shadow", "random"):
                    ms = []
                    for k in range(4):
                        if kind == "random":
                            ctx.to_device(d_r, rnd); t.intersect_device(d_r, n_rays)
                        else:
                            ctx.generate_primary(cam, d_r, 0, n_rays); t.intersect_device(d_r, n_rays)
                            if kind == "shadow":
                                ctx.generate_shadow(d_r, d_s, n_rays, (ext * 0.5, ext * 2.0, ext * 0.3), 1e-3); t.occluded_device(d_s, n_rays, d_o)
                        ctx.synchronize()
                        if k:
                            ms.append(ctx.time_last_ms())
                    rate[kind] = n_rays / min(ms) / 1e6
                say(f"n = {n:6d}  {'mixed' if mixed else 'grid ':5s}  {builder:4s}  rebuild {b[0]:7.3f} ({b[1]:.3f})  camera {rate['camera']:6.3f}  shadow {rate['shadow']:6.3f}  "
                    f"random {rate['random']:6.3f}  nodes {nodes.shape[0]:6d}  visits {tree_cost(nodes):6.2f}")
            t.free()
    for d in (d_r, d_s, d_o):
        ctx.free(d)
    blas.free()


def main():
    say("# tools/box_sah_bench.py; times: best of 4 after one warm-up")
    ctx = tb.Context(0)
    if "tlas" not in sys.argv[2:]:
        sweep(ctx)
        spheres(ctx)
    tlas(ctx)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
