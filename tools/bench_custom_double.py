"""fp64 custom-geometry (sphere BLAS) rates for DESIGN.md par. 9 / profiles/custom_double.txt (the sphere forms of kernels_double.hip).
Two sphere sets: the bunny as spheres (69 630, tests/golden/meshes/bunny.npz, the demos' recipe) and a soup of 1 M spheres; camera, shadow and diffuse
batches; a single BLAS, and 1000 instances under a TLAS_Double.  Each next to the fp64 triangle BVH_Double of the same primitive count and to the
fp32 SphereBVH of the same set (context: other arithmetic, the same geometry).  M rays/s from Context.time_last_ms: one warm-up, then the median
of --reps launches with the spread; the records go up again before every closest-hit launch (a traced record carries its hit distance).  Then a
device rebuild per frame against host build + upload + free, wall clock.
usage: python tools/bench_custom_double.py [--rays N] [--reps R] [--out profiles/custom_double.txt]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import custom_lib as cl  # noqa: E402
import tinybvh_amd as tb  # noqa: E402
from tinybvh_amd import scenes  # noqa: E402

OUT = []


def say(line):
    print(line, flush=True)
    OUT.append(line)


def batches(lo, hi, n, seed):
    """(O, D, tmax) per kind: camera rays from outside the box, shadow rays towards a light above, diffuse rays from inside the box"""
    rng = np.random.default_rng(seed)
    c, ext = (lo + hi) * 0.5, float((hi - lo).max())
    eye = c + np.array([0.15, 0.3, 0.9]) * ext
    tgt = c + rng.uniform(-0.5, 0.5, (n, 3)) * (hi - lo)
    P = lo + rng.random((n, 3)) * (hi - lo)
    light = c + np.array([0, 0.6, 0]) * ext
    return {"camera": (np.broadcast_to(eye, (n, 3)), tgt - eye, None), "shadow": (P, light - P, np.sqrt(((light - P) ** 2).sum(1))),
            "diffuse": (P, rng.normal(size=(n, 3)), None)}


def run(ctx, scene, label, kinds, reps, fp32=False):
    for kind, (O, D, tmax) in kinds.items():
        if fp32:
            rays = tb.make_rays(O.astype(np.float32), D.astype(np.float32))
            if tmax is not None:
                rays["t"] = tmax.astype(np.float32)
        else:
            rays = tb.make_rays_ex(O, D)
            if tmax is not None:
                rays["t"] = tmax
        n = rays.shape[0]
        d = ctx.malloc(rays.nbytes); o = ctx.malloc(n)
        try:
            ms = []
            for _ in range(reps + 1):
                ctx.to_device(d, rays)
                if kind == "shadow":
                    scene.occluded_device(d, n, o)
                else:
                    scene.intersect_device(d, n)
                ctx.synchronize()
                ms.append(ctx.time_last_ms())
            ms = np.array(ms[1:])
            say(f"{label:58s} {kind:8s} {n / np.median(ms) / 1e3:8.1f} M rays/s  (median of {reps}; {n / ms.max() / 1e3:.1f} .. {n / ms.min() / 1e3:.1f})")
        finally:
            ctx.free(d); ctx.free(o)


def frame_times(ctx, sph, reps):
    """wall ms per frame, median of reps after one warm-up: (a) host build + upload + free, (b) rebuild from host spheres, (c) from device spheres"""
    def wall(fn):
        t = []
        for _ in range(reps + 1):
            t0 = time.perf_counter(); fn(); ctx.synchronize(); t.append((time.perf_counter() - t0) * 1e3)
        t = np.array(t[1:])
        return f"{np.median(t):.3f} ({t.min():.3f} .. {t.max():.3f})"

    def a():
        tb.SphereBVH_Double(ctx).Build(sph).free()
    sc = tb.SphereBVH_Double(ctx).BuildOnDevice(sph)
    d = ctx.malloc(sph.nbytes)
    ctx.to_device(d, sph)
    try:
        say(f"frame, {sph.shape[0]} spheres, wall ms, median of {reps} (min .. max): host build + upload + free {wall(a)}; "
            f"device rebuild from host spheres {wall(lambda: sc.RebuildOnDevice(sph))}; from device spheres {wall(lambda: sc.RebuildOnDevice((d, sph.shape[0])))}")
    finally:
        ctx.free(d); sc.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 21)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = tb.Context(0)
    rng = np.random.default_rng(3)
    bunny = cl.bunny_verts()
    soup_sph = np.concatenate([rng.uniform(-50, 50, (1_000_000, 3)), rng.uniform(0.05, 0.5, (1_000_000, 1))], 1)
    sets = {"bunny": (cl.spheres_from_tris(bunny, 1.2, 0.55).astype(np.float64), bunny[:, :3].astype(np.float64)),
            "soup": (soup_sph, scenes.soup(1_000_000, seed=5, extent=100.0, size=0.7)[:, :3].astype(np.float64) - 50.0)}
    for name, (sph, verts) in sets.items():
        lo, hi = (sph[:, :3] - sph[:, 3:4]).min(0), (sph[:, :3] + sph[:, 3:4]).max(0)
        kinds = batches(lo, hi, a.rays, 7)
        s = tb.SphereBVH_Double(ctx).Build(sph)
        run(ctx, s, f"{name}: {sph.shape[0]} spheres, SphereBVH_Double (host tree)", kinds, a.reps)
        dv = tb.SphereBVH_Double(ctx).BuildOnDevice(sph)
        run(ctx, dv, f"{name}: {sph.shape[0]} spheres, SphereBVH_Double (device LBVH)", kinds, a.reps)
        dv.free()
        t = tb.BVH_Double(ctx).Build(verts)
        run(ctx, t, f"{name}: {verts.shape[0] // 3} triangles, BVH_Double", kinds, a.reps)
        s32 = tb.SphereBVH(ctx).Build(sph.astype(np.float32))
        run(ctx, s32, f"{name}: {sph.shape[0]} spheres, fp32 SphereBVH", kinds, a.reps, fp32=True)
        s32.free()
        # 1000 instances on a 10 x 10 x 10 grid, scaled to fit their cells
        ext = float((hi - lo).max())
        T = np.tile(np.eye(4), (1000, 1, 1))
        g = np.arange(10) * ext
        T[:, :3, :3] *= 0.6
        T[:, :3, 3] = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
        tk = batches(np.zeros(3) + lo * 0.6, g[-1] + hi * 0.6, a.rays, 9)
        for label, blas in ((f"{name}: TLAS_Double, 1000 sphere instances", s), (f"{name}: TLAS_Double, 1000 triangle instances", t)):
            tl = tb.TLAS_Double(ctx).Build(tb.make_instances_ex(T, 0), [blas])
            run(ctx, tl, label, tk, a.reps)
            tl.free()
        s.free(); t.free()
        frame_times(ctx, sph, a.reps)
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
