"""Custom-geometry sphere BLAS rates (kernels_custom.hip, the sphere step of kernels_tlas.hip) for DESIGN.md par. 12 / profiles/r10_custom.txt.
Two sphere BLASes: the bunny as spheres (tiny_bvh_anim.cpp's, tests/golden/meshes/bunny.npz) and the Bistro stand-in (scenes.street()) as one
sphere per triangle (tiny_bvh_custom.cpp's recipe); per scene camera, shadow and diffuse batches of 16.7 M rays, G rays/s from
Context.time_last_ms (median and spread over --reps launches), beside the library's BVH_GPU triangle query on the same mesh (context only:
different geometry, different hits).  Then the anim-like TLAS: 1000 scaled bunny-sphere instances plus one triangle BLAS (the Sponza
stand-in) in each triangle layout, and the spheres alone.
usage: python tools/bench_custom.py [--rays N] [--reps R] [--scenes bunny,bistro]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import custom_lib as cl  # noqa: E402
import tinybvh_amd as tb  # noqa: E402
from tinybvh_amd import scenes  # noqa: E402


def timed(ctx, fn, reps):
    ms = []
    for _ in range(reps + 1):
        fn(); ctx.synchronize()
        ms.append(ctx.time_last_ms())
    ms = np.array(ms[1:])
    return float(np.median(ms)), float(ms.min()), float(ms.max())


def batches(lo, hi, n, seed):
    """camera rays from outside the box, diffuse rays (origins in the box, random directions), shadow rays (towards a light above)"""
    rng = np.random.default_rng(seed)
    c, ext = (lo + hi) * 0.5, float((hi - lo).max())
    eye = (c + np.array([0.15, 0.3, 0.9], np.float32) * ext).astype(np.float32)
    tgt = c + rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32) * (hi - lo)
    cam = tb.make_rays(np.broadcast_to(eye, (n, 3)), tgt - eye)
    P = (lo + rng.random((n, 3)).astype(np.float32) * (hi - lo)).astype(np.float32)
    dif = tb.make_rays(P, rng.normal(size=(n, 3)).astype(np.float32))
    light = (c + np.array([0, 0.6, 0], np.float32) * ext).astype(np.float32)
    sh = tb.make_rays(P, light - P)
    sh["t"] = np.sqrt(((light - P) ** 2).sum(1)).astype(np.float32)
    return {"camera": cam, "shadow": sh, "diffuse": dif}


def run_scene(ctx, scene, label, rays_by_kind, reps, out):
    d = ctx.malloc(next(iter(rays_by_kind.values())).nbytes)
    o = ctx.malloc(next(iter(rays_by_kind.values())).shape[0])
    try:
        for kind, rays in rays_by_kind.items():
            n = rays.shape[0]
            ctx.to_device(d, rays)
            if kind == "shadow":
                med, lo, hi = timed(ctx, lambda: scene.occluded_device(d, n, o), reps)
            else:   # the fresh variant: every launch starts from tmax = 1e30, whatever the previous one left in the records
                med, lo, hi = timed(ctx, lambda: scene.intersect_device_fresh(d, n, 1e30), reps)
            line = f"{label:44s} {kind:8s} {n / med / 1e6:7.3f} G rays/s  (median of {reps}; {n / hi / 1e6:.3f} .. {n / lo / 1e6:.3f})"
            print(line, flush=True)
            out.append(line)
    finally:
        ctx.free(d); ctx.free(o)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scenes", default="bunny,bistro")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = tb.Context(0)
    out = []
    for name in a.scenes.split(","):
        verts = cl.bunny_verts() if name == "bunny" else scenes.street()
        sph = cl.spheres_from_tris(verts, 1.2, 0.55) if name == "bunny" else cl.spheres_from_tris(verts, 0.35, 0.25)
        lo, hi = verts[:, :3].min(0), verts[:, :3].max(0)
        rays = batches(lo, hi, a.rays, 7)
        s = tb.SphereBVH(ctx).Build(sph)
        run_scene(ctx, s, f"{name}: {sph.shape[0]} spheres (SphereBVH)", rays, a.reps, out)
        s.free()
        t = tb.BVH_GPU(ctx).Build(verts)
        run_scene(ctx, t, f"{name}: {verts.shape[0] // 3} triangles (BVH_GPU)", rays, a.reps, out)
        t.free()
    # the anim-like TLAS: 1000 bunny-sphere instances (10^3 grid, scale 0.6 as tiny_bvh_anim.cpp) + the Sponza stand-in
    sph = cl.spheres_from_tris(cl.bunny_verts(), 1.2, 0.55)
    tris = scenes.atrium()
    g = np.arange(10, dtype=np.float32) * np.float32(5) - np.float32(25)
    xf = np.zeros((1001, 4, 4), np.float32)
    k = 0
    for x in g:
        for y in g:
            for z in g:
                xf[k] = np.eye(4, dtype=np.float32) * np.float32(0.6); xf[k, 3, 3] = 1; xf[k, :3, 3] = [x, y + 7, z + 1]; k += 1
    xf[1000] = np.eye(4, dtype=np.float32)
    lo, hi = np.array([-30, -20, -30], np.float32), np.array([30, 40, 30], np.float32)
    rays = batches(lo, hi, a.rays, 9)
    s = tb.SphereBVH(ctx).Build(sph)
    inst = tb.make_instances(xf[:1000], [0] * 1000)
    tl = tb.TLAS(ctx).Build(inst, [s])
    run_scene(ctx, tl, "TLAS: 1000 sphere instances", rays, a.reps, out)
    tl.free()
    for layout in (tb.LAYOUT_BVH_GPU, tb.LAYOUT_BVH4_GPU, tb.LAYOUT_CWBVH):
        t = tb.LAYOUT_CLASSES[layout](ctx).Build(tris)
        inst = tb.make_instances(xf, [0] * 1000 + [1])
        tl = tb.TLAS(ctx).Build(inst, [s, t])
        run_scene(ctx, tl, f"TLAS: 1000 sphere inst. + atrium ({t.__class__.__name__})", rays, a.reps, out)
        tl.free()
        # what routing a TLAS through the flat loop costs its triangles: the triangle BLAS alone under a TLAS of one instance, through the
        # library's own two-level kernels, and the same instance next to one sphere instance no ray enters (mask 0), through the flat loop
        tl = tb.TLAS(ctx).Build(tb.make_instances(xf[1000:], [0]), [t])
        run_scene(ctx, tl, f"TLAS: atrium alone ({t.__class__.__name__}, k_tlas*)", rays, a.reps, out)
        tl.free()
        inst = tb.make_instances(xf[999:], [0, 1])
        inst["mask"][0] = 0
        tl = tb.TLAS(ctx).Build(inst, [s, t])
        run_scene(ctx, tl, f"TLAS: atrium + masked sphere ({t.__class__.__name__}, flat)", rays, a.reps, out)
        tl.free(); t.free()
    s.free()
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
