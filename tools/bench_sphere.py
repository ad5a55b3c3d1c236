"""Sphere-overlap query rates (tbvh_intersect_spheres_device, kernels_sphere.hip) for DESIGN.md par. 11 / profiles/r09_sphere.txt.
For bunny (tests/golden/meshes/bunny.npz) and the bench's street stand-in (scenes.street()), in all three layouts: G spheres/s from
Context.time_last_ms (best of a few launches) for small (~ one triangle) and large radii, spatially coherent (a particle cloud sorted
into 3-D cells) and random centres, with the hit fraction; beside them the same scene's any-hit ray rate; and the restatement
(tests/oracle_sphere.c) on 16 CPU threads as a CPU baseline (the reference itself is not on the GPU machine).
usage: python tools/bench_sphere.py [--spheres N] [--reps R] [--scenes bunny,street]"""
import argparse
import os
import sys
import tempfile
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sphere_lib as sl  # noqa: E402
import tinybvh_amd as tb  # noqa: E402
from tinybvh_amd import scenes  # noqa: E402


def sphere_set(verts, n, radius, coherent, seed):
    """centres on / near the surface (a particle cloud: high hit fractions) or, with coherent = None, uniform over the scene box (low hit
    fractions); coherent = sorted by 3-D cell (64^3 over the scene box), else in random order"""
    rng = np.random.default_rng(seed)
    t = verts.reshape(-1, 3, 4)[:, :, :3]
    k = rng.integers(0, t.shape[0], n)
    w = rng.dirichlet(np.ones(3), n).astype(np.float32)
    lo, hi = verts[:, :3].min(0), verts[:, :3].max(0)
    p = (t[k] * w[:, :, None]).sum(1) + rng.normal(0, 1, (n, 3)).astype(np.float32) * np.float32(2.0 * radius)
    if coherent is None:
        p = (lo + rng.random((n, 3)) * (hi - lo)).astype(np.float32)
    elif coherent:
        c = np.clip(((p - lo) / (hi - lo) * 63.999).astype(np.int64), 0, 63)
        p = p[np.argsort((c[:, 2] * 64 + c[:, 1]) * 64 + c[:, 0], kind="stable")]
    return np.ascontiguousarray(np.concatenate([p, np.full((n, 1), radius, np.float32)], 1), np.float32)


def gpu_rate(ctx, sc, sp, verts, reps):
    d_sp, d_v, d_hit = ctx.malloc(sp.nbytes), ctx.malloc(verts.nbytes), ctx.malloc(sp.shape[0])
    try:
        ctx.to_device(d_sp, sp); ctx.to_device(d_v, verts)
        best = 1e30
        for _ in range(reps + 1):
            sc.intersect_spheres_device(d_sp, sp.shape[0], d_v, verts.shape[0] // 3, d_hit)
            ctx.synchronize()
            best = min(best, ctx.time_last_ms())
        hit = np.zeros(sp.shape[0], np.uint8)
        ctx.from_device(hit, d_hit)
    finally:
        for p in (d_sp, d_v, d_hit):
            ctx.free(p)
    return sp.shape[0] / best / 1e6, float(hit.mean())   # (G spheres/s: best is in ms)


def ray_rate(ctx, sc, verts, n, reps):
    rng = np.random.default_rng(5)
    lo, hi = verts[:, :3].min(0), verts[:, :3].max(0)
    O = (lo + rng.random((n, 3)) * (hi - lo)).astype(np.float32)
    rays = tb.make_rays(O, rng.normal(size=(n, 3)).astype(np.float32))
    d_r, d_o = ctx.malloc(rays.nbytes), ctx.malloc(n)
    try:
        ctx.to_device(d_r, rays)
        best = 1e30
        for _ in range(reps + 1):
            sc.occluded_device(d_r, n, d_o)
            ctx.synchronize()
            best = min(best, ctx.time_last_ms())
    finally:
        ctx.free(d_r); ctx.free(d_o)
    return n / best / 1e6   # G rays/s


def cpu_rate(orc, layout, blobs, verts, sp, threads=16):
    """the restatement of the same layout on `threads` threads (ctypes releases the GIL)"""
    parts = np.array_split(sp, threads)
    outs = [None] * threads

    def run(i):
        outs[i] = orc.layout(layout, blobs, verts, parts[i])

    t0 = time.perf_counter()
    th = [threading.Thread(target=run, args=(i,)) for i in range(threads)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    return sp.shape[0] / (time.perf_counter() - t0) / 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spheres", type=int, default=1 << 22)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scenes", default="bunny,street")
    ap.add_argument("--cpu-spheres", type=int, default=1 << 16)
    a = ap.parse_args()
    orc = sl.compile_oracle(tempfile.mkdtemp())
    ctx = tb.Context(0)
    print(f"# spheres per launch {a.spheres}, best of {a.reps}; GPU in G spheres/s (kernel time), CPU = the restatement on 16 threads in M spheres/s")
    for name in a.scenes.split(","):
        verts = sl.bunny() if name == "bunny" else scenes.street()
        t = verts.reshape(-1, 3, 4)[:, :, :3]
        edge = float(np.median(np.linalg.norm(t[:, 1] - t[:, 0], axis=1)))
        for layout in (tb.LAYOUT_BVH_GPU, tb.LAYOUT_BVH4_GPU, tb.LAYOUT_CWBVH):
            sc = tb.LAYOUT_CLASSES[layout](ctx).Build(verts)
            hb = sc.host
            blobs = ([hb.blob(0, np.uint32, 16), hb.blob(1, np.uint32, 1).reshape(-1)] if layout == tb.LAYOUT_BVH_GPU else
                     [hb.blob(0, np.uint32, 4)] if layout == tb.LAYOUT_BVH4_GPU else [hb.blob(0, np.uint32, 4), hb.blob(1, np.uint32, 4)])
            rays = ray_rate(ctx, sc, verts, a.spheres, a.reps)
            print(f"{name:7s} {verts.shape[0] // 3:8d} tris  layout {layout:2d}  any-hit rays (random origins and directions) {rays:6.2f} G/s")
            for rname, radius in (("small", edge), ("large", 10 * edge)):
                for coherent in (True, False, None):
                    sp = sphere_set(verts, a.spheres, radius, coherent, seed=11)
                    rate, frac = gpu_rate(ctx, sc, sp, verts, a.reps)
                    cpu = cpu_rate(orc, layout, blobs, verts, sp[: a.cpu_spheres])
                    print(f"    r = {radius:9.5f} ({rname})  {'coherent' if coherent else 'random  ' if coherent is not None else 'uniform '}  GPU {rate:6.2f} G/s  hit fraction {frac:5.3f}"
                          f"  CPU {cpu:7.2f} M/s  x{rate * 1000 / cpu:6.0f}")
            sc.free()
    ctx.close()


if __name__ == "__main__":
    main()
