"""fp64 traversal rate of BVH_DOUBLE scenes (tbvh_intersect_ex_device) next to the library's native BVH_GPU kernel (tbvh_set_variant(scene, 1))
on the same scenes and rays: MRays/s from the HIP-event kernel time (Context.time_last_ms), best of a few launches.

    python tools/bench_double.py [--reps 5] [--out profiles/r07_double.txt]

Scenes: the atrium stand-in (262 k triangles) and the street stand-in (2.83 M); rays: camera rays (one per pixel, 1920 x 1080) and one diffuse
bounce from their hits.  The fp32 kernel traces the rays in float (float-exact vertices: the scenes are generated in float)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import tinybvh_amd as tb  # noqa: E402
from tinybvh_amd import rays as R, scenes  # noqa: E402


def best_ms(ctx, launch, reps):
    ts = []
    for _ in range(reps):
        launch()
        ts.append(ctx.time_last_ms())
    return min(ts)


def run_fp64(ctx, sc, rays, reps):
    d = ctx.malloc(rays.nbytes)
    try:
        def launch():
            ctx.to_device(d, rays)   # (every launch starts from the untraced records: a traced record's shorter hit.t would speed the next one up)
            sc.intersect_device(d, rays.shape[0])
        ms = best_ms(ctx, launch, reps)
        out = np.zeros_like(rays)
        ctx.from_device(out, d)
    finally:
        ctx.free(d)
    return ms, out


def run_fp32(ctx, sc, rays, reps):
    d = ctx.malloc(rays.nbytes)
    try:
        ctx.to_device(d, rays)
        ms = best_ms(ctx, lambda: sc.intersect_device_fresh(d, rays.shape[0], 1e30), reps)
        out = np.zeros_like(rays)
        ctx.from_device(out, d)
    finally:
        ctx.free(d)
    return ms, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    ctx = tb.Context(0)
    lines = [f"# fp64 BVH_DOUBLE (tbvh_intersect_ex_device) vs fp32 BVH_GPU native (variant 1), {a.width} x {a.height} rays, best of {a.reps}; MRays/s",
             f"{'scene':<10} {'tris':>9} {'rays':<8} {'fp64 ms':>9} {'fp64 MR/s':>10} {'fp32 ms':>9} {'fp32 MR/s':>10} {'fp32/fp64':>9}"]
    print(lines[0]); print(lines[1])
    agree = []
    for name, gen, cams in (("atrium", lambda: scenes.atrium(262_267, seed=1), scenes.SPONZA_CAMERAS), ("street", lambda: scenes.street(2_832_120, seed=2), scenes.STREET_CAMERAS)):
        v32 = gen()
        v64 = np.ascontiguousarray(v32[:, :3], np.float64)
        d = tb.BVH_Double(ctx).Build(v64)
        g = tb.BVH_GPU(ctx).Build(v32)
        g.set_variant(1)
        eye, view = cams[0]
        cam32 = R.primary(R.camera(eye, view, a.width, a.height, 1, 1))
        cam64 = tb.make_rays_ex(cam32["O"].astype(np.float64), cam32["D"].astype(np.float64))
        ms64, traced = run_fp64(ctx, d, cam64, a.reps)
        ms32, traced32 = run_fp32(ctx, g, cam32, a.reps)
        h32, h64 = traced32["t"] < 1e29, traced["t"] < 1e299
        differ = int(((h32 != h64) | (h32 & h64 & (traced32["prim"].astype(np.uint64) != traced["prim"]))).sum())
        agree.append(f"{name}: camera rays whose hit / triangle differ between fp64 and fp32 BVH_GPU: {differ} of {cam64.shape[0]}")
        # one diffuse bounce from the fp64 hits (the same rays for both kernels: directions and origins rounded to float for BVH_GPU)
        rng = np.random.default_rng(5)
        hit = traced["t"] < 1e299
        I = traced["O"] + np.where(hit, traced["t"], 20.0)[:, None] * traced["D"]
        Dn = rng.normal(size=I.shape)
        Dn = np.where(((Dn * traced["D"]).sum(1) > 0)[:, None], -Dn, Dn)
        Dn /= np.linalg.norm(Dn, axis=1, keepdims=True)
        O = I + 1e-3 * Dn
        dif64 = tb.make_rays_ex(O, Dn)
        dif32 = tb.make_rays(O.astype(np.float32), Dn.astype(np.float32))
        ms64d, _ = run_fp64(ctx, d, dif64, a.reps)
        ms32d, _ = run_fp32(ctx, g, dif32, a.reps)
        n = cam64.shape[0]
        for kind, m64, m32 in (("camera", ms64, ms32), ("diffuse", ms64d, ms32d)):
            line = f"{name:<10} {v32.shape[0] // 3:>9} {kind:<8} {m64:>9.3f} {n / m64 / 1e3:>10.1f} {m32:>9.3f} {n / m32 / 1e3:>10.1f} {m64 / m32:>9.2f}"
            print(line, flush=True)
            lines.append(line)
        d.free(); g.free()
    ctx.close()
    for line in agree:
        print(line)
    lines += agree
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
