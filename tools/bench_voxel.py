"""Traversal rate of VoxelSet scenes (kernels_voxel.hip): GRays/s from the HIP-event kernel time (Context.time_last_ms), best of a few launches.

    python tools/bench_voxel.py [--reps 5] [--rays 16777216] [--out profiles/r08_voxel.txt]

Scenes: the reference's legocar (128^3 voxels in the 256^3 object), a procedural 256^3 heightfield terrain, and a TLAS of 1000 instances of
legocar / rock / terrain (rotated about y, scaled 1-4, on a 60 x 60 field).  Rays: camera rays made on the device (tbvh_generate_primary_device,
4 x 4 samples per pixel) and incoherent rays (origins in and around the scene's box, uniform directions).  Closest hits through
tbvh_intersect_device_fresh (every launch starts from tmax = 1e30), any-hit queries through tbvh_occluded_device."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tinybvh_amd as tb  # noqa: E402
from tinybvh_amd import rays as R  # noqa: E402
import voxel_lib as V  # noqa: E402


def best_ms(ctx, launch, reps):
    ts = []
    for _ in range(reps):
        launch()
        ctx.synchronize()
        ts.append(ctx.time_last_ms())
    return min(ts)


def hit_fraction(ctx, d, n):
    """share of the n records at d with a hit (every record read back)"""
    hits = np.zeros(n, tb.RAY_DTYPE)
    ctx.from_device(hits, d)
    return float((hits["t"] < 1e29).mean())


def incoherent(n, lo, hi, seed):
    rng = np.random.default_rng(seed)
    lo = np.asarray(lo, np.float32); hi = np.asarray(hi, np.float32)
    c, ext = (lo + hi) / 2, (hi - lo)
    O = (c + (rng.random((n, 3), dtype=np.float32) - np.float32(0.5)) * ext * np.float32(1.5)).astype(np.float32)
    D = rng.standard_normal((n, 3), dtype=np.float32)
    return tb.make_rays(O, D)


def tlas_instances(n, seed, n_sets):
    rng = np.random.default_rng(seed)
    T = np.zeros((n, 4, 4), np.float32)
    ang = rng.uniform(0, 2 * np.pi, n)
    sc = rng.uniform(1, 4, n)
    T[:, 0, 0] = np.cos(ang) * sc; T[:, 0, 2] = np.sin(ang) * sc
    T[:, 1, 1] = sc
    T[:, 2, 0] = -np.sin(ang) * sc; T[:, 2, 2] = np.cos(ang) * sc
    T[:, 0, 3] = rng.uniform(-30, 30, n); T[:, 2, 3] = rng.uniform(-30, 30, n); T[:, 1, 3] = rng.uniform(-1, 1, n)
    T[:, 3, 3] = 1
    return tb.make_instances(T, rng.integers(0, n_sets, n).astype(np.uint32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rays", type=int, default=1 << 24)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n = a.rays
    ctx = tb.Context(0)
    ctx.set_timing(True)
    lego, rock, terrain = (V.scene_dense(k) for k in ("legocar", "rock", "terrain"))
    sets = {"legocar": tb.VoxelSet(ctx).Build(lego), "terrain": tb.VoxelSet(ctx).Build(terrain)}
    rock_set = tb.VoxelSet(ctx).Build(rock)
    inst = tlas_instances(1000, 3, 3)
    tlas = tb.TLAS(ctx).Build(inst, [sets["legocar"], rock_set, sets["terrain"]])
    cases = [
        ("legocar", sets["legocar"], ((0.55, 0.35, -0.1), (-0.302, -0.102, 0.346)), ((0, 0, 0), (0.5, 0.5, 0.5))),
        ("terrain 256^3", sets["terrain"], ((0.5, 1.2, -0.6), (0.0, -0.7, 1.0)), ((0, 0, 0), (1, 1, 1))),
        ("TLAS 1000 inst", tlas, ((0, 12, -45), (0.0, -0.3, 1.0)), ((-34, -1, -34), (34, 4, 34))),
    ]
    side = int(np.sqrt(n / 16))
    side -= side % 4
    cam_n = side * side * 16
    d = ctx.malloc(max(n, cam_n) * 64); dout = ctx.malloc(max(n, cam_n))
    rows = []
    try:
        for name, sc, (eye, view), (lo, hi) in cases:
            cam = R.camera(eye, view, side, side, 4, 4)
            ctx.generate_primary(cam, d, 0, cam_n)
            ctx.synchronize()
            ms_c = best_ms(ctx, lambda: sc.intersect_device_fresh(d, cam_n, 1e30), a.reps)
            hit_frac = hit_fraction(ctx, d, cam_n)
            ctx.generate_primary(cam, d, 0, cam_n)
            ms_ca = best_ms(ctx, lambda: sc.occluded_device(d, cam_n, dout), a.reps)
            rays = incoherent(n, lo, hi, 7)
            ctx.to_device(d, rays)
            ctx.synchronize()
            ms_i = best_ms(ctx, lambda: sc.intersect_device_fresh(d, n, 1e30), a.reps)
            hit_frac_i = hit_fraction(ctx, d, n)
            ctx.to_device(d, rays)
            ms_ia = best_ms(ctx, lambda: sc.occluded_device(d, n, dout), a.reps)
            del rays
            for rk, cnt, ms_closest, ms_any in (("camera", cam_n, ms_c, ms_ca), ("incoherent", n, ms_i, ms_ia)):
                rows.append({"scene": name, "rays": rk, "n": cnt, "closest_ms": round(ms_closest, 3), "closest_grays": round(cnt / ms_closest / 1e6, 3),
                             "any_ms": round(ms_any, 3), "any_grays": round(cnt / ms_any / 1e6, 3),
                             "hit_fraction": round(hit_frac if rk == "camera" else hit_frac_i, 3)})
    finally:
        ctx.free(d); ctx.free(dout)
    lines = [f"{'scene':<16} {'rays':<11} {'n':>9} {'hit':>6} {'closest GRays/s':>16} {'any-hit GRays/s':>16}"]
    for r in rows:
        lines.append(f"{r['scene']:<16} {r['rays']:<11} {r['n']:>9} {r['hit_fraction']:>6.3f} {r['closest_grays']:>16.3f} {r['any_grays']:>16.3f}")
    text = "\n".join(lines)
    print(text)
    print(json.dumps(rows))
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n" + json.dumps(rows) + "\n")


if __name__ == "__main__":
    main()
