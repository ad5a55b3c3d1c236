"""Animated sphere sets (DESIGN.md par. 12, profiles/r11_sphere_anim.txt): what a frame of moving spheres costs, and what the trees trace at.
Two sets: the anim demo's bunny as spheres (69 630, tests/golden/meshes/bunny.npz) and a seeded uniform cloud of 1 000 000 spheres, r in
[0.002, 0.01] of the extent.
 (a) the per-frame path without the device builder: tbvh_host_build_custom_spheres + tbvh_upload_custom_spheres, wall clock;
 (b) the device calls: LBVH build, PLOC build, rebuild in place, refit — tbvh_time_last_ms (device) and wall clock, host-resident and
     device-resident spheres;
 (c) trace rates, camera and incoherent batches of 2^22 rays, of the host SAH tree, LBVH with 1 / 2 / 4 spheres per leaf, PLOC, and an LBVH
     tree refitted through 30 frames of motion (beside a fresh LBVH build over the same moved spheres).
Every figure: one warm-up, then the median of --reps repetitions with the spread (min .. max).
usage: python tools/sphere_anim_bench.py [--sets bunny,cloud] [--reps R] [--rays N] [--out FILE]"""
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

OUT = []


def say(line):
    print(line, flush=True)
    OUT.append(line)


def spread(v):
    v = np.array(v, np.float64)
    return f"{np.median(v):9.3f}  ({v.min():.3f} .. {v.max():.3f})"


def sphere_set(name):
    if name == "bunny":
        return cl.sphere_set("bunny")
    rng = np.random.default_rng(21)
    s = np.empty((1_000_000, 4), np.float32)
    s[:, :3] = rng.uniform(-10, 10, (s.shape[0], 3))
    s[:, 3] = rng.uniform(0.002, 0.01, s.shape[0]) * 20.0
    return s


def ray_batches(sph, n):
    lo, hi = sph[:, :3].min(0), sph[:, :3].max(0)
    rng = np.random.default_rng(9)
    c, ext = (lo + hi) * 0.5, float((hi - lo).max())
    eye = (c + np.array([0.2, 0.35, 1.6], np.float32) * ext).astype(np.float32)
    tgt = c + rng.uniform(-0.45, 0.45, (n, 3)).astype(np.float32) * (hi - lo)
    cam = tb.make_rays(np.broadcast_to(eye, (n, 3)), tgt - eye)
    inc = tb.make_rays((lo + rng.random((n, 3)).astype(np.float32) * (hi - lo)).astype(np.float32), rng.normal(size=(n, 3)).astype(np.float32))
    return {"camera": cam, "incoherent": inc}


def timed_call(ctx, fn, reps):
    """(device ms, wall ms) per repetition after one warm-up; the calls return when the device is done"""
    dev, wall = [], []
    for k in range(reps + 1):
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        if k:
            dev.append(ctx.time_last_ms()); wall.append((t1 - t0) * 1e3)
    return dev, wall


def trace(ctx, scene, label, d_rays, batches, reps):
    for kind, rays in batches.items():
        n = rays.shape[0]
        ctx.to_device(d_rays, rays)
        ms = []
        for k in range(reps + 1):
            scene.intersect_device_fresh(d_rays, n, 1e30); ctx.synchronize()
            if k:
                ms.append(ctx.time_last_ms())
        ms = np.array(ms)
        say(f"  (c) {label:34s} {kind:10s} {n / np.median(ms) / 1e6:7.3f} G rays/s  ({n / ms.max() / 1e6:.3f} .. {n / ms.min() / 1e6:.3f})")


def run_set(ctx, name, reps, n_rays):
    sph = sphere_set(name)
    n = sph.shape[0]
    say(f"== {name}: {n} spheres ==")
    # (a) host build + upload per frame
    host_reps = reps if n < 200_000 else max(1, reps // 3)
    build_ms, up_ms = [], []
    nodes = pi = None
    for k in range(host_reps + 1):
        t0 = time.perf_counter()
        nodes, pi = tb.host_build_custom_spheres(sph)
        t1 = time.perf_counter()
        s = tb.SphereBVH(ctx).Upload(nodes, pi, sph); ctx.synchronize()
        t2 = time.perf_counter()
        if k:
            build_ms.append((t1 - t0) * 1e3); up_ms.append((t2 - t1) * 1e3)
        if k < host_reps:
            s.free()
    sah = s
    say(f"  (a) host build (binned SAH, one thread)   wall ms {spread(build_ms)}   [{host_reps} repetitions]")
    say(f"  (a) upload (validate, gather, copy)       wall ms {spread(up_ms)}")
    say(f"  (a) host build + upload                   wall ms {spread(np.array(build_ms) + np.array(up_ms))}")
    # (b) the device calls
    d_sph = ctx.malloc(sph.nbytes)
    ctx.to_device(d_sph, sph)
    holder = {}

    def build(kind, src, **kw):
        if holder.get("s") is not None:
            holder["s"].free()
        holder["s"] = tb.SphereBVH(ctx).BuildOnDevice(src, **kw)

    for label, kw in (("LBVH build, 1 per leaf", dict(builder="lbvh")), ("PLOC build, radius 16", dict(builder="ploc"))):
        for where, src in (("host spheres", sph), ("device spheres", (d_sph, n))):
            dev, wall = timed_call(ctx, lambda: build(label, src, **kw), reps)
            say(f"  (b) {label:24s} {where:15s} device ms {spread(dev)}   wall ms {spread(wall)}")
    build("lbvh", sph, builder="lbvh")
    s = holder["s"]
    for label, fn in (("rebuild in place (LBVH)", s.RebuildOnDevice), ("refit", s.Refit)):
        for where, src in (("host spheres", sph), ("device spheres", (d_sph, n))):
            dev, wall = timed_call(ctx, lambda: fn(src), reps)
            say(f"  (b) {label:24s} {where:15s} device ms {spread(dev)}   wall ms {spread(wall)}")
    # (c) trace rates
    batches = ray_batches(sph, n_rays)
    d_rays = ctx.malloc(n_rays * 64)
    trace(ctx, sah, "host SAH tree", d_rays, batches, reps)
    sah.free()
    for label, kw in (("LBVH, 1 per leaf", dict(max_leaf=1)), ("LBVH, 2 per leaf", dict(max_leaf=2)), ("LBVH, 4 per leaf", dict(max_leaf=4)),
                      ("PLOC, radius 16", dict(builder="ploc"))):
        build(label, (d_sph, n), **kw)
        trace(ctx, holder["s"], label, d_rays, batches, reps)
    # 30 frames of motion: every sphere drifts by a seeded velocity of up to 0.3 % of the extent per frame
    build("lbvh", (d_sph, n), builder="lbvh")
    s = holder["s"]
    rng = np.random.default_rng(33)
    ext = float((sph[:, :3].max(0) - sph[:, :3].min(0)).max())
    vel = rng.uniform(-0.003, 0.003, (n, 3)).astype(np.float32) * np.float32(ext)
    moved = sph.copy()
    for _ in range(30):
        moved[:, :3] += vel
        s.Refit(moved)
    trace(ctx, s, "LBVH refitted through 30 frames", d_rays, batches, reps)
    s.RebuildOnDevice(moved)
    trace(ctx, s, "LBVH rebuilt over the same spheres", d_rays, batches, reps)
    s.free(); holder["s"] = None
    ctx.free(d_rays); ctx.free(d_sph)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="bunny,cloud")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rays", type=int, default=1 << 22)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = tb.Context(0)
    say(f"sphere_anim_bench: {a.reps} repetitions after one warm-up, median (min .. max); rates over {a.rays} rays")
    for name in a.sets.split(","):
        run_set(ctx, name, a.reps, a.rays)
        if a.out:   # (kept current set by set)
            with open(a.out, "w") as f:
                f.write("\n".join(OUT) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
