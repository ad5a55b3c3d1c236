"""A frame of a double-precision scene that moves (DESIGN.md par. 9, profiles/double_anim.txt), at 1000 and at 100 000 instances of three BLASes
around (1e6, -2e6, 3e6) (tests/double_lib.instance_scene's content, the cloud widened with the cube root of the count so the density stays):
 (a) the only route before the device rebuild: tbvh_host_build_tlas_double + tbvh_upload_tlas_double into a NEW scene + tbvh_free_scene of the old
     one; wall clock around the three calls, after a tbvh_synchronize;
 (b) tbvh_rebuild_tlas_double_device from host transforms and from device transforms: HIP-event time (tbvh_time_last_ms) and wall clock (call +
     tbvh_synchronize);
 (c) the Intersect rate of the same 2 M camera rays (device-resident RayEx records, re-uploaded before every launch) on the host-built (binned SAH)
     tree and on the device-built (LBVH) tree;
 (d) tbvh_refit_double on the 262 k-triangle atrium (host-staged and device-resident vertices) against a fresh tbvh_upload_bvh_double + free.
Every figure: one warm-up, then the best of --reps repetitions with the spread (min .. max).  The GPU should be otherwise idle.
usage: python tools/double_anim_bench.py [--counts 1000,100000] [--reps R] [--rays N] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tinybvh_amd as tb  # noqa: E402
from tinybvh_amd import scenes  # noqa: E402
from double_lib import instance_scene, to_dbl  # noqa: E402

OUT = []
CENTRE = np.array([1.0e6, -2.0e6, 3.0e6])


def say(line):
    print(line, flush=True)
    OUT.append(line)


def best(v):
    v = np.array(v, np.float64)
    return f"{v.min():10.3f}  ({v.min():.3f} .. {v.max():.3f})"


def wall_ms(ctx, fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


def instances(n, seed=3):
    """instance_scene's instances, vectorised: random rotation, scale 0.5 .. 2, offsets within +-half around CENTRE."""
    rng = np.random.default_rng(seed)
    half = 60.0 * (n / 500.0) ** (1.0 / 3.0)
    q = rng.normal(size=(n, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    Rm = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                   2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1).reshape(n, 3, 3)
    T = np.zeros((n, 4, 4))
    T[:, :3, :3] = Rm * rng.uniform(0.5, 2.0, n)[:, None, None]
    T[:, :3, 3] = CENTRE + rng.uniform(-half, half, (n, 3))
    T[:, 3, 3] = 1.0
    inst = tb.make_instances_ex(T, rng.integers(0, 3, n))
    return inst, T, half


def camera_rays(n_rays, half):
    w = 2048; h = max(n_rays // w, 1)
    u, v = np.meshgrid((np.arange(w) + 0.5) / w - 0.5, (np.arange(h) + 0.5) / h - 0.5)
    D = np.stack([u.reshape(-1) * 1.2, v.reshape(-1) * 0.8, np.ones(w * h)], 1)
    O = np.broadcast_to(CENTRE + np.array([0.0, 0.0, -2.5 * half]), D.shape)
    return tb.make_rays_ex(O, D)


def run_tlas(ctx, blas, bounds, n, reps, n_rays):
    inst, T, half = instances(n)
    say(f"== {n} instances of 3 BLASes, cloud +-{half:.0f} units around (1e6, -2e6, 3e6) ==")
    # (a)
    state = {"tl": tb.TLAS_Double(ctx).Build(inst.copy(), blas)}
    parts = {"build": [], "upload": [], "free": [], "frame": []}

    def host_frame(k):
        moved = inst.copy(); moved["transform"].reshape(-1, 4, 4)[:, :3, 3] += 0.01 * k
        ctx.synchronize()
        t0 = time.perf_counter()
        host = tb.host_build_tlas_double(moved, bounds)
        t1 = time.perf_counter()
        fresh = tb.TLAS_Double(ctx).Upload(host.nodes(), host.prim_idx(), moved, blas)
        t2 = time.perf_counter()
        state["tl"].free()
        t3 = time.perf_counter()
        state["tl"] = fresh; state["host"] = host
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t3 - t0) * 1e3

    for k in range(reps + 1):
        r = host_frame(k)
        if k:
            for key, val in zip(parts, r):
                parts[key].append(val)
    say(f"  (a) host build                      wall ms {best(parts['build'])}")
    say(f"  (a) upload into a new scene         wall ms {best(parts['upload'])}")
    say(f"  (a) free of the old scene           wall ms {best(parts['free'])}")
    say(f"  (a) frame                           wall ms {best(parts['frame'])}")
    a_frame = min(parts["frame"])
    # (c) on the host-built tree
    rays = camera_rays(n_rays, half)
    d_rays = ctx.malloc(rays.nbytes)

    def rate(tl):
        ms = []
        hits = 0
        for k in range(reps + 1):
            ctx.to_device(d_rays, rays)
            tl.intersect_device(d_rays, rays.shape[0])
            ctx.synchronize()
            if k:
                ms.append(ctx.time_last_ms())
        out = np.zeros_like(rays); ctx.from_device(out, d_rays)
        hits = int((out["t"] < 1e299).sum())
        return rays.shape[0] / (min(ms) * 1e3), ms, hits, out

    host_tl = state["tl"]
    mr_host, ms_host, hits_host, out_host = rate(host_tl)
    # (b) on a second scene with the same instances
    dev_tl = tb.TLAS_Double(ctx).Upload(state["host"].nodes(), state["host"].prim_idx(), host_tl.instances, blas)
    before = dev_tl.device_bytes
    dev_tl.RebuildOnDevice()
    ctx.synchronize()
    say(f"  device bytes of the TLAS: {before} as uploaded, {dev_tl.device_bytes} with room for 2 n - 1 nodes and the rebuild's scratch")
    T0 = np.ascontiguousarray(host_tl.instances["transform"].reshape(-1, 4, 4))
    d_T = ctx.malloc(T0.nbytes)
    ev_h, wall_h, ev_d, wall_d = [], [], [], []
    for k in range(reps + 1):
        Tk = T0.copy(); Tk[:, :3, 3] += 0.01 * k
        w = wall_ms(ctx, lambda: dev_tl.RebuildOnDevice(Tk))
        if k:
            wall_h.append(w); ev_h.append(ctx.time_last_ms())
    for k in range(reps + 1):
        ctx.to_device(d_T, T0)
        w = wall_ms(ctx, lambda: dev_tl.RebuildOnDevice(d_T, on_device=True))
        if k:
            wall_d.append(w); ev_d.append(ctx.time_last_ms())
    say(f"  (b) rebuild, host transforms        event ms {best(ev_h)}   wall ms {best(wall_h)}")
    say(f"  (b) rebuild, device transforms      event ms {best(ev_d)}   wall ms {best(wall_d)}")
    say(f"  (a) / (b), wall, host transforms: {a_frame / min(wall_h):.1f}    device transforms: {a_frame / min(wall_d):.1f}")
    mr_dev, ms_dev, hits_dev, out_dev = rate(dev_tl)
    same = int((out_dev.view(np.uint8).reshape(-1, 128) == out_host.view(np.uint8).reshape(-1, 128)).all(1).sum())
    say(f"  (c) Intersect, {rays.shape[0]} camera rays, host-built (SAH) tree    {mr_host:8.1f} MRays/s   ms {best(ms_host)}   {hits_host} hits")
    say(f"  (c) Intersect, {rays.shape[0]} camera rays, device-built (LBVH) tree {mr_dev:8.1f} MRays/s   ms {best(ms_dev)}   {hits_dev} hits, {rays.shape[0] - same} records differ")
    ctx.free(d_rays); ctx.free(d_T)
    host_tl.free(); dev_tl.free()


def run_refit(ctx, reps):
    verts = to_dbl(scenes.atrium(262_267, seed=1)) + np.array([1e7, 0.0, -1e7])
    t0 = time.perf_counter()
    host = tb.host_build_double(verts)
    nodes, idx = host.nodes(), host.prim_idx()
    say(f"== atrium, {verts.shape[0] // 3} triangles, {len(nodes)} nodes at (1e7, 0, -1e7): host build {time.perf_counter() - t0:.2f} s ==")
    sc = tb.BVH_Double(ctx).Upload(nodes, idx, verts)
    up = []
    for k in range(reps + 1):
        ctx.synchronize()
        t0 = time.perf_counter()
        fresh = tb.BVH_Double(ctx).Upload(nodes, idx, verts)
        fresh.free()
        if k:
            up.append((time.perf_counter() - t0) * 1e3)
    first = wall_ms(ctx, lambda: sc.Refit(verts))
    d_v = ctx.malloc(verts.nbytes)
    ev_h, wall_h, ev_d, wall_d = [], [], [], []
    for k in range(reps + 1):
        v = verts + 0.01 * k
        w = wall_ms(ctx, lambda: sc.Refit(v))
        if k:
            wall_h.append(w); ev_h.append(ctx.time_last_ms())
    for k in range(reps + 1):
        ctx.to_device(d_v, verts)
        w = wall_ms(ctx, lambda: sc.Refit(d_v, on_device=True))
        if k:
            wall_d.append(w); ev_d.append(ctx.time_last_ms())
    ctx.free(d_v)
    say(f"  (d) fresh upload + free             wall ms {best(up)}")
    say(f"  (d) first refit (parent pass)       wall ms {first:10.3f}")
    say(f"  (d) refit, host vertices            event ms {best(ev_h)}   wall ms {best(wall_h)}")
    say(f"  (d) refit, device vertices          event ms {best(ev_d)}   wall ms {best(wall_d)}")
    say(f"  upload / refit, wall, host vertices: {min(up) / min(wall_h):.1f}    device vertices: {min(up) / min(wall_d):.1f}")
    sc.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", default="1000,100000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rays", type=int, default=1 << 21)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "double_anim.txt"))
    a = ap.parse_args()
    ctx = tb.Context(0)
    say(f"double_anim_bench: one warm-up, then the best of {a.reps} (min .. max)")
    blas_verts, _ = instance_scene(3)
    blas = [tb.BVH_Double(ctx).Build(v) for v in blas_verts]
    bounds = np.stack([b.bounds for b in blas])
    for n in [int(x) for x in a.counts.split(",") if x]:
        run_tlas(ctx, blas, bounds, n, a.reps, a.rays)
    run_refit(ctx, a.reps)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
