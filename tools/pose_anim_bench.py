"""Skinned / morphed meshes per frame (DESIGN.md par. 14, profiles/pose_anim.txt): what a frame of an animated mesh costs
 (a) as a caller has it without the device pose: Mesh::SetPose on the host (tbvh_host_pose_skin, one thread, the restated arithmetic) + a host-staged
     Refit of the shared vertices (n_verts * 16 bytes over the link);
 (b) with it: SetPose (n_joints * 64 bytes over the link, k_pose_skin) + Pose.Refit, everything else on the device;
for BVH_GPU and BVH8_CWBVH, on two indexed meshes: the bunny (34 817 vertices, 69 630 triangles) and a procedural tube of 1024 x 1024 vertices
(1 048 576 vertices, 2 095 104 triangles), 24 joints.  (a) and (b) alternate frame by frame on the same scene with a new set of joint matrices every
frame; wall clock around calls that return when the device is done.
 (k) the pose kernels alone, device-resident parameters: bytes moved per vertex / kernel time (tbvh_time_last_ms) beside tbvh_measure_copy_bandwidth
     of the same run.  Skin streams 64 bytes per vertex (rest, joints, weights in, vertex out) and gathers 4 x 64 bytes from the joint table, which
     stays in cache; morph streams 12 (T + 1) + 16.
Every figure: one warm-up, then the median of --reps repetitions with the spread (min .. max).
usage: python tools/pose_anim_bench.py [--sets bunny,tube] [--reps R] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pose_lib as P  # noqa: E402
import tinybvh_amd as tb  # noqa: E402

OUT = []


def say(line):
    print(line, flush=True)
    OUT.append(line)


def spread(v):
    v = np.array(v, np.float64)
    return f"{np.median(v):9.3f}  ({v.min():.3f} .. {v.max():.3f})"


def mesh_set(name):
    """(rest (n, 4), indices (m, 3), joints, weights, joint heights)"""
    if name == "bunny":
        rest, joints, weights, jy, idx = P.skinned_bunny(step=1, indexed=True)
        return rest, idx, joints, weights, jy
    rings = sides = 1024
    r, s = np.meshgrid(np.arange(rings), np.arange(sides), indexing="ij")
    a = (2 * np.pi / sides) * s
    rest = np.zeros((rings * sides, 4), np.float32)
    rest[:, 0] = (np.cos(a) * (1.0 + 0.2 * np.sin(9 * np.pi * r / rings))).reshape(-1)
    rest[:, 1] = (10.0 * r / (rings - 1)).reshape(-1)
    rest[:, 2] = (np.sin(a) * (1.0 + 0.2 * np.sin(9 * np.pi * r / rings))).reshape(-1)
    v0 = (r[:-1] * sides + s[:-1]).reshape(-1); v1 = (r[:-1] * sides + (s[:-1] + 1) % sides).reshape(-1)
    idx = np.stack([v0, v1, v0 + sides, v1, v1 + sides, v0 + sides], 1).reshape(-1, 3).astype(np.uint32)
    joints, weights, jy = P.skeleton(rest)
    return rest, idx, joints, weights, jy


def run_set(ctx, name, reps):
    rest, idx, joints, weights, jy = mesh_set(name)
    n, m = rest.shape[0], idx.shape[0]
    say(f"== {name}: {n} vertices, {m} triangles, {jy.size} joints ==")
    pose = tb.Pose(ctx).Skin(rest, joints, weights, jy.size)
    frames = [P.joint_mats(jy, f, scale=(f % 3 == 2)) for f in range(reps + 1)]
    for label, cls in (("BVH_GPU", tb.BVH_GPU), ("BVH8_CWBVH", tb.BVH8_CWBVH)):
        t0 = time.perf_counter()
        sc = cls(ctx).Build(rest, indices=idx)
        say(f"  {label}: host build + upload {time.perf_counter() - t0:.2f} s")
        a_pose, a_refit, b_set, b_refit, b_dev = [], [], [], [], []
        for k, mats in enumerate(frames):
            t0 = time.perf_counter()
            posed = tb.host_pose_skin(rest, joints, weights, mats)
            t1 = time.perf_counter()
            sc.Refit(posed, mesh=True)
            t2 = time.perf_counter()
            pose.SetPose(mats)
            t3 = time.perf_counter()
            pose.Refit(sc)
            t4 = time.perf_counter()
            if k:
                a_pose.append((t1 - t0) * 1e3); a_refit.append((t2 - t1) * 1e3); b_set.append((t3 - t2) * 1e3); b_refit.append((t4 - t3) * 1e3)
        a = np.array(a_pose) + np.array(a_refit); b = np.array(b_set) + np.array(b_refit)
        say(f"  (a) {label:11s} host SetPose                 wall ms {spread(a_pose)}")
        say(f"  (a) {label:11s} host-staged Refit            wall ms {spread(a_refit)}")
        say(f"  (a) {label:11s} frame                        wall ms {spread(a)}")
        say(f"  (b) {label:11s} SetPose (returns at once)    wall ms {spread(b_set)}")
        say(f"  (b) {label:11s} Pose.Refit                   wall ms {spread(b_refit)}")
        say(f"  (b) {label:11s} frame                        wall ms {spread(b)}     (a) / (b) = {np.median(a) / np.median(b):.2f}")
        sc.free()
    # (k) the kernels alone
    d_mats = ctx.malloc(frames[0].nbytes); ctx.to_device(d_mats, frames[1])
    ms = []
    for k in range(reps + 1):
        pose.SetPose(d_mats, on_device=True); ctx.synchronize()
        if k:
            ms.append(ctx.time_last_ms())
    ms = np.array(ms)
    say(f"  (k) k_pose_skin   device us {spread(ms * 1e3)}   64 B/vertex streamed: {n * 64 / np.median(ms) / 1e6:8.1f} GB/s  ({n * 64 / ms.max() / 1e6:.1f} .. {n * 64 / ms.min() / 1e6:.1f}); "
        f"with the 256 B/vertex of cached matrix gathers: {n * 320 / np.median(ms) / 1e6:.1f} GB/s")
    ctx.free(d_mats); pose.free()
    T = 3
    rng = np.random.default_rng(5)
    pos = np.empty((T + 1, n, 3), np.float32)
    pos[0] = rest[:, :3]
    for t in range(T):
        pos[t + 1] = pos[0] + rng.normal(scale=0.01, size=(n, 3)).astype(np.float32)
    mp = tb.Pose(ctx).Morph(pos)
    d_w = ctx.malloc(16); ctx.to_device(d_w, np.array([0.3, -0.2, 0.7, 0], np.float32))
    ms = []
    for k in range(reps + 1):
        mp.SetPose(d_w, on_device=True); ctx.synchronize()
        if k:
            ms.append(ctx.time_last_ms())
    ms = np.array(ms)
    per = 12 * (T + 1) + 16
    say(f"  (k) k_pose_morph  device us {spread(ms * 1e3)}   {per} B/vertex ({T} targets): {n * per / np.median(ms) / 1e6:8.1f} GB/s  ({n * per / ms.max() / 1e6:.1f} .. {n * per / ms.min() / 1e6:.1f})")
    ctx.free(d_w); mp.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="bunny,tube")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = tb.Context(0)
    say(f"pose_anim_bench: {a.reps} frames after one warm-up, median (min .. max); (a) and (b) alternate frame by frame")
    say(f"tbvh_measure_copy_bandwidth (1 GiB, read + write): {ctx.copy_bandwidth_gbps():.0f} GB/s")
    for name in a.sets.split(","):
        run_set(ctx, name, a.reps)
        if a.out:   # (kept current set by set)
            with open(a.out, "w") as f:
                f.write("\n".join(OUT) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
