#!/usr/bin/env python
"""The animated frame with the scene graph on the host against the scene graph on the device (DESIGN.md par. 17), interleaved A/B:
  (a) tbvh_host_scenegraph_advance on one thread, then the instance transforms, joint matrices and morph weights go up from host memory
  (b) tbvh_scenegraph_advance: one float goes up, the outputs are read where the graph wrote them
both followed by the same TLAS.RebuildOnDevice + Pose.SetPose + Pose.Refit and one synchronize.  Two sizes: the drone fixture (93 nodes, 100 channels, 39
instances) and a crowd (a 24-joint rig replicated 4096 times under one root: ~100 k nodes, ~100 k channels, 4096 instances).  One warm-up frame, then the median of
9 frames per side with the spread; the device time of each graph kernel comes from tbvh_debug_scenegraph_step (one kernel as a timed operation of its own).
usage: python tools/scenegraph_anim_bench.py [--out profiles/scenegraph_anim.txt] [--copies 4096]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import pose_lib as P  # noqa: E402
import scenegraph_lib as L  # noqa: E402
import tinybvh_amd as tb  # noqa: E402

FRAMES, DT = 9, 1.0 / 60


def crowd(copies, seed=11):
    """one root; per copy a mesh node (an instance, a skin use) followed by its 24-joint chain with a rotation channel per joint; 24 samplers shared by all copies"""
    rng = np.random.default_rng(seed)
    b = L.Builder()
    root = b.node(-1)
    samplers = [b.sampler(L.LINEAR, L.QUAT, L._times(rng, 8, dur=2.0), L._rot_keys(rng, 8)) for _ in range(P.N_JOINTS)]
    ib = [L._affine(rng, 0.1) for _ in range(P.N_JOINTS)]
    side = int(np.ceil(np.sqrt(copies)))
    for c in range(copies):
        place = np.eye(4, dtype=np.float32); place[0, 3] = 0.4 * (c % side); place[2, 3] = 0.4 * (c // side)
        mesh = b.node(root, local=place.reshape(16))
        p, joints = root, []
        for j in range(P.N_JOINTS):
            p = b.node(p if j else root, t=(0, 0.01, 0), local=L.IDENT)
            joints.append(p)
            b.channel(0, samplers[j], p, 1)
        b.instance(mesh)
        b.skin(mesh, joints, ib)
    return b.desc()


def depth_of(d):
    par = np.asarray(d["parent"]); depth = np.zeros(par.size, np.int64); todo = list(range(par.size))
    order = np.asarray(d["visit_order"]) if d.get("visit_order") is not None else np.arange(par.size)
    for n in order:
        depth[n] = 1 + (depth[par[n]] if par[n] >= 0 else 0)
    return int(depth.max())


def host_array(ptr, shape):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_float)), shape)


def measure(ctx, name, d, lines):
    dev, host = tb.SceneGraph(ctx, d), tb.HostSceneGraph(d)
    n_inst = dev.n_instances
    gs = P.golden("skin_bunny16"); rest = P.rest4(gs)
    blas = tb.BVH8_CWBVH(ctx).Build(rest)
    ext = rest[:, :3].max(0) - rest[:, :3].min(0)
    blas._bounds = np.concatenate([rest[:, :3].min(0) - 4 * ext, rest[:, :3].max(0) + 4 * ext]).astype(np.float32)
    tlas = tb.TLAS(ctx).Build(tb.make_instances(np.stack([np.eye(4, dtype=np.float32)] * n_inst), np.zeros(n_inst, np.uint32)), [blas])
    skinned = dev.n_skin_uses > 0 and dev.JointMatrices(0)[1] == P.N_JOINTS
    pose = tb.Pose(ctx).Skin(rest, gs["joints"], gs["weights"], P.N_JOINTS) if skinned else None
    d_inst = dev.InstanceTransforms()[0]
    h_inst = host_array(host.InstanceTransforms()[0], (n_inst, 16))
    d_joints = dev.JointMatrices(0)[0] if skinned else None
    h_joints = host_array(host.JointMatrices(0)[0], (P.N_JOINTS, 16)) if skinned else None

    def frame_host():
        host.Advance(DT)
        tlas.RebuildOnDevice(h_inst)
        if skinned:
            pose.SetPose(h_joints).Refit(blas)
        ctx.synchronize()

    def frame_device():
        dev.Advance(DT)
        tlas.RebuildOnDevice(d_inst, on_device=True)
        if skinned:
            pose.SetPose(d_joints, on_device=True).Refit(blas)
        ctx.synchronize()

    frame_host(); frame_device()      # the warm-up
    ta, tb_ = [], []
    for _ in range(FRAMES):
        t0 = time.perf_counter(); frame_host(); t1 = time.perf_counter(); frame_device(); t2 = time.perf_counter()
        ta.append((t1 - t0) * 1e3); tb_.append((t2 - t1) * 1e3)
    cpu = []
    for _ in range(FRAMES):
        t0 = time.perf_counter(); host.Advance(DT); cpu.append((time.perf_counter() - t0) * 1e3)
    wall, whole, kern = [], [], [[], [], [], []]
    for _ in range(FRAMES):
        t0 = time.perf_counter(); dev.Advance(DT); ctx.synchronize(); wall.append((time.perf_counter() - t0) * 1e3)
        whole.append(ctx.time_last_ms())
    for _ in range(FRAMES):
        for step in range(4):
            tb.check(tb.lib.tbvh_debug_scenegraph_step(dev._h, step, DT), "tbvh_debug_scenegraph_step")
            ctx.synchronize(); kern[step].append(ctx.time_last_ms())
    st = lambda v: f"{np.median(v):8.3f} ms (min {min(v):.3f}, max {max(v):.3f})"
    lines.append(f"{name}: {dev.n_nodes} nodes, {dev.n_channels} channels, {n_inst} instances, {dev.n_joints} joints, depth {depth_of(d)}; chain: TLAS rebuild"
                 + (" + skin pose of one 24-joint BLAS + refit" if skinned else " only (the graph has no 24-joint skin)"))
    lines.append(f"  (a) host graph + upload + chain, wall clock per frame   {st(ta)}")
    lines.append(f"  (b) device graph + chain, wall clock per frame          {st(tb_)}")
    lines.append(f"      host twin advance alone, one thread                 {st(cpu)}")
    lines.append(f"      device advance + synchronize alone, wall clock          {st(wall)}")
    lines.append(f"      device time of one advance (all four kernels)       {st(whole)}")
    for step, kn in enumerate(("k_graph_sample", "k_graph_local", "k_graph_combine", "k_graph_outputs")):
        lines.append(f"      device time: {kn:<38s} {st(kern[step])}")
    lines.append(f"      per-frame upload saved by (b): {n_inst * 64 + (P.N_JOINTS * 64 if skinned else 0)} bytes of the chain's inputs ({n_inst * 64 + dev.n_joints * 64 + dev.n_weights * 4} bytes for every output)")
    if pose is not None:
        pose.free()
    tlas.free(); blas.free(); dev.free(); host.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--copies", type=int, default=4096)
    a = ap.parse_args()
    ctx = tb.Context(0)
    lines = ["scene graph on the host (a) against the scene graph on the device (b); interleaved, 1 warm-up, median of 9 frames, dt = 1/60 s",
             "device times are tbvh_time_last_ms of a kernel launched as an operation of its own (tbvh_debug_scenegraph_step)", ""]
    measure(ctx, "drone", L.golden_desc(L.golden("drone")), lines)
    lines.append("")
    measure(ctx, f"crowd x{a.copies}", crowd(a.copies), lines)
    ctx.close()
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
