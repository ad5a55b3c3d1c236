"""The device SBVH builder (tbvh_build_device_sbvh: the reference's BVH::BuildHQ tree, kernels_sbvhbuild.hip) beside the reference's own host build
and the device SAH builder, in one run: build time on the device, host BuildHQ time through oracle/_ref (threaded and not), the builder's kernel
split from a rocprofv3 --kernel-trace --stats run of its own (a child process, started before this one opens the GPU), and what the trees cost at
trace time (camera and first-bounce MRays/s; node visits per ray where the library in use has the instrumented kernel, i.e. the EXPERIMENTS build
through TBVH_LIB_OVERRIDE).  No threshold is set for any of it: the file says what came out.  Writes profiles/sbvh_device_build.txt.
    python tools/sbvh_build_bench.py [out.txt] [side]
    python tools/sbvh_build_bench.py --trace-child     (what the rocprofv3 run executes: three builds of street_rot(262144))"""
import csv
import ctypes as C
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tinybvh_amd as tb  # noqa: E402
from tinybvh_amd import rays as R  # noqa: E402
from tinybvh_amd import scenes  # noqa: E402

TRACE_SCENE = 262144
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def rot_atrium(v):
    return scenes.rotate(scenes.rotate(v, 1, 0.6), 0, 0.35)


def rot_atrium_camera():
    eye, view = scenes.SPONZA_CAMERAS[0]
    e = rot_atrium(np.asarray([list(eye) + [0.0]], np.float32)); d = rot_atrium(np.asarray([list(view) + [0.0]], np.float32))
    return tuple(float(x) for x in e[0, :3]), tuple(float(x) for x in d[0, :3])


def trace_child():
    verts = scenes.street_rot(TRACE_SCENE)
    ctx = tb.Context(0)
    for _ in range(3):
        tb.build_bvh2_sbvh(ctx, verts)
    ctx.close()


def kernel_split():
    """per kernel of the builder: calls, total ms and share over three builds of street_rot(262144), from rocprofv3's kernel_stats.csv"""
    if shutil.which("rocprofv3") is None:
        say("kernel split: rocprofv3 is not installed here: not measured")
        return
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(["rocprofv3", "--output-format", "csv", "--kernel-trace", "--stats", "-d", d, "-o", "kt", "--", sys.executable, os.path.abspath(__file__), "--trace-child"],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        found = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode or not found:
            say(f"kernel split: the rocprofv3 run failed (exit {r.returncode}): not measured")
            return
        rows = list(csv.DictReader(open(found[0])))
    rows = [x for x in rows if "sbvh" in x["Name"]]
    total = sum(float(x["TotalDurationNs"]) for x in rows)
    say(f"kernel split, street_rot({TRACE_SCENE}), three builds under rocprofv3 --kernel-trace --stats (kernel time {total / 3e6:.2f} ms per build):")
    for x in sorted(rows, key=lambda x: -float(x["TotalDurationNs"])):
        m = re.search(r"k_sbvh_\w+", x["Name"])
        name = m.group(0) if m else x["Name"][:32]
        say(f"  {name:32s} {int(x['Calls']) // 3:6d} launches per build, {float(x['TotalDurationNs']) / 3e6:9.3f} ms per build, {100 * float(x['TotalDurationNs']) / total:5.1f} %")


def visits(ctx, sc, d_rays, n):
    """node visits and triangle tests per ray from the instrumented kernel, or None where the library has none"""
    try:
        sc.set_variant(59)
    except tb.TbvhError:
        return None
    st = (C.c_uint64 * 8)()
    tb.lib.tbvh_debug_stats(ctx._h, st, 1)
    sc.intersect_device(d_rays, n)
    tb.lib.tbvh_debug_stats(ctx._h, st, 1)
    sc.set_variant(0)
    return (int(st[2]) / n, int(st[4]) / n) if int(st[2]) else None


def host_build_hq(reference, verts, threaded):
    t0 = time.perf_counter()
    s = reference.build(verts, hq=True, threaded=threaded)
    t = (time.perf_counter() - t0) * 1e3
    del s
    return t


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sbvh_device_build.txt")
    side = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
    say(f"# tools/sbvh_build_bench.py, {side} x {side} rays per batch; device times: best of 3 after one warm-up build (median in brackets)")
    kernel_split()   # (first: the child process has the GPU to itself, this process has not opened it yet)
    from oracle_lib import Reference, have_reference
    reference = Reference() if have_reference() else None
    ctx = tb.Context(0)
    for label, verts, cam in (("street_rot(2832120)", scenes.street_rot(), scenes.street_rot_camera(0)), (f"street_rot({TRACE_SCENE})", scenes.street_rot(TRACE_SCENE), scenes.street_rot_camera(0)),
                              ("rotated atrium(262267)", rot_atrium(scenes.atrium(262267)), rot_atrium_camera())):
        n_tris = verts.shape[0] // 3
        if reference is None:
            say(f"{label}: host BuildHQ: oracle/_ref is not built: not measured")
        else:
            say(f"{label}: host BuildHQ (the reference, this machine's CPU): {host_build_hq(reference, verts, True):.0f} ms threaded, {host_build_hq(reference, verts, False):.0f} ms non-threaded")
        d_verts = ctx.malloc(verts.nbytes); ctx.to_device(d_verts, verts)
        m = tb.device_mesh(d_verts, verts.shape[0], n_tris)
        cap_n, cap_i = 3 * n_tris, n_tris + n_tris // 2
        d_n = ctx.malloc(cap_n * 32); d_i = ctx.malloc(cap_i * 4)
        nn, ni = C.c_uint64(0), C.c_uint64(0)
        st = (C.c_uint64 * len(tb.SBVH_STATS))()
        for k in (0, 3):
            ts, ws = [], []
            for it in range(4):
                ctx.synchronize()
                t0 = time.perf_counter()
                tb.check(tb.lib.tbvh_build_bvh2_sbvh_device(ctx._h, C.byref(m), k, C.c_void_p(d_n), cap_n, C.c_void_p(d_i), cap_i, 1, C.byref(nn), C.byref(ni), st), "tbvh_build_bvh2_sbvh_device")
                ws.append((time.perf_counter() - t0) * 1e3); ts.append(ctx.time_last_ms())
            say(f"{label}: device SBVH, BVH2 alone (resident vertices, max_leaf_tris {k}): {min(ts[1:]):.2f} ms on the device ({np.median(ts[1:]):.2f}), {min(ws[1:]):.2f} ms wall, "
                f"{nn.value} nodes, {ni.value} references, {n_tris / min(ts[1:]) / 1e3:.2f} Mtris/s")
        say(f"{label}: " + ", ".join(f"{k[2:]} {int(v)}" for k, v in zip(tb.SBVH_STATS, st)))
        ts = []
        for it in range(4):
            tb.check(tb.lib.tbvh_build_bvh2_sah_device(ctx._h, C.byref(m), 0, C.c_void_p(d_n), cap_n, C.c_void_p(d_i), cap_i, 1, C.byref(nn)), "tbvh_build_bvh2_sah_device")
            ts.append(ctx.time_last_ms())
        say(f"{label}: device SAH, BVH2 alone: {min(ts[1:]):.2f} ms on the device, {nn.value} nodes")
        ctx.free(d_n); ctx.free(d_i)
        trees = []
        for nm, builder in (("device SBVH blob", "sbvh"), ("device SAH blob", "sah")):
            ts = []
            sc = None
            for it in range(3):
                if sc is not None:
                    sc.free()
                sc = tb.BVH8_CWBVH(ctx).BuildOnDevice(verts, builder=builder); ctx.synchronize()
                ts.append(ctx.time_last_ms())
            say(f"{label}: {nm}: build + conversion {min(ts[1:]):.2f} ms on the device; {sc.device_bytes / 1e6:.0f} MB")
            trees.append((nm, sc))
        n = side * side
        camera = R.camera(*cam, side, side, 1, 1)
        d = ctx.malloc(n * 64); d_b = ctx.malloc(n * 64)
        for nm, sc in trees:
            tc_, tb_ = [], []
            for p in range(4):
                ctx.generate_primary(camera, d, 0, n); sc.intersect_device(d, n); tc_.append(ctx.time_last_ms())
                ctx.generate_bounce(d_verts, d, d_b, n, 1); sc.intersect_device(d_b, n); tb_.append(ctx.time_last_ms())
            vb = visits(ctx, sc, d_b, n)
            ctx.generate_primary(camera, d, 0, n)
            vc = visits(ctx, sc, d, n)
            extra = "; node visits: not measured (no instrumented kernel in this library)" if vb is None or vc is None else \
                f"; node visits per ray: camera {vc[0]:.2f}, bounce {vb[0]:.2f}; triangle tests: camera {vc[1]:.2f}, bounce {vb[1]:.2f}"
            say(f"  {label}: {nm:17s}: camera {n / np.mean(tc_[1:]) / 1e3:.0f} MRays/s, bounce {n / np.mean(tb_[1:]) / 1e3:.0f} MRays/s{extra}")
        ctx.free(d); ctx.free(d_b)
        for _, sc in trees:
            sc.free()
        ctx.free(d_verts)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--trace-child":
        trace_child()
    else:
        main()
