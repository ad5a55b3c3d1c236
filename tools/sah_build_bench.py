"""The device SAH builder (tbvh_build_device_sah: the reference's binned-SAH tree, kernels_sahbuild.hip) against the LBVH, PLOC and the host path,
in one run: build time (device and wall) and what the trees cost at trace time (camera and first-bounce MRays/s; node visits per ray where the
library in use has the instrumented kernel, i.e. the EXPERIMENTS build through TBVH_LIB_OVERRIDE).  Writes profiles/sah_device_build.txt.
    python tools/sah_build_bench.py [out.txt] [side]"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tinybvh_amd as tb  # noqa: E402
from tinybvh_amd import rays as R  # noqa: E402
from tinybvh_amd import scenes  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sah_device_build.txt")
side = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed_build(ctx, make, reps=4):
    """(scene, best device ms, best wall ms) over reps builds; the first one warms allocations and code objects up and does not count"""
    dev, wall, sc = [], [], None
    for it in range(reps + 1):
        if sc is not None:
            sc.free()
        ctx.synchronize()
        t0 = time.perf_counter(); sc = make(); ctx.synchronize(); t = (time.perf_counter() - t0) * 1e3
        if it:
            dev.append(ctx.time_last_ms()); wall.append(t)
    return sc, min(dev), min(wall), float(np.median(dev))


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


say(f"# tools/sah_build_bench.py, {side} x {side} rays per batch; times: best of 4 after one warm-up build (median in brackets)")
ctx = tb.Context(0)
for label, verts, cams in (("atrium(262267)", scenes.atrium(262267), scenes.SPONZA_CAMERAS), ("street(2832120)", scenes.street(2832120), scenes.STREET_CAMERAS),
                           ("soup(3000)", scenes.soup(3000, seed=5), None)):
    n_tris = verts.shape[0] // 3
    d_verts = ctx.malloc(verts.nbytes); ctx.to_device(d_verts, verts)
    t0 = time.perf_counter(); host = tb.BVH8_CWBVH(ctx).Build(verts); ctx.synchronize(); t_host = (time.perf_counter() - t0) * 1e3
    say(f"{label}: host path (build + encode + upload) {t_host:.0f} ms wall")
    trees = [("library host builder", host)]
    for nm, kw in (("device SAH", dict(builder="sah")), ("device LBVH", dict()), ("device PLOC r16", dict(builder="ploc"))):
        sc, ms, wall, med = timed_build(ctx, lambda: tb.BVH8_CWBVH(ctx).BuildOnDevice(verts, **kw))
        say(f"{label}: {nm:16s} build + conversion {ms:8.2f} ms on the device ({med:.2f}), {wall:8.1f} ms wall incl. uploading {verts.nbytes / 1e6:.0f} MB of vertices; {sc.device_bytes / 1e6:.0f} MB")
        trees.append((nm + " tree", sc))
    # the builder alone, vertices resident: the BVH2 stays on the device
    d_n = ctx.malloc(2 * n_tris * 32); d_i = ctx.malloc(n_tris * 4)
    m = tb.device_mesh(d_verts, verts.shape[0], n_tris)
    nn = C.c_uint64(0)
    for k in (0, 3):
        ts, ws = [], []
        for it in range(5):
            ctx.synchronize()
            t0 = time.perf_counter()
            tb.check(tb.lib.tbvh_build_bvh2_sah_device(ctx._h, C.byref(m), k, C.c_void_p(d_n), 2 * n_tris, C.c_void_p(d_i), n_tris, 1, C.byref(nn)), "tbvh_build_bvh2_sah_device")
            ws.append((time.perf_counter() - t0) * 1e3); ts.append(ctx.time_last_ms())
        say(f"{label}: BVH2 alone (resident vertices, max_leaf_tris {k}): {min(ts[1:]):.2f} ms on the device, {min(ws[1:]):.2f} ms wall, {nn.value} nodes, {n_tris / min(ts[1:]) / 1e3:.1f} Mtris/s")
    # the small-subtree threshold (tbvh_debug_set_sah_small_subtree): the tree is the same, the time is not
    sweep = []
    for thr in (0, 8, 16, 32, 64, 128, 256, 1024):
        tb.check(tb.lib.tbvh_debug_set_sah_small_subtree(ctx._h, thr), "tbvh_debug_set_sah_small_subtree")
        ts = []
        for it in range(4):
            tb.check(tb.lib.tbvh_build_bvh2_sah_device(ctx._h, C.byref(m), 0, C.c_void_p(d_n), 2 * n_tris, C.c_void_p(d_i), n_tris, 1, C.byref(nn)), "tbvh_build_bvh2_sah_device")
            ts.append(ctx.time_last_ms())
        sweep.append(f"{thr}: {min(ts[1:]):.2f}")
    tb.check(tb.lib.tbvh_debug_set_sah_small_subtree(ctx._h, 64), "tbvh_debug_set_sah_small_subtree")
    say(f"{label}: BVH2 alone, ms on the device by small-subtree threshold: " + ", ".join(sweep))
    ctx.free(d_n); ctx.free(d_i)
    # the same tree from the host: the twin's BVH2 through the device conversion
    n2h, pih = tb.host_build_bvh2_sah(verts, max_leaf_tris=3)
    trees.append(("host twin's tree, converted", tb.BVH8_CWBVH(ctx).ConvertFromBVH2(n2h, pih, verts)))
    if cams is not None:
        n = side * side
        cam = R.camera(*cams[0], side, side, 1, 1)
        d = ctx.malloc(n * 64); d_b = ctx.malloc(n * 64)
        for nm, sc in trees:
            tc_, tb_ = [], []
            for p in range(4):
                ctx.generate_primary(cam, d, 0, n); sc.intersect_device(d, n); tc_.append(ctx.time_last_ms())
                ctx.generate_bounce(d_verts, d, d_b, n, 1); sc.intersect_device(d_b, n); tb_.append(ctx.time_last_ms())
            vb = visits(ctx, sc, d_b, n)
            ctx.generate_primary(cam, d, 0, n)
            vc = visits(ctx, sc, d, n)
            extra = "" if vb is None or vc is None else f"; node visits per ray: camera {vc[0]:.2f}, bounce {vb[0]:.2f}; triangle tests: camera {vc[1]:.2f}, bounce {vb[1]:.2f}"
            say(f"  {label}: {nm:27s}: camera {n / np.mean(tc_[1:]) / 1e3:.0f} MRays/s, bounce {n / np.mean(tb_[1:]) / 1e3:.0f} MRays/s{extra}")
        ctx.free(d); ctx.free(d_b)
    for _, sc in trees:
        sc.free()
    ctx.free(d_verts)
ctx.close()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
