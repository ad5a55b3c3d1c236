"""A viewer frame on the device (DESIGN.md par. 22, profiles/viewer.txt): what a frame of tiny_bvh_gltf.cpp's viewer costs from the camera to the pixels
 (d) on the device: tbvh_viewer_render, the frame's event pair (tbvh_viewer_stats::frame_ms), rounds and rays per round;
 (h) as a caller has it without it: trace + tbvh_shade_hits_device on the device, the 64 + 48 bytes per pixel copied back, the alpha rule, the continue
     step, the lighting and the pack on --threads host threads (at most 16) through the host twins; the rays that continue go up again, are traced and
     shaded as a batch of their own and come back, round by round;
at 800 x 600 and 4096 x 4096 on the bench's street scene (one BVH8_CWBVH BLAS; --tris scales it) from its first camera, one FatTri per triangle, one
material with a 1024 x 1024 texture of which a quarter of the texels are masked for the viewer's alpha rule (x + y + z <= 5), a 1024 x 512 sky.  One
warm-up, then (d) and (h) alternate; median and spread (min .. max) of the repeats.  The per-stage split of (d) is not measured here, and (h)'s "host
arithmetic and gathers" includes this script's NumPy gathers and scatters between the threaded calls: a C caller would pay less for them.
The tool rewrites its own section of the output file and leaves what stands before it (tools/viewer_math_error.c's lines).
usage: python tools/viewer_bench.py [--tris N] [--reps R] [--host-reps R] [--threads T] [--out FILE]"""
import argparse
import ctypes as C
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tinybvh_amd as tb  # noqa: E402
from tinybvh_amd import rays as R  # noqa: E402
from tinybvh_amd import scenes  # noqa: E402
from shade_bench import flat_fat_tris, spread  # noqa: E402

MARK = "# ---- tools/viewer_bench.py ----"
OUT = []


def say(line):
    print(line, flush=True)
    OUT.append(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=2_832_120)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "viewer.txt"))
    a = ap.parse_args()
    threads = max(1, min(16, a.threads))
    if tb.device_count() <= 0:
        sys.exit("tools/viewer_bench.py measures on the GPU: no HIP device")
    ctx = tb.Context(0)
    verts = scenes.street(a.tris)
    fat = flat_fat_tris(verts)
    rng = np.random.default_rng(3)
    tex = ((rng.integers(3, 256, (1024, 1024)).astype(np.uint32) << 24) | rng.integers(0x060606, 1 << 24, (1024, 1024)).astype(np.uint32))
    tex[rng.random((1024, 1024)) < 0.25] = 0xFF010101
    mats = np.zeros(1, tb.MATERIAL_DTYPE); mats["color_texture"] = 0; mats["normal_texture"] = tb.NO_TEXTURE
    sky_pixels = rng.uniform(0, 2, (512, 1024, 3)).astype(np.float32)
    sc = tb.BVH8_CWBVH(ctx).Build(verts)
    sh = tb.Shading(ctx, mats, [tex]).SetFatTris(0, fat)
    sky = tb.SkyDome(ctx, sky_pixels)
    eye, view = scenes.cameras("street")[0]
    pool = ThreadPoolExecutor(threads)
    say(MARK)
    say(f"viewer_bench: street scene, {fat.size} triangles, one 1024 x 1024 texture (a quarter of its texels masked), a 1024 x 512 sky, mode TBVH_VIEWER_GLTF, "
        f"{threads} host threads for (h)")
    for w, h in ((800, 600), (4096, 4096)):
        n = w * h
        cam = R.camera(eye, view, w, h, 1, 1)
        v = tb.Viewer(ctx, w, h)
        d_rays, d_out, d_q, d_qo = ctx.malloc(n * 64), ctx.malloc(n * 48), ctx.malloc(n * 64), ctx.malloc(n * 48)
        rays = tb._aligned(np.zeros(n, tb.RAY_DTYPE)); out = tb._aligned(np.zeros((n, 12), np.float32))
        rgb = tb._aligned(np.zeros((n, 4), np.float32)); pix = np.zeros(n, np.uint32); went = np.zeros(n, np.uint8)
        cuts = np.linspace(0, n, threads + 1).astype(np.int64)

        def parts(m):
            c = np.linspace(0, m, threads + 1).astype(np.int64)
            return [(int(c[k]), int(c[k + 1] - c[k])) for k in range(threads) if c[k + 1] > c[k]]

        def host_frame():
            """(total ms, copy ms, host arithmetic ms, rays per round): generation is not counted (the parent's callers make their rays on the host or with the
            tile generator); everything from the trace on is"""
            tb.viewer_generate(ctx, cam, d_rays)
            ctx.synchronize()
            t0 = time.perf_counter()
            copy = host = 0.0
            sc.intersect_device(d_rays, n)
            sh.ShadeHitsDevice(sc, d_rays, n, d_out)
            c0 = time.perf_counter()
            ctx.from_device(rays, d_rays); ctx.from_device(out, d_out)
            copy += time.perf_counter() - c0
            live = np.arange(n)
            per_round = [n]
            for _ in range(1, 8):
                h0 = time.perf_counter()
                sub = tb._aligned(rays[live]) if live.size != n else rays
                sub_out = tb._aligned(out[live]) if live.size != n else out
                m = sub.shape[0]

                def cont(p):
                    lo, k = p
                    tb.check(tb.lib.tbvh_host_viewer_continue(C.c_void_p(mats.ctypes.data), 1, 1, C.c_void_p(sub.ctypes.data + 64 * lo), 64, C.c_void_p(sub_out.ctypes.data + 48 * lo), k,
                                                              C.c_void_p(went.ctypes.data + lo), None), "tbvh_host_viewer_continue")
                list(pool.map(cont, parts(m)))
                go = went[:m].astype(bool)
                host += time.perf_counter() - h0
                if not go.any():
                    break
                live = live[go]
                q = np.ascontiguousarray(sub[go])
                c0 = time.perf_counter()
                ctx.to_device(d_q, q)
                copy += time.perf_counter() - c0
                sc.intersect_device(d_q, q.shape[0])
                sh.ShadeHitsDevice(sc, d_q, q.shape[0], d_qo)
                back, back_out = np.zeros(q.shape[0], tb.RAY_DTYPE), np.zeros((q.shape[0], 12), np.float32)
                c0 = time.perf_counter()
                ctx.from_device(back, d_q); ctx.from_device(back_out, d_qo)
                copy += time.perf_counter() - c0
                h0 = time.perf_counter()
                rays[live] = back; out[live] = back_out
                host += time.perf_counter() - h0
                per_round.append(int(live.size))
            h0 = time.perf_counter()

            def light(p):
                lo, k = p
                tb.check(tb.lib.tbvh_host_viewer_light(0, C.c_void_p(sky_pixels.ctypes.data), 1024, 512, C.c_void_p(rays.ctypes.data + 64 * lo), 64, C.c_void_p(out.ctypes.data + 48 * lo),
                                                       None, k, None, C.c_void_p(rgb.ctypes.data + 16 * lo)), "tbvh_host_viewer_light")
                tb.check(tb.lib.tbvh_host_viewer_pack(C.c_void_p(rgb.ctypes.data + 16 * lo), k, C.c_void_p(pix.ctypes.data + 4 * lo)), "tbvh_host_viewer_pack")
            list(pool.map(light, parts(n)))
            host += time.perf_counter() - h0
            return (time.perf_counter() - t0) * 1e3, copy * 1e3, host * 1e3, per_round

        st = v.Render(sc, sh, sky, cam)                                   # warm-up (the schedule tuner samples its first launches)
        for _ in range(6):
            st = v.Render(sc, sh, sky, cam)
        host_frame()
        dev, tot, cp, ho = [], [], [], []
        for r in range(a.reps):
            st = v.Render(sc, sh, sky, cam)
            dev.append(st["frame_ms"])
            if r < a.host_reps:
                t, c, hh, per_round = host_frame()
                tot.append(t); cp.append(c); ho.append(hh)
        same = np.array_equal(v.Pixels().reshape(-1), pix)
        say(f"  {w} x {h}: rays per round {st['rays']}")
        say(f"    (d) tbvh_viewer_render, frame ms                  {spread(dev)}   {n / np.median(dev) / 1e3:8.1f} M pixels/s")
        say(f"    (h) device trace + shade, 112 bytes per pixel back, loop and lighting on {threads} host threads, ms   {spread(tot)}")
        say(f"        of which copies, ms                           {spread(cp)}")
        say(f"        of which host arithmetic and gathers, ms      {spread(ho)}")
        say(f"        (d) is {np.median(tot) / np.median(dev):.0f} x faster; rays per round on the host path {per_round}; pixels equal bit for bit: {same}")
        for d in (d_rays, d_out, d_q, d_qo):
            ctx.free(d)
        v.free()
        if not same:
            sys.exit(1)
    sky.free(); sh.free(); sc.free(); ctx.close()
    keep = []
    if os.path.exists(a.out):
        with open(a.out) as f:
            for line in f.read().split("\n"):
                if line.strip() == MARK:
                    break
                keep.append(line)
    while keep and not keep[-1].strip():
        keep.pop()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(keep + [""] + OUT) + "\n")


if __name__ == "__main__":
    main()
