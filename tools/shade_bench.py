"""Hits resolved to shading data (DESIGN.md par. 16, profiles/shade.txt): what GetShadingData costs per batch of hit records
 (d) on the device: tbvh_shade_hits_device, kernel time (tbvh_time_last_ms), device-resident records in and out;
 (h) as a caller has it without the kernel: the 64-byte records copied back (tbvh_copy_from_device) + tbvh_host_shade_hits, the records split over
     --threads host threads (at most 16), each calling the C entry point on its slice (arguments and output prepared outside the timed region);
on 4096 x 4096 = 16.7 M primary rays of the first street camera through the bench's street scene (one BVH8_CWBVH BLAS; --tris scales it), one FatTri per
triangle (flat normals, UVs from the positions), one material with a 1024 x 1024 texture; and (s) the same records in a random order, so that
neighbouring lanes gather far-apart FatTris.  Bytes: STREAMED per record 64 read (48 are used, the line comes whole) and 48 written; GATHERED per hit 80
of the FatTri, the 20-byte material, a 16-byte descriptor and a 4-byte texel — neighbouring camera rays share them, so they are cache hits more often
than memory traffic.  The streamed rate is set against tbvh_measure_read_bandwidth of the same run.  One warm-up, then (d), (s) and (h) alternate; median
and spread (min .. max) of the repeats.
usage: python tools/shade_bench.py [--tris N] [--side S] [--reps R] [--host-reps R] [--threads T] [--out FILE]"""
import argparse
import ctypes as C
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tinybvh_amd as tb  # noqa: E402
from tinybvh_amd import rays as R  # noqa: E402
from tinybvh_amd import scenes  # noqa: E402

OUT = []


def say(line):
    print(line, flush=True)
    OUT.append(line)


def spread(v):
    v = np.array(v, np.float64)
    return f"{np.median(v):10.3f}  ({v.min():.3f} .. {v.max():.3f})"


def flat_fat_tris(verts):
    t = verts.reshape(-1, 3, 4)[:, :, :3]
    f = np.zeros(t.shape[0], tb.FATTRI_DTYPE)
    N = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    l = np.sqrt((N * N).sum(1, keepdims=True))
    N = (N / np.where(l == 0, 1, l)).astype(np.float32)
    f["Nx"], f["Ny"], f["Nz"] = N[:, 0], N[:, 1], N[:, 2]
    for k in range(3):
        f[f"vertex{k}"] = t[:, k]
        f[f"vN{k}"] = N
        f[f"u{k}"] = t[:, k, 0] * np.float32(0.37) + t[:, k, 1] * np.float32(0.11)
        f[f"v{k}"] = t[:, k, 2] * np.float32(0.37) + t[:, k, 1] * np.float32(0.23)
    f["ltriIdx"] = -1
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=2_832_120)
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shade.txt"))
    a = ap.parse_args()
    threads = max(1, min(16, a.threads))
    if tb.device_count() <= 0:
        sys.exit("tools/shade_bench.py measures on the GPU: no HIP device")
    ctx = tb.Context(0)
    verts = scenes.street(a.tris)
    fat = flat_fat_tris(verts)
    rng = np.random.default_rng(3)
    tex = ((rng.integers(0, 256, (1024, 1024)).astype(np.uint32) << 24) | rng.integers(0, 1 << 24, (1024, 1024)).astype(np.uint32))
    mats = np.zeros(1, tb.MATERIAL_DTYPE); mats["color_texture"] = 0; mats["normal_texture"] = tb.NO_TEXTURE
    sc = tb.BVH8_CWBVH(ctx).Build(verts)
    sh = tb.Shading(ctx, mats, [tex]).SetFatTris(0, fat)
    n = a.side * a.side
    eye, view = scenes.cameras("street")[0]
    cam = R.camera(eye, view, a.side, a.side, 1, 1)
    d_rays, d_out = ctx.malloc(n * 64), ctx.malloc(n * 48)
    ctx.generate_primary(cam, d_rays, 0, n)
    sc.intersect_device(d_rays, n)
    ctx.synchronize()
    host_rays = np.zeros(n, tb.RAY_DTYPE)
    ctx.from_device(host_rays, d_rays)
    hits = int((host_rays["t"] < 1e30).sum())
    streamed, gathered = n * 112, hits * 120
    d_shuf = ctx.malloc(n * 64)
    ctx.to_device(d_shuf, host_rays[np.random.default_rng(9).permutation(n)])
    bw = ctx.read_bandwidth_gbps()
    say(f"shade_bench: {fat.size} triangles ({fat.nbytes / 1e6:.0f} MB of FatTri records), {n} records, {hits} hits ({100.0 * hits / n:.1f} %), "
        f"{streamed / 1e6:.0f} MB streamed + {gathered / 1e6:.0f} MB gathered per batch; read bandwidth measured {bw:.0f} GB/s")
    ctx.set_timing(True)

    def device_ms(d=None):
        sh.ShadeHitsDevice(sc, d or d_rays, n, d_out)
        ctx.synchronize()
        return ctx.time_last_ms()

    # (h): everything a call needs is made once — the descriptor arrays, one record slice and one output slice per thread — so that the timed region
    # holds the copy back and tbvh_host_shade_hits alone
    pool = ThreadPoolExecutor(threads)
    back = np.zeros(n, tb.RAY_DTYPE)
    host_out = np.zeros((n, 12), np.float32)
    cuts = np.linspace(0, n, threads + 1).astype(np.int64)
    tex_arr = (tb.AlphaTexture * 1)(tb.AlphaTexture(C.c_void_p(tex.ctypes.data), 1024, 1024))
    slot_ptrs = (C.c_void_p * 1)(fat.ctypes.data)
    slot_counts = np.array([fat.size], np.uint64)
    assert back.ctypes.data % 16 == 0 and host_out.ctypes.data % 16 == 0 and fat.ctypes.data % 16 == 0

    def host_slice(k):
        lo, m = int(cuts[k]), int(cuts[k + 1] - cuts[k])
        tb.check(tb.lib.tbvh_host_shade_hits(C.c_void_p(mats.ctypes.data), 1, tex_arr, 1, slot_ptrs, C.c_void_p(slot_counts.ctypes.data), 1, None, 0,
                                             C.c_void_p(back.ctypes.data + 64 * lo), m, 64, C.c_void_p(host_out.ctypes.data + 48 * lo)), "tbvh_host_shade_hits")

    def host_ms():
        t0 = time.perf_counter()
        ctx.from_device(back, d_rays)
        t1 = time.perf_counter()
        list(pool.map(host_slice, range(threads)))
        t2 = time.perf_counter()
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3

    device_ms(); device_ms(d_shuf); host_ms()                  # warm-up
    dev, shuf, copy, host = [], [], [], []
    for r in range(a.reps):
        shuf.append(device_ms(d_shuf))
        dev.append(device_ms())
        if r < a.host_reps:
            c, h = host_ms()
            copy.append(c); host.append(h)
    got = np.zeros((n, 12), np.float32)
    ctx.from_device(got, d_out)
    same = np.array_equal(got.view(np.uint32), host_out.view(np.uint32))
    say(f"  (d) tbvh_shade_hits_device, kernel ms             {spread(dev)}   {n / np.median(dev) / 1e3:8.1f} M records/s   streamed {streamed / np.median(dev) / 1e6:7.1f} GB/s "
        f"= {100.0 * streamed / np.median(dev) / 1e6 / bw:.1f} % of the measured read bandwidth")
    say(f"  (s) the same records in a random order, kernel ms   {spread(shuf)}   {n / np.median(shuf) / 1e3:8.1f} M records/s   streamed + gathered "
        f"{(streamed + gathered) / np.median(shuf) / 1e6:7.1f} GB/s")
    say(f"  (h) records copied back, ms                       {spread(copy)}")
    say(f"      tbvh_host_shade_hits on {threads:2d} threads, ms          {spread(host)}")
    total = np.array(copy) + np.array(host)
    say(f"      (h) in all, ms                                {spread(total)}   {n / np.median(total) / 1e3:8.1f} M records/s; (d) is {np.median(total) / np.median(dev):.0f} x faster")
    say(f"  device records equal the host's bit for bit: {same}")
    ctx.free(d_rays); ctx.free(d_out); ctx.free(d_shuf)
    sh.free(); sc.free(); ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(OUT) + "\n")
    if not same:
        sys.exit(1)


if __name__ == "__main__":
    main()
