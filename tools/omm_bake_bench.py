"""Opacity micromaps from alpha textures (DESIGN.md par. 15, profiles/omm_bake.txt): what Mesh::CreateOpacityMicroMaps( N ) costs
 (h) as a caller has it without the device bake: tbvh_host_bake_opacity_micromaps (the restated arithmetic; the triangles split over --threads host threads,
     at most 16, each calling the entry point on its slice) + tbvh_set_opacity_micromaps of the result (n_tris * words * 4 bytes over the link);
 (d) the device bake alone, device-resident source: kernel time (tbvh_set_timing / tbvh_time_last_ms), and samples per second — a textured triangle
     takes (4N - 1) * 2N samples, each one texel fetch;
 (f) the fused bake-and-install (tbvh_bake_set_opacity_micromaps), wall clock around the call (it returns when the maps are installed): from a
     device-resident source, and from host arrays (UVs, indices and the 4 MB texture go up first);
on two indexed meshes — every second triangle of the bunny (34 815 triangles, UVs generated from the positions) and a grid of 724 x 724 quads
(1 048 352 triangles) — with a 1024 x 1024 leaf texture repeated over them, N = 8 and 32, on a BVH8_CWBVH scene.
Every figure: one warm-up, then the median of --reps repetitions with the spread (min .. max); (h) takes --host-reps.
usage: python tools/omm_bake_bench.py [--sets bunny,grid] [--reps R] [--host-reps R] [--threads T] [--out FILE]"""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import omm_lib as O  # noqa: E402
import tinybvh_amd as tb  # noqa: E402

OUT = []


def say(line):
    print(line, flush=True)
    OUT.append(line)


def spread(v):
    v = np.array(v, np.float64)
    return f"{np.median(v):10.3f}  ({v.min():.3f} .. {v.max():.3f})"


def mesh_set(name):
    """(positions (n, 4), indices (m, 3), uv (n, 2)): an indexed mesh with one UV per vertex"""
    if name == "bunny":
        d = np.load(os.path.join(ROOT, "tests", "golden", "meshes", "bunny.npz"))
        idx = d["indices"][::2]
        used, inv = np.unique(idx.reshape(-1), return_inverse=True)
        pos = np.zeros((used.size, 4), np.float32); pos[:, :3] = d["positions"][used]
        idx = np.ascontiguousarray(inv.reshape(-1, 3).astype(np.uint32))
        p = pos[:, :3]; ext = p.max(0) - p.min(0)
        # a cylindrical unwrap, 6 x 4 repeats of the leaf: a bunny triangle covers a few hundred texels
        uv = np.stack([np.arctan2(p[:, 2] - p[:, 2].mean(), p[:, 0] - p[:, 0].mean()) / (2 * np.pi) * 6, (p[:, 1] - p[:, 1].min()) / ext[1] * 4], 1)
        return pos, idx, np.ascontiguousarray(uv, np.float32)
    q = 724
    gy, gx = np.meshgrid(np.arange(q + 1), np.arange(q + 1), indexing="ij")
    pos = np.zeros(((q + 1) * (q + 1), 4), np.float32)
    pos[:, 0] = gx.reshape(-1) * (10.0 / q); pos[:, 2] = gy.reshape(-1) * (10.0 / q)
    pos[:, 1] = 0.3 * np.sin(pos[:, 0] * 3) * np.cos(pos[:, 2] * 2)
    v0 = (gy[:-1, :-1] * (q + 1) + gx[:-1, :-1]).reshape(-1)
    idx = np.stack([v0, v0 + 1, v0 + q + 1, v0 + 1, v0 + q + 2, v0 + q + 1], 1).reshape(-1, 3).astype(np.uint32)
    uv = np.stack([pos[:, 0] * 4.0, pos[:, 2] * 4.0], 1)     # 40 x 40 repeats: a quad covers about 57 x 57 texels
    return pos, np.ascontiguousarray(idx), np.ascontiguousarray(uv, np.float32)


def host_bake_threads(pool, threads, uv, tex, N, idx):
    """the host entry point over `threads` slices of the triangles"""
    cuts = np.linspace(0, idx.shape[0], threads + 1).astype(np.int64)
    parts = list(pool.map(lambda k: tb.host_bake_opacity_micromaps(uv, tex, N, indices=idx[cuts[k]:cuts[k + 1]]), range(threads)))
    return np.concatenate(parts)


def run_set(ctx, name, a, pool):
    pos, idx, uv = mesh_set(name)
    m = idx.shape[0]
    tex = O.leaf_texture(1024)
    say(f"== {name}: {m} triangles, {pos.shape[0]} vertices, one 1024 x 1024 texture ({100.0 * float((tex >> 24 > 2).mean()):.0f} % opaque) ==")
    t0 = time.perf_counter()
    sc = tb.BVH8_CWBVH(ctx).Build(pos, indices=idx)
    say(f"  BVH8_CWBVH host build + upload {time.perf_counter() - t0:.2f} s")
    d_uv, d_idx, d_tex = ctx.malloc(uv.nbytes), ctx.malloc(idx.nbytes), ctx.malloc(tex.nbytes)
    ctx.to_device(d_uv, uv); ctx.to_device(d_idx, idx.reshape(-1)); ctx.to_device(d_tex, tex)
    dsrc = tb.device_omm_source(d_uv, uv.shape[0], m, [(d_tex, 1024, 1024)], d_indices=d_idx)
    for N in (8, 32):
        W = O.words_per_tri(N)
        samples = m * (4 * N - 1) * 2 * N
        say(f"  -- N = {N}: {W} words per triangle, {m * W * 4 / 1e6:.1f} MB of maps, {samples / 1e6:.0f} M samples --")
        want = None
        h_bake, h_set = [], []
        for k in range(a.host_reps + 1):
            t0 = time.perf_counter()
            want = host_bake_threads(pool, a.threads, uv, tex, N, idx)
            t1 = time.perf_counter()
            sc.SetOpacityMicroMaps(want, N)
            t2 = time.perf_counter()
            if k:
                h_bake.append((t1 - t0) * 1e3); h_set.append((t2 - t1) * 1e3)
        h = np.array(h_bake) + np.array(h_set)
        say(f"  (h) host bake, {a.threads} threads            wall ms {spread(h_bake)}   {samples / np.median(h_bake) / 1e6:9.2f} G samples/s")
        say(f"  (h) tbvh_set_opacity_micromaps       wall ms {spread(h_set)}")
        say(f"  (h) bake + install                   wall ms {spread(h)}")
        d_out = ctx.malloc(m * W * 4)
        ms = []
        for k in range(a.reps + 1):
            tb.bake_opacity_micromaps(ctx, dsrc, N=N, d_out=d_out); ctx.synchronize()
            if k:
                ms.append(ctx.time_last_ms())
        got = np.zeros((m, W), np.uint32); ctx.from_device(got, d_out); ctx.free(d_out)
        assert np.array_equal(got, want), "the device bake and the host bake differ"
        ms = np.array(ms)
        say(f"  (d) k_omm_bake, device-resident      dev  ms {spread(ms)}   {samples / np.median(ms) / 1e6:9.2f} G samples/s  "
            f"({samples / ms.max() / 1e6:.2f} .. {samples / ms.min() / 1e6:.2f})")
        f_dev, f_host = [], []
        for k in range(a.reps + 1):
            t0 = time.perf_counter()
            sc.BakeOpacityMicroMaps(dsrc, None, N)
            t1 = time.perf_counter()
            sc.BakeOpacityMicroMaps(uv, tex, N, indices=idx)
            t2 = time.perf_counter()
            if k:
                f_dev.append((t1 - t0) * 1e3); f_host.append((t2 - t1) * 1e3)
        say(f"  (f) fused, device-resident source    wall ms {spread(f_dev)}   (h) / (f) = {np.median(h) / np.median(f_dev):.1f}")
        say(f"  (f) fused, host arrays               wall ms {spread(f_host)}   (h) / (f) = {np.median(h) / np.median(f_host):.1f}")
    for d in (d_uv, d_idx, d_tex):
        ctx.free(d)
    sc.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="bunny,grid")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    a.threads = max(1, min(16, a.threads))
    ctx = tb.Context(0)
    ctx.set_timing(True)
    say(f"omm_bake_bench: {a.reps} repetitions after one warm-up ((h): {a.host_reps}), median (min .. max); the host baseline uses {a.threads} threads")
    with ThreadPoolExecutor(a.threads) as pool:
        for name in a.sets.split(","):
            run_set(ctx, name, a, pool)
            if a.out:   # (kept current set by set)
                with open(a.out, "w") as f:
                    f.write("\n".join(OUT) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
