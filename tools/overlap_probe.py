"""What overlapping independent launches within ONE context is worth (tbvh_context_set_overlap): a stream of two independent batches — camera rays in one
buffer, their diffuse bounces in another — traced alternately, 10 pairs enqueued back to back, wall clock between two synchronizes; overlap off and on
interleaved, medians of 7.  The counterpart of tools/two_context_overlap.py (two contexts) and of profiles/r05_split_halves.txt (one query cut in halves).
Usage: python tools/overlap_probe.py [scene] [side ...]"""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tinybvh_amd as tb
from tinybvh_amd import rays as R, scenes

name = sys.argv[1] if len(sys.argv) > 1 else "bistro"
sides = [int(x) for x in sys.argv[2:]] or [1024, 2048]
verts, label = scenes.get(name)
cams = scenes.cameras(name)
ctx = tb.Context(0)
sc = tb.BVH8_CWBVH(ctx).Build(verts)
d_verts = ctx.malloc(verts.nbytes); ctx.to_device(d_verts, verts)
PAIRS, REPS = 10, 7
for side in sides:
    n = side * side
    cam = R.camera(*cams[0], side, side, 1, 1)
    d_a, d_b = ctx.malloc(n * 64), ctx.malloc(n * 64)
    ctx.generate_primary(cam, d_a, 0, n)
    sc.intersect_device(d_a, n)
    ctx.generate_bounce(d_verts, d_a, d_b, n, 4001)
    ctx.synchronize()
    for d in (d_a, d_b):                         # the scene's schedule tuner decides before anything is timed (it serialises what it measures)
        for _ in range(14):
            sc.intersect_device_fresh(d, n, 1e30); ctx.synchronize()
            if sc.coherent_schedule(False)[0]:
                break
    wall = {False: [], True: []}
    sums = {False: [], True: []}
    lane1 = 0
    for r in range(REPS + 1):
        for on in (False, True):
            ctx.set_overlap(on)
            s0 = ctx.overlap_stats()[0]
            ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(PAIRS):
                sc.intersect_device_fresh(d_a, n, 1e30)
                sc.intersect_device_fresh(d_b, n, 1e30)
            ctx.synchronize()
            t1 = time.perf_counter()
            if r:
                wall[on].append((t1 - t0) / PAIRS)
                sums[on].append(sum(ctx.time_history(2 * PAIRS)) / PAIRS)
                lane1 += ctx.overlap_stats()[0] - s0
    f = lambda x: f"{np.median(x) * 1e6:7.1f} us (min {np.min(x) * 1e6:7.1f}, max {np.max(x) * 1e6:7.1f})"
    print(f"{label[:28]:28s} 2 x {n:8d} rays per pair: overlap off {f(wall[False])} = {2 * n / np.median(wall[False]) / 1e6:6.0f} MRays/s   on {f(wall[True])} = "
          f"{2 * n / np.median(wall[True]) / 1e6:6.0f} MRays/s   x{np.median(wall[False]) / np.median(wall[True]):.3f}   reported per pair off {np.median(sums[False]) * 1e3:.1f} us, on {np.median(sums[True]) * 1e3:.1f} us   "
          f"launches on the second lane {lane1}", flush=True)
    ctx.free(d_a); ctx.free(d_b)
ctx.close()
