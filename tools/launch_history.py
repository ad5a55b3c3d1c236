"""A fixed history of query launches on ONE context, for comparing two builds of the library launch by launch (profiles/launch_plan.txt): a small scene
(under 48 MB) and a street of about a million triangles (between 48 and 384 MB) as BVH8_CWBVH, the small one also as BVH_GPU and BVH4_GPU, one TLAS per
BLAS layout; batch sizes on both sides of every threshold of tinybvh_amd/csrc/launch_plan.h those scenes reach; closest and any hit; two ray buffers
taken alternately.  The context synchronises after every launch, so nothing the library decides depends on timing as long as TBVH_COHERENT_TUNER pins the
schedule (0, 2 or 3: modes 1, 2, 3).

  python tools/launch_history.py history             the history, one line per launch on stdout; meant to run under `rocprofv3 --kernel-trace`
  python tools/launch_history.py dispatches DIR      the trace rocprofv3 left under DIR as lines of kernel name, grid size, workgroup size, in dispatch order
  python tools/launch_history.py hosttime [LAUNCHES] the host's cost of a launch call: wall time of LAUNCHES (4000) back-to-back tbvh_intersect_device calls
                                                     of 4096 rays on the small scene, synchronised once at the end; us per call with and without that wait

TBVH_TREE names another checkout whose package is loaded instead of this one's (the parent commit's, built)."""
import csv
import glob
import os
import sys
import time

import numpy as np

ROOT = os.environ.get("TBVH_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dispatches(d):
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    dims = lambda r, what: "x".join(str(r[k]) for k in sorted(r) if k.startswith(what))
    for r in rows:
        print(f'{r["Kernel_Name"]} grid {dims(r, "Grid_Size")} workgroup {dims(r, "Workgroup_Size")}')


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "dispatches":
        return dispatches(sys.argv[2])
    sys.path.insert(0, ROOT)
    import tinybvh_amd as tb
    from tinybvh_amd import rays as R, scenes

    ctx = tb.Context(0)
    small_verts = scenes.soup(20_000)
    small = tb.BVH8_CWBVH(ctx).Build(small_verts)
    if sys.argv[1:2] == ["hosttime"]:
        launches = int(sys.argv[2]) if len(sys.argv) > 2 else 4000
        n = 4096
        d = ctx.malloc(n * 64)
        ctx.generate_primary(R.camera((5.0, 5.0, -12.0), (0.0, 0.0, 1.0), 64, 64, 1, 1), d, 0, n)
        for _ in range(launches // 4):                      # warm: code objects, the second lane, the event ring all the way round
            small.intersect_device(d, n)
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(launches):
            small.intersect_device(d, n)
        t1 = time.perf_counter()
        ctx.synchronize()
        t2 = time.perf_counter()
        print(f"hosttime launches {launches} rays {n} us_per_call_enqueue {(t1 - t0) / launches * 1e6:.3f} us_per_call_with_final_sync {(t2 - t0) / launches * 1e6:.3f}")
        return
    street = tb.BVH8_CWBVH(ctx).Build(scenes.street(1_000_000, seed=2))
    blob_verts = scenes.soup(4_000, seed=3, extent=1.6, size=0.2)
    step = [0]
    n_max = 12 << 20
    bufs = [ctx.malloc(n_max * 64), ctx.malloc(n_max * 64)]
    d_occ = ctx.malloc(n_max)

    def run(label, sc, cam_pose, sizes, anyhits=(False, True)):
        cam = R.camera(*cam_pose, 4096, 4096, 1, 1)
        for n in sizes:
            for anyhit in anyhits:
                d = bufs[step[0] & 1]
                ctx.generate_primary(cam, d, 0, n)
                if anyhit:
                    sc.occluded_device(d, n, d_occ)
                elif step[0] % 3 == 2:
                    sc.intersect_device_fresh(d, n, 1e30)
                else:
                    sc.intersect_device(d, n)
                ctx.synchronize()
                print(f"launch {step[0]:3d} {label:12s} n {n:9d} {'any' if anyhit else 'closest'} buffer {step[0] & 1} probe {ctx.last_probe()[2] != 0}", flush=True)
                step[0] += 1

    soup_cam = ((5.0, 5.0, -12.0), (0.0, 0.0, 1.0))
    # on 256 CUs: the rays at which the grid leaves its floor (4 workgroups per CU), reaches the persistent grid (24 per CU) and, on a small scene, a third more
    floor, cap, cap_small = 256 * 4 * 128, 256 * 24 * 128, 256 * 32 * 128
    grid_edges = [1000, floor, floor + 64, cap - 128, cap, cap + 128]
    probe_edges = [x + dx for x in (3 << 18, 3 << 19, 1 << 21, 6 << 20, 12 << 20) for dx in (-64, 0)]
    run("small", small, soup_cam, sorted(set(grid_edges + [cap_small - 128, cap_small, cap_small + 128] + probe_edges)))
    run("street", street, scenes.STREET_CAMERAS[0], sorted(set(grid_edges + probe_edges)))
    ctx.set_debug_flags(64)
    run("street f64", street, scenes.STREET_CAMERAS[0], [1 << 21])
    ctx.set_debug_flags(4)
    run("street f4", street, scenes.STREET_CAMERAS[0], [1 << 21])
    ctx.set_debug_flags(0)
    run("street again", street, scenes.STREET_CAMERAS[1], [(1 << 21) - 64, 1 << 21])          # (the copies for incoherent batches exist by now)
    for name, cls in (("bvh_gpu", tb.BVH_GPU), ("bvh4_gpu", tb.BVH4_GPU)):
        sc = cls(ctx).Build(small_verts)
        run(name, sc, soup_cam, [1000, 1023, 1024, cap - 64, cap + 128, 1 << 21])
    grid = np.stack([np.eye(4, dtype=np.float32)] * 27)
    grid[:, :3, 3] = np.array([[x, y, z] for x in range(3) for y in range(3) for z in range(3)], np.float32) * 2.0
    for name, cls in (("tlas cwbvh", tb.BVH8_CWBVH), ("tlas bvh4", tb.BVH4_GPU), ("tlas bvh_gpu", tb.BVH_GPU)):
        blas = cls(ctx).Build(blob_verts)
        tl = tb.TLAS(ctx).Build(tb.make_instances(grid, 0), [blas])
        run(name, tl, ((2.8, 2.8, -9.0), (0.0, 0.0, 1.0)), grid_edges + [1 << 21])
    ctx.synchronize()
    ctx.close()


if __name__ == "__main__":
    main()
