"""A fixed history of query launches on two-level scenes, for comparing two builds of the library launch by launch (profiles/tlas_plan.txt): the rows a to h
of tests/tlas_edges_lib.py (one per class of two-level kernel and kind of query; stated again here so that the tool runs on a tree without the tests), each
as a TLAS of 27 instances over the row's two BLASes: closest and any hit at two batch sizes, TLAS.Update with the same arrays, the queries again,
RebuildOnDevice, the queries again.  The context synchronises after every launch.  The sibling of tools/launch_history.py, whose `dispatches` reads the trace.

  python tools/tlas_history.py history             the history, one line per step on stdout (with each scene's device_bytes); meant to run under
                                                   `rocprofv3 --kernel-trace`
  python tools/tlas_history.py hosttime [LAUNCHES] the host's cost of a launch call on a TLAS: wall time of LAUNCHES (4000) back-to-back tbvh_intersect_device
                                                   calls of 4096 rays on row d's TLAS, synchronised once at the end; us per call with and without that wait

TBVH_TREE names another checkout whose package is loaded instead of this one's (the parent commit's, built)."""
import os
import sys
import time

import numpy as np

ROOT = os.environ.get("TBVH_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

L2, L4, L8, LS = 5, 8, 10, 1
ROWS = {   # layouts, variants of the two BLASes
    "a": ((L4, L4), (0, 0)), "a1": ((L4, L4), (1, 1)), "b": ((L8, L8), (0, 0)), "c": ((L8, L8), (72, 72)), "d": ((L2, L2), (0, 0)),
    "e": ((L2, L2), (1, 1)), "f": ((L8, L2), (72, 1)), "g": ((L4, L8), (1, 72)), "h": ((LS, L4), (0, 0)),
}


def make_row(tb, scenes, ctx, key):
    meshes = [scenes.blob(3000, seed=3), scenes.soup(1500, seed=9, extent=1.6, size=0.25)]
    rng = np.random.default_rng(21)
    sph = np.concatenate([rng.uniform(-0.7, 0.7, (400, 3)), rng.uniform(0.02, 0.1, (400, 1))], 1).astype(np.float32)
    blas = []
    for k, (lay, var) in enumerate(zip(*ROWS[key])):
        b = tb.SphereBVH(ctx).Build(sph) if lay == LS else tb.LAYOUT_CLASSES[lay](ctx).Build(meshes[k])
        if var:
            b.set_variant(var)
        blas.append(b)
    grid = np.stack([np.eye(4, dtype=np.float32)] * 27)
    grid[:, :3, 3] = np.array([[x, y, z] for x in range(3) for y in range(3) for z in range(3)], np.float32) * 2.0
    inst = tb.make_instances(grid, (np.arange(27) % 2).astype(np.uint32))
    return blas, tb.TLAS(ctx).Build(inst, blas), inst


def main():
    sys.path.insert(0, ROOT)
    import tinybvh_amd as tb
    from tinybvh_amd import rays as R, scenes

    ctx = tb.Context(0)
    cam = R.camera((2.8, 2.8, -9.0), (0.0, 0.0, 1.0), 1024, 1024, 1, 1)
    if sys.argv[1:2] == ["hosttime"]:
        launches = int(sys.argv[2]) if len(sys.argv) > 2 else 4000
        n = 4096
        blas, tl, _ = make_row(tb, scenes, ctx, "d")
        d = ctx.malloc(n * 64)
        ctx.generate_primary(R.camera((2.8, 2.8, -9.0), (0.0, 0.0, 1.0), 64, 64, 1, 1), d, 0, n)
        for _ in range(launches // 4):                      # warm: code objects, the second lane, the event ring all the way round
            tl.intersect_device(d, n)
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(launches):
            tl.intersect_device(d, n)
        t1 = time.perf_counter()
        ctx.synchronize()
        t2 = time.perf_counter()
        print(f"hosttime tlas launches {launches} rays {n} us_per_call_enqueue {(t1 - t0) / launches * 1e6:.3f} us_per_call_with_final_sync {(t2 - t0) / launches * 1e6:.3f}")
        return
    n_max = 1 << 20
    d, d_occ = ctx.malloc(n_max * 64), ctx.malloc(n_max)
    step = [0]

    def say(key, what, tl, blas):
        print(f"step {step[0]:3d} row {key:2s} {what:22s} tlas bytes {tl.device_bytes} blas bytes {[b.device_bytes for b in blas]}", flush=True)
        step[0] += 1

    def queries(key, tl, blas):
        for n in (1000, n_max):
            for anyhit in (False, True):
                ctx.generate_primary(cam, d, 0, n)
                if anyhit:
                    tl.occluded_device(d, n, d_occ)
                else:
                    tl.intersect_device(d, n)
                ctx.synchronize()
                say(key, f"{'any' if anyhit else 'closest'} n {n}", tl, blas)

    for key in ROWS:
        blas, tl, inst = make_row(tb, scenes, ctx, key)
        say(key, "upload", tl, blas)
        queries(key, tl, blas)
        tl.Build(inst, blas)                                  # tbvh_update_tlas with the same arrays
        say(key, "update", tl, blas)
        queries(key, tl, blas)
        tl.RebuildOnDevice()
        ctx.synchronize()
        say(key, "rebuild on device", tl, blas)
        queries(key, tl, blas)
        tl.free()
        for b in blas:
            b.free()
    ctx.close()


if __name__ == "__main__":
    main()
