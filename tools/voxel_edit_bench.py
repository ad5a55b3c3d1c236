"""What editing a voxel set on the device costs (kernels_voxel_edit.hip), against the only way there was to change a voxel before: build the dense
array's set on the host, upload it as a new scene, free the old one (tbvh_upload_voxelset_dense + tbvh_free_scene).  One MI355X, best of --reps.

    python tools/voxel_edit_bench.py [--reps 5] [--out profiles/voxel_edit.txt]

Batches of 1, 10^3 and 10^5 seeded random records {x, y, z, v} go into the legocar set (128^3 voxels in the 256^3 object):
  event ms     the call's two timed operations together, capacity reserved (no growth): HIP events around the mark pass with its 8-byte copy back, and
               around everything that writes the set
  read-back    the first of the two alone: the mark pass and the copy back the host waits for before it decides growth
  wall ms      host clock around the call and a synchronize, device-resident records, capacity reserved
  host recs    the same with the records in host memory (staged by the call)
  + growth     the same batch into a freshly uploaded set (capacity = used bricks), so the call reallocates: allocate, copy, zero the tail, swap
  top grid     tbvh_voxelset_update_top_grid, event ms
  re-upload    wall ms of tbvh_upload_voxelset_dense of the 128^3 array into a new scene, then tbvh_free_scene: the parent's path, whatever the
               number of voxels changed
Then tbvh_voxelize_device of the Sponza stand-in and of the bunny (tinybvh_amd/scenes.py: get("sponza"), get("dragon")), each into an empty set, with a
one-material shading table and with a constant colour: rounds, records, bricks, and the HIP-event time of every stage summed over the rounds (each
stage is a timed operation: tbvh_time_history), beside the wall time of the whole call, which adds the per-round read-backs and the allocations.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tinybvh_amd as tb  # noqa: E402
from tinybvh_amd import lib  # noqa: E402
import voxel_lib as V  # noqa: E402


def wall_ms(ctx, f):
    ctx.synchronize()
    t0 = time.perf_counter()
    f()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


def voxelize_stages(ctx, reps):
    """tbvh_voxelize_device stage by stage: the call's timed operations are, per round, trace, (shade,) step, then sort, the Set's two and UpdateTopGrid"""
    from tinybvh_amd import scenes
    rows = []
    for name in ("sponza", "dragon"):
        verts, label = scenes.get(name)
        blas = tb.LAYOUT_CLASSES[tb.LAYOUT_CWBVH](ctx).Build(verts)
        n_tris = verts.shape[0] // 3
        mats = np.zeros(1, tb.MATERIAL_DTYPE)
        mats["color"] = (0.8, 0.6, 0.4); mats["color_texture"] = tb.NO_TEXTURE; mats["normal_texture"] = tb.NO_TEXTURE
        table = tb.Shading(ctx, mats, None).SetFatTris(0, np.zeros(n_tris, tb.FATTRI_DTYPE))
        v3 = verts[:, :3]
        bmin, max_size, ext = tb.voxelize_bounds(np.concatenate([v3.min(0), v3.max(0)]))
        for sh, how in ((table, "table"), (None, "colour")):
            tried = []
            for _ in range(reps + 1):                      # (the first repetition builds the scene's derived copies and is dropped)
                vs = tb.VoxelSet(ctx).CreateOnDevice(40000)
                st = {}
                w = wall_ms(ctx, lambda: st.update(vs.Voxelize(blas, bmin, max_size, ext, shading=sh, color=0xC08040)))
                per = 3 if sh is not None else 2
                k = st["rounds"] * per + 4
                h = ctx.time_history(k) if k <= 256 else []
                vs.free()
                if len(h) != k:
                    row = {"trace_ms": float("nan"), "shade_ms": float("nan"), "step_ms": float("nan"), "sort_ms": float("nan"), "set_ms": float("nan"), "top_ms": float("nan")}
                else:
                    body = h[:st["rounds"] * per]
                    row = {"trace_ms": sum(body[0::per]), "shade_ms": sum(body[1::per]) if per == 3 else 0.0, "step_ms": sum(body[per - 1::per]),
                           "sort_ms": h[-4], "set_ms": h[-3] + h[-2], "top_ms": h[-1]}
                row.update({"scene": f"{name} ({n_tris} tris), {how}", "label": label, "wall_ms": w, **st})
                tried.append(row)
            best = min(tried[1:] or tried, key=lambda r: r["wall_ms"])
            rows.append({k2: (round(v, 4) if isinstance(v, float) else v) for k2, v in best.items()})
        table.free(); blas.free()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = tb.Context(0)
    ctx.set_timing(True)
    dense = np.ascontiguousarray(V.scene_dense("legocar"))
    arrays = tb.host_build_voxelset(dense)
    rng = np.random.default_rng(1)
    rows = []
    for n in (1, 1000, 100000):
        recs = rng.integers(0, 256, (n, 4)).astype(np.uint32)
        recs[:, 3] = rng.integers(1, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        d = ctx.malloc(recs.nbytes)
        ctx.to_device(d, recs)
        ev, rb, wall, wall_host, grow, top = [], [], [], [], [], []
        bricks_added = 0
        for _ in range(a.reps + 1):            # (the first repetition warms the allocations up and is dropped)
            sc = tb.VoxelSet(ctx).Upload(*arrays).Reserve(40000)
            sc.SetOnDevice(np.array([[0, 0, 0, 1]], np.uint32))      # the scene's scratch is made by its first edit: not part of a batch's cost
            used0 = sc.Capacity()[1]
            wall.append(wall_ms(ctx, lambda: sc.SetOnDevice(d, n=n)))
            two = ctx.time_history(2)
            ev.append(sum(two)); rb.append(two[0])
            bricks_added = sc.Capacity()[1] - used0
            sc.UpdateTopGridOnDevice(); ctx.synchronize()
            top.append(ctx.time_last_ms())
            sc.free()
            sc = tb.VoxelSet(ctx).Upload(*arrays).Reserve(40000)
            sc.SetOnDevice(np.array([[0, 0, 0, 1]], np.uint32))
            wall_host.append(wall_ms(ctx, lambda: sc.SetOnDevice(recs)))
            sc.free()
            sc = tb.VoxelSet(ctx).Upload(*arrays)
            sc.SetOnDevice(np.array([[0, 0, 0, 1]], np.uint32))      # (its cell has a brick: no growth yet)
            grow.append(wall_ms(ctx, lambda: sc.SetOnDevice(d, n=n)))
            sc.free()
        ctx.free(d)
        rows.append({"records": n, "bricks_added": int(bricks_added), "event_ms": round(min(ev[1:]), 4), "readback_event_ms": round(min(rb[1:]), 4), "wall_ms": round(min(wall[1:]), 4),
                     "wall_host_records_ms": round(min(wall_host[1:]), 4), "wall_with_growth_ms": round(min(grow[1:]), 4), "top_grid_event_ms": round(min(top[1:]), 4)})
    re_up = []
    nz, ny, nx = dense.shape
    for _ in range(a.reps + 1):
        def reupload():
            h = C.c_void_p()
            tb.check(lib.tbvh_upload_voxelset_dense(ctx._h, dense.ctypes.data_as(C.c_void_p), nx, ny, nz, C.byref(h)), "tbvh_upload_voxelset_dense")
            lib.tbvh_free_scene(h)
        re_up.append(wall_ms(ctx, reupload))
    reupload_ms = round(min(re_up[1:]), 4)
    lines = [f"legocar: {arrays[1].size // 512} bricks in use; re-upload of the dense 128^3 array into a new scene + free (the path before): {reupload_ms} ms wall",
             f"{'records':>8} {'bricks+':>8} {'event ms':>9} {'read-back':>9} {'wall ms':>9} {'host recs':>10} {'+ growth':>9} {'top grid':>9} {'re-upload / wall':>17}"]
    for r in rows:
        lines.append(f"{r['records']:>8} {r['bricks_added']:>8} {r['event_ms']:>9.4f} {r['readback_event_ms']:>9.4f} {r['wall_ms']:>9.4f} {r['wall_host_records_ms']:>10.4f} {r['wall_with_growth_ms']:>9.4f} "
                     f"{r['top_grid_event_ms']:>9.4f} {reupload_ms / r['wall_ms']:>16.1f}x")
    vox_rows = voxelize_stages(ctx, a.reps)
    lines.append("")
    lines.append(f"{'voxelise':<34} {'rounds':>6} {'records':>9} {'bricks':>7} {'trace':>8} {'shade':>8} {'step':>8} {'sort':>8} {'set':>8} {'top':>7} {'wall ms':>9}")
    for r in vox_rows:
        lines.append(f"{r['scene']:<34} {r['rounds']:>6} {r['records']:>9} {r['bricks']:>7} {r['trace_ms']:>8.3f} {r['shade_ms']:>8.3f} {r['step_ms']:>8.3f} "
                     f"{r['sort_ms']:>8.3f} {r['set_ms']:>8.3f} {r['top_ms']:>7.4f} {r['wall_ms']:>9.3f}")
    text = "\n".join(lines)
    print(text)
    out = {"reupload_wall_ms": reupload_ms, "rows": rows, "voxelize": vox_rows, "reps": a.reps}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n" + json.dumps(out) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
