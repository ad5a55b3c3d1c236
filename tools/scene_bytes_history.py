"""A fixed history over every kind of scene, for comparing what two builds of the library report as tbvh_scene_device_bytes step by step
(profiles/scene_bytes.txt).  The sibling of tools/tlas_history.py; the context synchronises after every launch.

  python tools/scene_bytes_history.py history             one line per step on stdout: the step, and device_bytes of every scene alive; meant to run under
                                                          `rocprofv3 --kernel-trace` too (tools/launch_history.py dispatches DIR reads the trace)
  python tools/scene_bytes_history.py hosttime [LAUNCHES] the host's cost of a launch call on a BVH4_GPU scene with a live 8-wide copy: wall time of LAUNCHES
                                                          (4000) back-to-back tbvh_intersect_device calls of 4096 rays, synchronised once at the end; us per
                                                          call with and without that wait (a TLAS: tools/tlas_history.py hosttime)

TBVH_TREE names another checkout whose package is loaded instead of this one's (the parent commit's, built)."""
import os
import sys
import time

import numpy as np

ROOT = os.environ.get("TBVH_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    sys.path.insert(0, ROOT)
    import tinybvh_amd as tb
    from tinybvh_amd import rays as R, scenes

    ctx = tb.Context(0)
    if sys.argv[1:2] == ["hosttime"]:
        launches = int(sys.argv[2]) if len(sys.argv) > 2 else 4000
        n = 4096
        sc = tb.BVH4_GPU(ctx).Build(scenes.blob(40_000, seed=21))
        d = ctx.malloc(n * 64)
        ctx.generate_primary(R.camera((0.0, 0.0, -4.0), (0.0, 0.0, 1.0), 64, 64, 1, 1), d, 0, n)
        plain = sc.device_bytes
        for _ in range(launches // 4):                      # warm: the copy, code objects, the second lane, the event ring all the way round
            sc.intersect_device(d, n)
        ctx.synchronize()
        assert sc.device_bytes > plain, "the scene has no 8-wide copy"
        t0 = time.perf_counter()
        for _ in range(launches):
            sc.intersect_device(d, n)
        t1 = time.perf_counter()
        ctx.synchronize()
        t2 = time.perf_counter()
        print(f"hosttime bvh4 launches {launches} rays {n} us_per_call_enqueue {(t1 - t0) / launches * 1e6:.3f} us_per_call_with_final_sync {(t2 - t0) / launches * 1e6:.3f}")
        return

    os.environ["TBVH_WIDE_COPY_MIN"] = "64"   # small scenes get their copies
    alive = {}
    step = [0]

    def say(what):
        ctx.synchronize()
        print(f"step {step[0]:3d} {what:34s} " + " ".join(f"{k} {s.device_bytes}" for k, s in alive.items()), flush=True)
        step[0] += 1

    verts = scenes.soup(2000, seed=9, extent=1.6, size=0.25)
    pos, idx = scenes.weld(verts)
    lo, hi = verts[:, :3].min(0), verts[:, :3].max(0)
    n = 4096
    d, d_occ = ctx.malloc(n * 64), ctx.malloc(n)
    ctx.to_device(d, R.random_rays(n, lo, hi, seed=5))

    def ask(s, what, times=1):
        for _ in range(times):
            s.intersect_device(d, n)
            say(what)

    # (every section frees its scenes: a number one build gets wrong stays wrong for the scene's life, and would repeat on every later line)
    # BVH_GPU and BVH4_GPU: upload, query (the 8-wide copy), update with a smaller blob, the queries that bring the copy back, update back, refit, maps
    for name, lay in (("bvh2", tb.LAYOUT_BVH_GPU), ("bvh4", tb.LAYOUT_BVH4_GPU)):
        big, small = tb.HostBVH(verts, lay, threads=1, max_leaf_tris=1), tb.HostBVH(verts, lay, threads=1)
        blob = (lambda h: (h.blob(0, np.uint32, 16), h.blob(1, np.uint32, 1).reshape(-1), verts)) if lay == tb.LAYOUT_BVH_GPU else (lambda h: (h.blob(0, np.uint32, 4),))
        s = alive[name] = tb.LAYOUT_CLASSES[lay](ctx).Upload(*blob(big)); say(name + " upload")
        ask(s, name + " query")
        s.Update(*blob(small)); say(name + " update smaller")
        ask(s, name + " query after update", 4)
        s.Update(*blob(big)); say(name + " update back")
        ask(s, name + " query after update", 4)
        s.Refit(verts); say(name + " refit")
        s.SetOpacityMicroMaps(np.full((verts.shape[0] // 3, 1), 0xFFFF, np.uint32), 4); say(name + " maps set")
        ask(s, name + " query with maps")
        s.SetOpacityMicroMaps(None, 0); say(name + " maps cleared")
        s.free(); del alive[name]

    # BVH8_CWBVH from an indexed mesh: maps, update to another topology and back, set_hybrid repeatedly, refit
    trees = []
    for leaf in (1, 3):
        h = tb.HostBVH(pos, tb.LAYOUT_BVH2_WALD, threads=1, max_leaf_tris=leaf, indices=idx)
        s = tb.BVH8_CWBVH(ctx).ConvertFromBVH2(h.bvh2_nodes(), h.bvh2_prim_idx(), pos, indices=idx)
        trees.append((s, s.download_blobs()))
    (s, blob_a), (other, blob_b) = trees
    other.free()
    alive["cwbvh"] = s; say("cwbvh converted, indexed")
    ask(s, "cwbvh query")
    s.SetOpacityMicroMaps(np.full((idx.shape[0], 1), 0xFFFF, np.uint32), 4); say("cwbvh maps set")
    s.Update(*blob_b); say("cwbvh update, another topology")
    s.Update(*blob_b); say("cwbvh update, same topology")
    s.Update(*blob_a); say("cwbvh update back")
    s.SetOpacityMicroMaps(None, 0); say("cwbvh maps cleared")
    n_nodes = blob_a[0].shape[0] // 5
    for k in (8, (n_nodes - 1) & ~7, -1, 8, -1):
        s.set_hybrid(k); say(f"cwbvh set_hybrid {k}")
    ask(s, "cwbvh query")
    s.Refit(pos, mesh=True); say("cwbvh refit, held indices")
    s.free(); del alive["cwbvh"]

    # a TLAS over the three: upload (4-wide copies), closest hit, any hit (8-wide copies, second wide tree), update, device rebuilds
    blas = [tb.BVH_GPU(ctx).Build(verts, threads=1), tb.BVH4_GPU(ctx).Build(verts, threads=1), tb.BVH8_CWBVH(ctx).Build(verts, threads=1)]
    alive.update(zip(("blas2", "blas4", "blas8"), blas)); say("three BLASes")
    grid = np.stack([np.eye(4, dtype=np.float32)] * 27)
    grid[:, :3, 3] = np.array([[x, y, z] for x in range(3) for y in range(3) for z in range(3)], np.float32) * 2.0
    inst = tb.make_instances(grid, (np.arange(27) % 3).astype(np.uint32))
    tl = alive["tlas"] = tb.TLAS(ctx).Build(inst, blas); say("tlas upload")
    ask(tl, "tlas closest hit")
    tl.occluded_device(d, n, d_occ); say("tlas any hit")
    tl.Build(inst[:9].copy(), blas); say("tlas update, fewer instances")
    tl.Build(inst, blas); say("tlas update back")
    tl.RebuildOnDevice(); say("tlas rebuild on device")
    tl.RebuildOnDevice(builder="sah"); say("tlas rebuild on device, sah")
    tl.occluded_device(d, n, d_occ); say("tlas any hit")
    blas[0].Update(blas[0].host.blob(0, np.uint32, 16), blas[0].host.blob(1, np.uint32, 1).reshape(-1), verts); say("blas2 update under the tlas")
    ask(tl, "tlas query after update", 4)
    tl.free(); del alive["tlas"]; say("tlas freed")
    for k in ("blas2", "blas4", "blas8"):
        alive.pop(k).free()

    # spheres: upload, device build, rebuild, refit
    rng = np.random.default_rng(21)
    sph = np.concatenate([rng.uniform(-0.7, 0.7, (400, 3)), rng.uniform(0.02, 0.1, (400, 1))], 1).astype(np.float32)
    alive["sph"] = tb.SphereBVH(ctx).Build(sph); say("spheres upload")
    ask(alive["sph"], "spheres query")
    alive["sph"].RebuildOnDevice(sph); say("uploaded spheres rebuilt on device")
    for builder in ("lbvh", "ploc", "sah"):
        s = alive["sph_" + builder] = tb.SphereBVH(ctx).BuildOnDevice(sph, builder=builder); say(f"spheres device build {builder}")
        s.RebuildOnDevice(sph); say(f"spheres rebuild {builder}")
        s.Refit(sph); say(f"spheres refit {builder}")
        ask(s, f"spheres query {builder}")

    # fp64: BLAS upload and refit, TLAS upload, rebuild, update
    dv = verts[:, :3].astype(np.float64)
    dbl = alive["dbl"] = tb.BVH_Double(ctx).Build(dv); say("fp64 upload")
    dbl.Refit(dv); say("fp64 refit")
    dbl.Refit(dv); say("fp64 refit again")
    inst_ex = tb.make_instances_ex(np.tile(np.eye(4), (5, 1, 1)), np.zeros(5, np.uint64))
    tdbl = alive["tdbl"] = tb.TLAS_Double(ctx).Build(inst_ex, [dbl]); say("fp64 tlas upload")
    tdbl.RebuildOnDevice(); say("fp64 tlas rebuild on device")
    tdbl.RebuildOnDevice(np.tile(np.eye(4), (5, 1, 1))); say("fp64 tlas rebuild, host transforms")
    rex = tb.make_rays_ex(rng.uniform(lo, hi, (256, 3)), rng.normal(size=(256, 3)))
    tdbl.Intersect(rex.copy()); say("fp64 tlas query")

    # voxels
    dense = (rng.uniform(size=(32, 32, 32)) < 0.2).astype(np.uint32) * 0xFFFFFF
    alive["vox"] = tb.VoxelSet(ctx).Build(dense); say("voxels upload")
    alive["vox"].IsOccluded(R.random_rays(256, (0, 0, 0), (1, 1, 1), seed=2)); say("voxels query")

    ctx.free(d); ctx.free(d_occ)
    tdbl.free()
    for k, s in alive.items():
        if k != "tdbl":
            s.free()
    ctx.close()


if __name__ == "__main__":
    main()
