"""What the watertight mode costs (tbvh_set_triangle_test; DESIGN.md par. 4.6): camera, diffuse and shadow rays of the bench scene, traced by one BVH8_CWBVH
scene at test 0 (Moeller-Trumbore, the schedules the library picks) and at test 1 (watertight), interleaved round by round.  Prints MRays/s per batch and
test — the median of the rounds, from the library's own event timing — and the ratio, and, where hipcc is at hand, the VGPR count, scratch and occupancy
of the watertight instantiations of k_cwbvh as the compiler reports them for gfx950 (--no-registers skips that compile).  Node visits per ray are not reported:
the watertight instantiations have no instrumented (STATS) form.  profiles/watertight.txt holds a run.

    python tools/watertight_bench.py [--scene bistro] [--side 2048] [--rounds 7]"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import tinybvh_amd as tb   # noqa: E402
from tinybvh_amd import rays as R   # noqa: E402
from tinybvh_amd import scenes   # noqa: E402


def kernel_resources():
    """[(any hit, micromaps, split rays, VGPRs, scratch bytes per lane, waves per SIMD)] of the WT = 1 instantiations, from hipcc's resource remarks; [] without hipcc"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return []
    src = os.path.join(ROOT, "tinybvh_amd", "csrc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-pass-failed", "-Wno-unused-value", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-c", "kernels_cwbvh.hip", "-o", os.devnull], cwd=src, capture_output=True, text=True)
    out = []
    for block in re.split(r"(?=remark: [^\n]*Function Name: )", r.stderr):
        m = re.search(r"Function Name: \S*k_cwbvhILb(\d)ELi8ELi16ELi1ELb0ELb(\d)ELi0ELi5ELi0ELi(\d+)ELi\d+ELi0ELi1EEEv", block)
        if m:
            g = lambda k: int(re.search(k + r": (\d+)", block).group(1))
            out.append((int(m.group(1)), int(m.group(2)), int(m.group(3)) != 0, g(" VGPRs"), g(r"ScratchSize \[bytes/lane\]"), g(r"Occupancy \[waves/SIMD\]")))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="bistro")
    ap.add_argument("--side", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=12, help="untimed launches per batch and test (test 0's schedule tuner settles in them)")
    ap.add_argument("--no-registers", action="store_true")
    a = ap.parse_args()
    regs = [] if a.no_registers else kernel_resources()
    for any_hit, omm, split, vgprs, scratch, waves in regs:
        print(f"k_cwbvh watertight: {'any hit    ' if any_hit else 'closest hit'} {'micromaps' if omm else '         '} {'split rays' if split else '          '} "
              f"{vgprs:3d} VGPRs  {scratch} bytes scratch  {waves} waves / SIMD")
    verts, label = scenes.get(a.scene)
    n = a.side * a.side
    ctx = tb.Context(0)
    sc = tb.BVH8_CWBVH(ctx).BuildOnDevice(verts, builder="sah")
    eye, view = scenes.cameras(a.scene)[0]
    cam = R.camera(eye, view, a.side, a.side, 1, 1)
    ext = float((verts[:, :3].max(0) - verts[:, :3].min(0)).max())
    light = (0.0, 0.9 * float(verts[:, 1].max()), 0.0)
    d_verts = ctx.malloc(verts.nbytes); ctx.to_device(d_verts, verts)
    d_prim, d_diff, d_shad = (ctx.malloc(n * 64) for _ in range(3))
    d_occ = ctx.malloc(n)
    ctx.generate_primary(cam, d_prim, 0, n)
    sc.intersect_device(d_prim, n)
    ctx.generate_shadow(d_prim, d_shad, n, light, ext * 5e-7)
    ctx.generate_bounce(d_verts, d_prim, d_diff, n, 7)
    ctx.reset_hits(d_prim, n)
    ctx.synchronize()

    def launch(kind):
        if kind == "shadow":
            sc.occluded_device(d_shad, n, d_occ)
        else:
            sc.intersect_device_fresh(d_prim if kind == "camera" else d_diff, n, 1e30)
        ctx.synchronize()
        return ctx.time_last_ms()

    kinds = ("camera", "diffuse", "shadow")
    ms = {(k, t): [] for k in kinds for t in (0, 1)}
    for t in (0, 1):
        sc.SetTriangleTest("watertight" if t else "moller-trumbore", (d_verts, verts.shape[0] // 3) if t else None)
        for k in kinds:
            for _ in range(a.warmup):
                launch(k)
    for _ in range(a.rounds):
        for t in (0, 1):
            sc.SetTriangleTest("watertight" if t else "moller-trumbore", (d_verts, verts.shape[0] // 3) if t else None)
            for k in kinds:
                launch(k)   # (the first launch after a switch is not a sample)
                ms[(k, t)].append(launch(k))
    out = {"registers": regs, "scene": label, "triangles": int(verts.shape[0] // 3), "rays": n, "rounds": a.rounds}
    for k in kinds:
        m0, m1 = float(np.median(ms[(k, 0)])), float(np.median(ms[(k, 1)]))
        out[k] = {"moller_trumbore_mrays_s": round(n / m0 / 1e3, 1), "watertight_mrays_s": round(n / m1 / 1e3, 1), "watertight_over_default": round(m0 / m1, 3),
                  "ms_default": [round(x, 3) for x in ms[(k, 0)]], "ms_watertight": [round(x, 3) for x in ms[(k, 1)]]}
        print(f"{k:8s} test 0 {n / m0 / 1e3:8.1f} MRays/s   test 1 {n / m1 / 1e3:8.1f} MRays/s   x {m0 / m1:.3f}")
    print(json.dumps(out))
    sc.free()
    ctx.close()


if __name__ == "__main__":
    main()
