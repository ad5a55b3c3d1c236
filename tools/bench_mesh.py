"""Indexed against flat triangle input (tbvh_mesh; DESIGN.md par. 13): per-frame refit and device build of one mesh in both
forms, alternating in one process.  Scenes: the committed bunny (tests/golden/meshes/bunny.npz: 69 630 triangles over 34 817 positions) and the
welded Bistro stand-in (scenes.weld( scenes.street(N) )).  Per layout and form: device time of the refit (Context.time_last_ms), host-staged and
device-resident, and for the host-staged case the wall clock around a synchronise; the LBVH device build from host and from device-resident
vertices; median and min .. max over --reps repetitions.  Results go to the next free profiles/rNN_mesh.txt (or --out).
--parent-tree DIR adds the regression guard for what must not move: DIR is a checkout of the parent commit with its library built; the flat
tbvh_refit of the bunny (all three layouts) and `python bench.py --gpus 1 --steps 20 --warmup 5` are run in child processes, parent and this
tree alternating (parent, new, parent, new), and printed with the margin = the spread between the two runs of the parent itself.  Every child's
exit status is checked: the first one that is not 0 (or runs out of time) ends the guard, is reported with its stderr, nothing further is started on
the GPU, what was measured so far is still written, and the script exits with status 1.
usage: python tools/bench_mesh.py [--reps R] [--street-tris N] [--scenes bunny,street] [--out FILE] [--parent-tree DIR]"""
import argparse
import glob
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tinybvh_amd as tb  # noqa: E402
from tinybvh_amd import scenes  # noqa: E402

LAYOUTS = {"BVH_GPU": tb.LAYOUT_BVH_GPU, "BVH4_GPU": tb.LAYOUT_BVH4_GPU, "BVH8_CWBVH": tb.LAYOUT_CWBVH}


def stat(x):
    x = np.array(x)
    return f"{np.median(x):8.3f} ms  ({x.min():.3f} .. {x.max():.3f})"


def load(name, street_tris):
    if name == "bunny":
        d = np.load(os.path.join(ROOT, "tests", "golden", "meshes", "bunny.npz"))
        pos = np.zeros((d["positions"].shape[0], 4), np.float32); pos[:, :3] = d["positions"]
        return pos, np.ascontiguousarray(d["indices"].astype(np.uint32))
    return scenes.weld(scenes.street(street_tris))


# the child of the guard: flat refits only, through calls both trees have (run with cwd = the tree under test)
FLAT_REFIT_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, '.')
import tinybvh_amd as tb
d = np.load(sys.argv[1]); reps = int(sys.argv[2])
flat = np.zeros((d['indices'].size, 4), np.float32); flat[:, :3] = d['positions'][d['indices'].reshape(-1)]
frames = [flat, flat.copy()]; frames[1][:, :3] *= np.float32(1.001)
ctx = tb.Context(0)
dv = ctx.malloc(flat.nbytes)
for name, lay in (('BVH_GPU', tb.LAYOUT_BVH_GPU), ('BVH4_GPU', tb.LAYOUT_BVH4_GPU), ('BVH8_CWBVH', tb.LAYOUT_CWBVH)):
    sc = tb.LAYOUT_CLASSES[lay](ctx).Build(flat)
    host, res = [], []
    for r in range(reps + 1):
        sc.Refit(frames[r & 1]); ctx.synchronize(); a = ctx.time_last_ms()
        ctx.to_device(dv, frames[r & 1]); sc.Refit((dv, flat.shape[0] // 3), on_device=True); ctx.synchronize(); b = ctx.time_last_ms()
        if r: host.append(a); res.append(b)
    print('GUARD', name, float(np.median(host)), float(np.median(res)))
"""


class ChildFailed(RuntimeError):
    pass


def run_child(cmd, cwd, env, limit, what, say):
    """one GPU child process.  A child that does not end with status 0 — a fault, an abort, a segmentation fault, a time limit or an ordinary
    error — ends the guard: its status and the end of its stderr are reported and NOTHING further is started on the GPU."""
    try:
        r = subprocess.run(cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired as e:
        say(f"guard  STOPPED: {what} in {cwd} exceeded {limit} s; nothing further is started")
        raise ChildFailed(what) from e
    if r.returncode != 0:
        say(f"guard  STOPPED: {what} in {cwd} ended with status {r.returncode}; nothing further is started.  Its stderr ends:")
        for l in r.stderr.strip().splitlines()[-12:]:
            say("guard    | " + l)
        raise ChildFailed(what)
    return r.stdout


def guard(parent_tree, reps, say):
    """False: a child failed and the guard stopped there (what was measured until then has been printed)"""
    bunny = os.path.join(ROOT, "tests", "golden", "meshes", "bunny.npz")
    runs = []
    try:
        for label, tree in (("parent", parent_tree), ("new", ROOT), ("parent", parent_tree), ("new", ROOT)):
            env = dict(os.environ); env.pop("PYTHONPATH", None)
            out = run_child([sys.executable, "-c", FLAT_REFIT_CHILD, bunny, str(reps)], tree, env, 300, f"flat refit ({label})", say)
            vals = {m[0]: (float(m[1]), float(m[2])) for m in re.findall(r"GUARD (\S+) (\S+) (\S+)", out)}
            if len(vals) != 3:
                say(f"guard  STOPPED: flat refit ({label}) printed {len(vals)} of 3 layouts; nothing further is started")
                return False
            out = run_child([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], tree, env, 600, f"bench.py ({label})", say)
            line = [l for l in out.splitlines() if l.startswith("{")]
            j = json.loads(line[-1]) if line else {}
            if j.get("value") is None:
                say(f"guard  STOPPED: bench.py ({label}) gave no value ({str(j.get('error'))[:200]}); nothing further is started")
                return False
            runs.append((label, vals, j.get("value"), j.get("unit")))
            say(f"guard  {label:6s} flat refit ms (host-staged, resident): " + "  ".join(f"{k} {v[0]:.3f} {v[1]:.3f}" for k, v in vals.items()) + f"   bench {j.get('value')} {j.get('unit')}")
    except ChildFailed:
        return False
    par = [r for r in runs if r[0] == "parent"]; new = [r for r in runs if r[0] == "new"]
    margin = abs(par[0][2] - par[1][2])
    say(f"guard  bench: parent {par[0][2]} / {par[1][2]} (margin = their spread = {margin:.1f}), new {new[0][2]} / {new[1][2]} {runs[0][3]}")
    for k in par[0][1]:
        say(f"guard  flat refit {k}: parent {par[0][1][k][1]:.3f} / {par[1][1][k][1]:.3f} ms resident (margin {abs(par[0][1][k][1] - par[1][1][k][1]):.3f}), new {new[0][1][k][1]:.3f} / {new[1][1][k][1]:.3f}")
    return True


def next_profile():
    n = 1 + max([int(m.group(1)) for f in glob.glob(os.path.join(ROOT, "profiles", "r*")) for m in [re.match(r"r(\d+)_", os.path.basename(f))] if m] + [0])
    return os.path.join(ROOT, "profiles", f"r{n:02d}_mesh.txt")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--street-tris", type=int, default=2_832_120)
    ap.add_argument("--scenes", default="bunny,street")
    ap.add_argument("--out", default="")
    ap.add_argument("--parent-tree", default="")
    a = ap.parse_args()
    ctx = tb.Context(0)
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)

    for name in a.scenes.split(","):
        pos, idx = load(name, a.street_tris)
        flat = np.ascontiguousarray(pos[idx.reshape(-1)])
        n_tris = idx.shape[0]
        say(f"== {name}: {n_tris} triangles, {pos.shape[0]} positions; flat {flat.nbytes / 1e6:.2f} MB, indexed {pos.nbytes / 1e6:.2f} + {idx.nbytes / 1e6:.2f} MB")
        frames = [pos.copy() for _ in range(2)]
        frames[1][:, :3] *= np.float32(1.001)
        flats = [np.ascontiguousarray(f[idx.reshape(-1)]) for f in frames]
        d_flat = ctx.malloc(flat.nbytes); d_pos = ctx.malloc(pos.nbytes)
        for lname, layout in LAYOUTS.items():
            cls = tb.LAYOUT_CLASSES[layout]
            sf = cls(ctx).Build(flat); si = cls(ctx).Build(pos, indices=idx)
            res = {k: [] for k in ("flat host dev", "flat host wall", "idx host dev", "idx host wall", "flat resident dev", "idx resident dev")}
            for r in range(a.reps + 1):
                k = r & 1
                ctx.synchronize(); t0 = time.perf_counter(); sf.Refit(flats[k]); ctx.synchronize(); w = (time.perf_counter() - t0) * 1e3
                d = ctx.time_last_ms()
                ctx.synchronize(); t0 = time.perf_counter(); si.Refit(frames[k], mesh=True); ctx.synchronize(); wi = (time.perf_counter() - t0) * 1e3
                di = ctx.time_last_ms()
                ctx.to_device(d_flat, flats[k]); ctx.to_device(d_pos, frames[k])
                sf.Refit((d_flat, n_tris), on_device=True); ctx.synchronize(); dr = ctx.time_last_ms()
                si.Refit(tb.device_mesh(d_pos, pos.shape[0], n_tris)); ctx.synchronize(); dri = ctx.time_last_ms()
                if r:   # (the first repetition allocates scratch and staging)
                    for key, v in zip(res, (d, w, di, wi, dr, dri)):
                        res[key].append(v)
            for key, v in res.items():
                say(f"refit  {lname:10s} {key:18s} {stat(v)}")
            sf.free(); si.free()
        for lname in ("BVH4_GPU", "BVH8_CWBVH"):
            cls = tb.LAYOUT_CLASSES[LAYOUTS[lname]]
            tf, ti, rf, ri = [], [], [], []
            d_idx = ctx.malloc(idx.nbytes); ctx.to_device(d_idx, idx)
            ctx.to_device(d_flat, flat); ctx.to_device(d_pos, pos)
            flat_dev = tb.device_mesh(d_flat, flat.shape[0], n_tris)          # the flat form, resident: the same kernels as tbvh_build_device( on_device = 1 )
            idx_dev = tb.device_mesh(d_pos, pos.shape[0], n_tris, d_idx)
            for r in range(a.reps + 1):
                s = cls(ctx).BuildOnDevice(flat); ctx.synchronize(); x = ctx.time_last_ms(); s.free()
                s = cls(ctx).BuildOnDevice(pos, indices=idx); ctx.synchronize(); y = ctx.time_last_ms(); s.free()
                s = cls(ctx).BuildOnDevice(flat_dev); ctx.synchronize(); xr = ctx.time_last_ms(); s.free()
                s = cls(ctx).BuildOnDevice(idx_dev); ctx.synchronize(); yr = ctx.time_last_ms(); s.free()
                if r:
                    tf.append(x); ti.append(y); rf.append(xr); ri.append(yr)
            say(f"build  {lname:10s} LBVH flat, host verts (link time included)    {stat(tf)}")
            say(f"build  {lname:10s} LBVH indexed, host verts (link time included) {stat(ti)}")
            say(f"build  {lname:10s} LBVH flat, device-resident                    {stat(rf)}")
            say(f"build  {lname:10s} LBVH indexed, device-resident                 {stat(ri)}")
            ctx.free(d_idx)
        ctx.free(d_flat); ctx.free(d_pos)
    ctx.close()
    ok = True
    if a.parent_tree:
        ok = guard(os.path.abspath(a.parent_tree), a.reps, say)
    out = a.out or next_profile()
    with open(out, "w") as f:   # (also after a stopped guard: what was measured until then)
        f.write("\n".join(lines) + "\n")
    print("written:", out)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
