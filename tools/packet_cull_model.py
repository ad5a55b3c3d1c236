"""The work model behind the wave packet's child filter (tinybvh_amd/csrc/packet_cull.h), next to tools/packet_union.py which it extends: the packet traversal
of kernels_cwbvh_packet.hip restated wave-uniformly in numpy (float64) over the host builder's CWBVH blob, for random 64-ray chunks of a 4096 x 4096 camera
batch, counting per chunk
  - the nodes the wave visits and the triangles it tests,
  - the non-empty children every lane tests today, interior and leaf,
  - how many of them some ray of the wave enters (the exact per-lane test, any lane),
  - how many pass the wave's interval test (origin box x reciprocal-direction box, tmax = the wave maximum, the 1 + 2^-20 cull slack),
under three policies: 0 = as shipped (enter a child when the exact test says so), 1 = enter on the interval test alone, 2 = interval for interior children,
exact for leaves.  Policies 1 and 2 change what is visited and are NOT what the kernel does; they are here because they were weighed and lost.
The kernel's filter = policy 0's visits with the interval test in front of the exact one: its per-lane child tests are policy 0's "interval passes".

    python tools/packet_cull_model.py [scene = bistro] [chunks = 80]

CPU only.  Results: profiles/r08_packet_cull.txt."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import tinybvh_amd as tb                      # noqa: E402
from tinybvh_amd import rays as R, scenes     # noqa: E402

name = sys.argv[1] if len(sys.argv) > 1 else "bistro"
NCH = int(sys.argv[2]) if len(sys.argv) > 2 else 80
verts, _ = scenes.get(name)
h = tb.HostBVH(verts, tb.LAYOUT_CWBVH)
nodes = h.blob(0, np.uint32, 4).reshape(-1, 5, 4).copy()
tris = h.blob(1, np.uint32, 4).copy()
nodesf, trisf = nodes.view(np.float32), tris.view(np.float32)
side = 4096
cam = R.camera(*scenes.cameras(name)[0], side, side, 1, 1)
chunks = np.random.default_rng(3).choice(side * side // 64, NCH, replace=False)
SLACK = 1 + 2.0 ** -20


def bytes4(w):
    return [(int(w) >> (8 * i)) & 255 for i in range(4)]


def decode(ni):
    n, f = nodes[ni], nodesf[ni]
    ew = int(n[0, 3])
    e = [((ew >> (8 * k)) & 255) for k in range(3)]
    sc = np.array([2.0 ** (x - 256 if x > 127 else x) for x in e])
    org = f[0, :3].astype(np.float64)
    meta = bytes4(n[1, 2]) + bytes4(n[1, 3])
    qlx, qly, qlz = bytes4(n[2, 0]) + bytes4(n[2, 1]), bytes4(n[2, 2]) + bytes4(n[2, 3]), bytes4(n[3, 0]) + bytes4(n[3, 1])
    qhx, qhy, qhz = bytes4(n[3, 2]) + bytes4(n[3, 3]), bytes4(n[4, 0]) + bytes4(n[4, 1]), bytes4(n[4, 2]) + bytes4(n[4, 3])
    return ew >> 24, int(n[1, 0]), int(n[1, 1]), meta, org + np.array([qlx, qly, qlz]).T * sc, org + np.array([qhx, qhy, qhz]).T * sc


def tri_test(O, D, ti, t):
    e2, e1, v0 = (trisf[ti + k, :3].astype(np.float64) for k in range(3))
    hh = np.cross(D, e2)
    a = (hh * e1).sum(1)
    ok = np.abs(a) > 1e-15
    f = 1.0 / np.where(ok, a, 1)
    s = O - v0
    u = f * (s * hh).sum(1)
    q = np.cross(s, e1)
    v = f * (D * q).sum(1)
    tt = f * (q * e2).sum(1)
    return np.where(ok & (u >= 0) & (v >= 0) & (u + v <= 1) & (tt > 0) & (tt < t), tt, t)


def traverse(O, D, rD, policy, cnt):
    t = np.full(64, 1e30)
    oct0 = int(7 - ((rD[0, 0] < 0) * 4 + (rD[0, 1] < 0) * 2 + (rD[0, 2] < 0)))
    neg = rD[0] < 0
    Omin, Omax, rmin, rmax = O.min(0), O.max(0), rD.min(0), rD.max(0)
    S = T = 0
    stack, ni, cur = [], 0, None
    while True:
        if cur is not None:
            if cur[1] == 0:
                if not stack:
                    break
                cur = stack.pop()
            cb_, hb_, im_ = cur
            bit = hb_.bit_length() - 1
            hb_ &= ~(1 << bit)
            if hb_:
                stack.append((cb_, hb_, im_))
            slot = bit ^ oct0
            ni = cb_ + bin(im_ & ((1 << slot) - 1)).count("1")
        S += 1
        imask, cb, tbase, meta, lo, hi = decode(ni)
        near, far = np.where(neg, hi, lo), np.where(neg, lo, hi)     # (8, 3)
        tn = (near[None, :, :] - O[:, None, :]) * rD[:, None, :]
        tf = (far[None, :, :] - O[:, None, :]) * rD[:, None, :]       # (64, 8, 3)
        exact_any = (np.maximum(tn.max(2), 0) <= np.minimum(tf.min(2), t[:, None] * SLACK)).any(0)
        cn, cf = [], []
        for Oc in (Omin, Omax):
            for rc in (rmin, rmax):
                cn.append((near - Oc) * rc)
                cf.append((far - Oc) * rc)
        iv = np.maximum(np.min(cn, 0).max(1), 0) <= np.minimum(np.max(cf, 0).min(1), t.max() * SLACK)
        hb, tl = 0, []
        for c in range(8):
            m = meta[c]
            if m == 0:
                continue
            inner = (m & 0x18) == 0x18
            k_ = 0 if inner else 1
            cnt[k_] += 1
            cnt[2 + k_] += int(iv[c])
            cnt[4 + k_] += int(exact_any[c])
            ent = exact_any[c] if policy == 0 else (iv[c] if (policy == 1 or inner) else exact_any[c])
            if not ent:
                continue
            if inner:
                hb |= 1 << (((m & 31) - 24) ^ oct0)
            else:
                tl += [tbase + 3 * ((m & 31) + k) for k in range(bin(m >> 5).count("1"))]
        for ti in tl:
            T += 1
            t = tri_test(O, D, ti, t)
        cur = (cb, hb, imask)
    return S, T, t


res = {p: [] for p in (0, 1, 2)}
CNT = {p: [0] * 6 for p in (0, 1, 2)}
mixed = 0
for c in chunks:
    r = R.primary(cam, int(c) * 64, 64)
    O, D, rD = (r[k].astype(np.float64) for k in ("O", "D", "rD"))
    if len({tuple(x) for x in (rD < 0).tolist()}) > 1:
        mixed += 1
        continue
    ts = []
    for p in (0, 1, 2):
        S, T, t = traverse(O, D, rD, p, CNT[p])
        res[p].append((S, T))
        ts.append(t)
    assert np.array_equal(ts[0], ts[1]) and np.array_equal(ts[0], ts[2]), c      # the hits do not depend on the policy
for p in (0, 1, 2):
    a = np.array(res[p])
    print(f"{name} policy {p}: {len(a)} chunks, nodes per chunk {a[:, 0].mean():.1f}, triangle tests per chunk {a[:, 1].mean():.1f}")
print("mixed-octant chunks skipped:", mixed)
for p in (0, 2):
    c, n = CNT[p], len(res[p])
    print(f"policy {p} per chunk: interior children tested {c[0] / n:.1f} (interval passes {c[2] / n:.1f}, some ray enters {c[4] / n:.1f}); "
          f"leaf children tested {c[1] / n:.1f} (interval passes {c[3] / n:.1f}, some ray enters {c[5] / n:.1f})")
