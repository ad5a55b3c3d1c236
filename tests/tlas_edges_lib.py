"""Shared pieces of the two-level edge-case tests (tests/test_tlas_edges_gpu.py and the hostile-instance pin in tests/test_oracle_vs_reference.py):
the table of BLAS configurations, one per class of two-level kernel and kind of query, the hostile instance families, the ray groups traced
through them, hand-made TLAS trees (Wald nodes for the oracle, Aila-Laine nodes for TLAS.Upload) and the deep-chain scene.

Which kernel serves a configuration is the rule of tinybvh_amd/csrc/tlas_plan.h, which capi_scene.hip (reclassifyTlas) applies and capi_query.hip
(enqueueKernels) reads.  A BLAS with variant 0 is entered by closest-hit queries through its 4-wide copy (BVH_GPU, BVH8_CWBVH; made at the TLAS
upload, from 64 entries on) and by any-hit queries through its 8-wide copy (BVH_GPU, BVH4_GPU; made by the TLAS's first IsOccluded); a forced
variant on the BLAS pins the uploaded nodes for both.  Any-hit queries get a class of their own only where the 8-wide kernel serves it.  The table is
checked twice: tests/test_tlas_plan_host.py holds each row to the rule on the CPU, and the scene fixture of tests/test_tlas_edges_gpu.py asserts through
TLAS.debug_plan() that the row's live TLAS stores that family and those views (assert_kernel below).

    row  BLASes (variant)                    Intersect                         IsOccluded
    a    BVH4_GPU                            k_tlas4, uploaded nodes           k_tlas8, 8-wide copies
    a1   BVH4_GPU (1)                        k_tlas4, uploaded nodes           k_tlas4, uploaded nodes
    b    BVH8_CWBVH                          k_tlas4, 4-wide copies            k_tlas8, uploaded nodes
    c    BVH8_CWBVH (72)                     k_tlas8, uploaded nodes           k_tlas8, uploaded nodes
    d    BVH_GPU                             k_tlas4, 4-wide copies            k_tlas8, 8-wide copies
    e    BVH_GPU (1)                         k_tlas2                           k_tlas2
    f    BVH8_CWBVH (72) + BVH_GPU (1)       k_tlas8 with mixed                k_tlas8 with mixed
    g    BVH4_GPU (1) + BVH8_CWBVH (72)      k_tlas_flat_*                     k_tlas_flat_*
    h    spheres + BVH4_GPU                  k_tlas_flat_sph_*                 k_tlas_flat_sph_*

(a1 is not in the issue's table: without it no test reaches the any-hit form of k_tlas4.  In g both BLASes are pinned: an unpinned BVH4_GPU
BLAS gets an 8-wide copy from the first IsOccluded, and any-hit queries would leave the flat loop for k_tlas8.)  `grows` in the table below is the
observable for it: whether device_bytes of each BLAS grows when the TLAS is uploaded (4-wide copy) and at the first IsOccluded (8-wide copy).
"""
import ctypes as C
from collections import namedtuple

import numpy as np

import tinybvh_amd as tb
from tinybvh_amd import rays as R
from tinybvh_amd import scenes

FAR = np.float32(1e30)

# layouts / variants per BLAS; grows = per BLAS (at the TLAS upload, at the first IsOccluded); kernel classes for the deep-chain depths
Row = namedtuple("Row", "layouts variants grows intersect occluded")
L2, L4, L8, LS = tb.LAYOUT_BVH_GPU, tb.LAYOUT_BVH4_GPU, tb.LAYOUT_CWBVH, tb.LAYOUT_BVH2_WALD
CONFIGS = {
    "a": Row((L4, L4), (0, 0), ((False, True), (False, True)), "tlas4", "tlas8copy"),
    "a1": Row((L4, L4), (1, 1), ((False, False), (False, False)), "tlas4", "tlas4"),
    "b": Row((L8, L8), (0, 0), ((True, False), (True, False)), "tlas4", "tlas8"),
    "c": Row((L8, L8), (72, 72), ((False, False), (False, False)), "tlas8", "tlas8"),
    "d": Row((L2, L2), (0, 0), ((True, True), (True, True)), "tlas4", "tlas8copy"),
    "e": Row((L2, L2), (1, 1), ((False, False), (False, False)), "tlas2", "tlas2"),
    "f": Row((L8, L2), (72, 1), ((False, False), (False, False)), "tlas8mixed", "tlas8mixed"),
    "g": Row((L4, L8), (1, 72), ((False, False), (False, False)), "flat", "flat"),
    "h": Row((LS, L4), (0, 0), ((False, False), (False, False)), "flatsph", "flatsph"),
}

# a Row's kernel name in the words of TLAS.debug_plan() / tbvh_debug_tlas_plan: (family, mix, the view every BLAS is entered through, or None where it
# depends on the BLAS's layout)
KERNEL_PLAN = {"tlas4": ("Tlas4", False, None), "tlas8": ("Tlas8", False, "own"), "tlas8copy": ("Tlas8", False, "copy8"), "tlas8mixed": ("Tlas8", True, "own"),
               "tlas2": ("Tlas2", False, "own"), "flat": ("TlasFlat", False, "own"), "flatsph": ("TlasSphere", False, "own")}


def assert_kernel(kind, name):
    """kind: plan["closest"] or plan["any"] of TLAS.debug_plan(); name: a Row's `intersect` or `occluded`"""
    family, mix, view = KERNEL_PLAN[name]
    assert kind["family"] == family and kind["mix"] == mix, (name, kind)
    assert view is None or all(v == view for v in kind["views"]), (name, kind)


# ---- BLAS meshes ------------------------------------------------------------------------------------------------------------------------
def _centred(v, extent=1.6):
    v = v.copy()
    v[:, :3] -= 0.5 * (v[:, :3].min(0) + v[:, :3].max(0))
    v[:, :3] *= np.float32(extent / float((v[:, :3].max(0) - v[:, :3].min(0)).max()))
    return np.ascontiguousarray(v, np.float32)


def meshes():
    """two small meshes around the origin, at most 1.6 across: a closed bumpy surface and a triangle soup"""
    return [_centred(scenes.blob(3000, seed=3)), _centred(scenes.soup(1500, seed=9, extent=1.6, size=0.25))]


def sphere_set():
    rng = np.random.default_rng(21)
    s = np.empty((400, 4), np.float32)
    s[:, :3] = rng.uniform(-0.7, 0.7, (400, 3))
    s[:, 3] = rng.uniform(0.02, 0.1, 400)
    return s


# ---- instance families (the issue's section 2) -------------------------------------------------------------------------------------------------
SPACING = 5.0
COLS = 5
MASK_NONE, MASK_SOME, RAY_MASK_SOME = 0x0000, 0x0001, 0x00F0   # RAY_MASK_SOME shares no bit with MASK_SOME


def _rot(axis, quarter_turns):
    """rotation by quarter_turns * 90 degrees about a coordinate axis with entries exactly 0 and +-1"""
    c, s = [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)][quarter_turns % 4]
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    m = np.eye(3)
    m[i, i] = c; m[j, j] = c; m[i, j] = -s; m[j, i] = s
    return m + 0.0   # (no -0 entries)


def _euler(a, b, c):
    ca, sa, cb, sb, cc, sc = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(c), np.sin(c)
    return np.array([[cb * cc, -cb * sc, sb], [sa * sb * cc + ca * sc, -sa * sb * sc + ca * cc, -sa * cb], [-ca * sb * cc + sa * sc, ca * sb * sc + sa * cc, ca * cb]])


def families(n_blas=2, seed=17):
    """(INSTANCE_DTYPE records with transform / blasIdx / mask set, names): one instance per family on a grid in the xy plane.  The instance
    stretched by 1e3 is stretched along z, out of the grid's plane."""
    rng = np.random.default_rng(seed)
    shear = np.eye(3); shear[0, 1] = 0.5; shear[2, 0] = -0.25
    fam = [("identity", np.eye(3)), ("translation", np.eye(3)), ("scale2", np.eye(3) * 2.0), ("scale0.5", np.eye(3) * 0.5),
           ("mirror", np.diag([-1.0, 1.0, 1.0]) @ _euler(*(rng.random(3) * 6.28)))]
    fam += [(f"rot90{'xyz'[a]}", _rot(a, 1)) for a in range(3)] + [(f"rot180{'xyz'[a]}", _rot(a, 2)) for a in range(3)]
    fam += [("thin", np.diag([1e-3, 1.0, 1.0])), ("long", np.diag([1.0, 1.0, 1e3])), ("shear", shear), ("projective", _euler(*(rng.random(3) * 6.28)) @ np.diag(0.6 + rng.random(3))),
            ("dup0", _euler(0.3, 0.5, 0.7)), ("dup1", None), ("mask_none", np.eye(3)), ("mask_some", np.eye(3) * 1.5), ("rotated", _euler(*(rng.random(3) * 6.28)))]
    n = len(fam)
    T = np.zeros((n, 4, 4), np.float32)
    names = [f[0] for f in fam]
    for k, (name, m) in enumerate(fam):
        if name == "dup1":
            T[k] = T[k - 1]
            continue
        T[k, :3, :3] = m; T[k, 3, 3] = 1.0
        T[k, :3, 3] = [0.0, 0.0, 0.0] if name == "identity" else [(k % COLS) * SPACING, (k // COLS) * SPACING, 0.0]
        if name == "projective":      # as _random_instances(projective_every=...) of tests/test_oracle_vs_reference.py makes the last row
            T[k, 3, :3] = rng.normal(0, 0.02, 3); T[k, 3, 3] = 1 + rng.normal(0, 0.05)
    idx = (np.arange(n) % n_blas).astype(np.uint32)
    idx[names.index("dup1")] = idx[names.index("dup0")]
    inst = tb.make_instances(T, idx)
    inst["mask"][names.index("mask_none")] = MASK_NONE
    inst["mask"][names.index("mask_some")] = MASK_SOME
    return inst, names


def fill_instances(inst, bounds):
    """invTransform and the world boxes by the library's restated BLASInstance::Update (tbvh_host_build_tlas), in place"""
    bounds = np.ascontiguousarray(bounds, np.float32).reshape(-1, 6)
    h = C.c_void_p()
    tb.check(tb.lib.tbvh_host_build_tlas(C.c_void_p(inst.ctypes.data), inst.shape[0], C.c_void_p(bounds.ctypes.data), bounds.shape[0], C.byref(h)), "tbvh_host_build_tlas")
    tb.lib.tbvh_host_free(h)
    return inst


def mesh_bounds(vs):
    return np.stack([np.concatenate([v[:, :3].min(0), v[:, :3].max(0)]) for v in vs]).astype(np.float32)


# ---- ray groups ------------------------------------------------------------------------------------------------------------------------------
def _centres(inst):
    T = inst["transform"].reshape(-1, 4, 4).astype(np.float64)
    return (T[:, :3, 3] / T[:, 3, 3:4]).astype(np.float32)


def ray_groups(inst, tri_meshes, seed=5, n_random=6000):
    """(rays, {group: slice}): random rays through the grid; the six axis-aligned directions through every instance's centre from outside and
    from inside its box, and from outside with the other two components -1e-13 (axis_tiny); rays starting inside instance boxes; bounce-style rays leaving triangles with the reference's 1e-3 offset; a group with
    ray mask 0.  inst: records with the world boxes filled; tri_meshes: {blasIdx: vertices} of the triangle BLASes.  Every third random ray carries RAY_MASK_SOME."""
    rng = np.random.default_rng(seed)
    n = inst.shape[0]
    lo = np.array([-2.0, -2.0, -3.0], np.float32); hi = np.array([(COLS - 1) * SPACING + 2, ((n - 1) // COLS) * SPACING + 2, 3.0], np.float32)
    parts = {}
    rnd = R.random_rays(n_random, lo, hi, seed=seed)
    rnd["mask"][::3] = RAY_MASK_SOME
    parts["random"] = rnd
    c = _centres(inst)
    axes = np.concatenate([np.eye(3), -np.eye(3)]).astype(np.float32)
    D = np.tile(axes, (n, 1)); Cc = np.repeat(c, 6, 0)
    parts["axis_outside"] = tb.make_rays(Cc - D * np.float32(4.0), D)
    parts["axis_inside"] = tb.make_rays(Cc, D)
    # nearly axis-aligned: the other two components are -1e-13, inside safercp's window (|x| <= 1e-12) and NEGATIVE, so rD = -1e30 there.  The slab tests
    # themselves do not care which sign a 1e30 carries; a kernel that takes the octant from the sign of D (the 8-wide nodes) and the planes' order from rD does
    Dt = np.where(D == 0, np.float32(-1e-13), D).astype(np.float32)
    parts["axis_tiny"] = tb.make_rays(Cc - D * np.float32(4.0), Dt, normalize=False)
    k = rng.integers(0, n, 1500)
    blo, bhi = np.maximum(inst["aabbMin"][k], lo - 1), np.minimum(inst["aabbMax"][k], hi + 1)
    parts["inside_boxes"] = tb.make_rays(blo + (bhi - blo) * rng.random((1500, 3), dtype=np.float32), rng.normal(size=(1500, 3)))
    # bounce style: a point on a triangle of an instance, carried to world space, then 1e-3 along the new direction (never exactly on the triangle)
    tri_inst = np.array([i for i in range(n) if int(inst["blasIdx"][i]) in tri_meshes])
    k = tri_inst[rng.integers(0, tri_inst.size, 1500)]
    P = np.zeros((1500, 4))
    for j, i in enumerate(k):
        v = tri_meshes[int(inst["blasIdx"][i])].reshape(-1, 3, 4)
        t = v[rng.integers(0, v.shape[0])][:, :3].astype(np.float64)
        w = rng.dirichlet((1.0, 1.0, 1.0))
        p = inst["transform"][i].reshape(4, 4).astype(np.float64) @ np.append(w @ t, 1.0)
        P[j] = p / p[3]
    d = rng.normal(size=(1500, 3)); d /= np.linalg.norm(d, axis=1)[:, None]
    parts["bounce"] = tb.make_rays(P[:, :3] + d * 1e-3, d)
    m0 = R.random_rays(500, lo, hi, seed=seed + 1)
    m0["mask"] = 0
    parts["mask0"] = m0
    groups, at = {}, 0
    for name, r in parts.items():
        groups[name] = slice(at, at + r.shape[0]); at += r.shape[0]
    return np.concatenate(list(parts.values())), groups


def scene_diagonal(inst):
    n = inst.shape[0]
    return float(np.linalg.norm([(COLS - 1) * SPACING + 4, ((n - 1) // COLS) * SPACING + 4, 6.0]))


def carried(rays, tmax):
    """records that carry a hit in: t = tmax, u = 7, prim = 12345, inst = 0xDEAD"""
    r = rays.copy()
    r["t"] = np.float32(tmax); r["u"] = 7.0; r["prim"] = 12345; r["inst"] = 0xDEAD
    return r


def bytes_of(r):
    return np.ascontiguousarray(r).view(np.uint8).reshape(-1, 64)


def differing(a, b):
    """rays whose 64-byte records differ"""
    return np.flatnonzero((bytes_of(a) != bytes_of(b)).any(1))


# ---- hand-made trees -----------------------------------------------------------------------------------------------------------------------------
def wald_to_al(nodes32):
    """32-byte BVHNode array (children adjacent, tiny_bvh.h:857-866) -> 64-byte Aila-Laine nodes (tiny_bvh.h:1095-1105) numbered as BVH_GPU::ConvertFrom
    numbers them (a node's children right after everything numbered before): lmin, left, lmax, right, rmin, triCount, rmax, firstTri."""
    u = np.ascontiguousarray(nodes32).view(np.uint32).reshape(-1, 8)
    out = np.zeros((u.shape[0], 16), np.uint32)
    stack, nxt = [(0, 0)], 1
    while stack:
        w, a = stack.pop()
        if u[w, 7]:
            out[a, 11] = u[w, 7]; out[a, 15] = u[w, 3]
            continue
        l = int(u[w, 3]); r = l + 1
        out[a, 0:3] = u[l, 0:3]; out[a, 4:7] = u[l, 4:7]; out[a, 8:11] = u[r, 0:3]; out[a, 12:15] = u[r, 4:7]
        out[a, 3] = nxt; out[a, 7] = nxt + 1
        stack += [(r, nxt + 1), (l, nxt)]
        nxt += 2
    return np.ascontiguousarray(out[:nxt])


def hand_tlas(inst, idx, leaves, shape):
    """Wald nodes [N, 8] uint32 of a hand-made TLAS over inst[idx[...]]: leaves = [(first, count), ...] into idx, in order; shape "balanced"
    (halve the list of leaves) or "caterpillar" (node = { first leaf, the rest }).  Node 1 stays unused, children are allocated in pairs, boxes are
    the unions of the instances' world boxes."""
    nodes = [[0, 0, None], [0, 0, None]]          # leftFirst, triCount, (leaf range) or None
    todo = [(0, 0, len(leaves))]
    while todo:
        me, a, b = todo.pop()
        if b - a == 1:
            nodes[me] = [leaves[a][0], leaves[a][1], None]
            continue
        c = len(nodes)
        nodes += [[0, 0, None], [0, 0, None]]
        nodes[me] = [c, 0, None]
        mid = a + 1 if shape == "caterpillar" else (a + b) // 2
        todo += [(c, a, mid), (c + 1, mid, b)]
    out = np.zeros((len(nodes), 8), np.uint32)
    f = out.view(np.float32)
    for k in range(len(nodes) - 1, -1, -1):       # children have larger indices than their parent
        if k == 1:
            continue
        lf, cnt, _ = nodes[k]
        out[k, 3] = lf; out[k, 7] = cnt
        if cnt:
            ii = idx[lf:lf + cnt]
            f[k, 0:3] = inst["aabbMin"][ii].min(0); f[k, 4:7] = inst["aabbMax"][ii].max(0)
        else:
            f[k, 0:3] = np.minimum(f[lf, 0:3], f[lf + 1, 0:3]); f[k, 4:7] = np.maximum(f[lf, 4:7], f[lf + 1, 4:7])
    return out


# ---- the deep chain under a TLAS -----------------------------------------------------------------------------------------------------------
# Entries the -x rays of test_deep_tree.py leave pending per level of chain_bvh2, by the node form the kernel walks:
#   4-wide (k_tlas4, BVH4_GPU in the flat loop): a wide node holds 3 clumps and the rest of the chain, the three clumps are pushed one entry each: 3 per 3 levels = 1
#   8-wide (k_tlas8, BVH8_CWBVH in the flat loop): one group entry for a node's 7 pending clumps: 1 per 7 levels
#   2-wide (k_tlas2, BVH_GPU in k_tlas8 with mixed / the flat loop): the clump of each level: 1
# Capacity beyond the LDS part: 232 32-bit entries per lane by default (capi_context.hip), 116 where an entry is 8 bytes (k_tlas8, the flat loops).
# The window is [2 * LDS_N, 3/4 * capacity] entries:
#   k_tlas4     LDS_N 12, 32-bit entries: 24 .. 174   depth 100 -> ~100 (uploaded BVH4_GPU nodes; a 4-wide copy of another layout has at most as many pending per level)
#   k_tlas2     LDS_N 16, 32-bit entries: 32 .. 174   depth 100 -> 100
#   k_tlas8     LDS_N 8 / 10 / 12, 8-byte entries: 24 .. 87   BVH8_CWBVH depth 350 -> 50; an 8-wide copy of a 4- or 2-wide chain, whose wide nodes
#               may hold fewer clumps: depth 250 -> 36 (7 clumps per node) .. 83 (3 per node); BVH_GPU under `mixed`: depth 50 -> 50
#   flat loops  LDS_N 12, 8-byte entries: 24 .. 87    BVH4_GPU depth 50 -> 50, BVH8_CWBVH depth 350 -> 50
# The TLAS level adds at most three entries beneath (the instances of DeepScene below).
DEEP_DEPTH = {
    ("tlas4", L4): 100, ("tlas4", L8): 100, ("tlas4", L2): 100,
    ("tlas2", L2): 100,
    ("tlas8", L8): 350, ("tlas8copy", L4): 250, ("tlas8copy", L2): 250,
    ("tlas8mixed", L8): 350, ("tlas8mixed", L2): 50,
    ("flat", L4): 50, ("flat", L8): 350,
    ("flatsph", L4): 50,
}


def deep_blas(ctx, layout, variant, depth):
    from test_deep_tree import chain_bvh2
    n2, pi, verts = chain_bvh2(depth)
    if layout == L2:
        sc = tb.BVH_GPU(ctx).Upload(wald_to_al(n2), pi, verts)
    else:
        sc = tb.LAYOUT_CLASSES[layout](ctx).ConvertFromBVH2(n2, pi, verts)
    if variant:
        sc.set_variant(variant)
    return sc


def chain_bounds(depth):
    from test_deep_tree import CLUMP
    return [0.0, -1.0, -1.0, float(np.float32(depth) + np.float32(CLUMP - 1) * np.float32(0.1)), 3.0, 3.0]


def deep_scene(bounds, use, d):
    """Instances of chain BLAS `use` (depth d; bounds: the root box of every BLAS) lined up along x, met by rays travelling in -x in the order A, B, C:
         A  translation only; covers y + z <= 2 of its box [-1, 3]^2
         B  diag(1, -1, -1), translated by (.., 3, 3): covers y + z >= 4 of the box [0, 4]^2
         C  scale 2: covers y + z <= 4 of the box [-2, 6]^2
    plus one instance of every other BLAS 1000 units off the rays' path (the TLAS keeps its kernel class).  The hand-made TLAS is
    { A, { B, { C, others } } }: while A is traversed the rest is pending beneath (base >= 1).  Ray groups (origin y, z; first triangle met):
    (0.05 .. 0.6, 0.2) A;  (2.5, 2.5) crosses A's whole chain inside every node box, outside every triangle, then B;  (1.5, 1.5) crosses A and B, then C.
    Returns (instances, wald nodes, idx, rays, expected t, expected inst, tolerance); the expected prim is the chain's last triangle."""
    from test_deep_tree import CLUMP
    length =np.float32(d) + np.float32(CLUMP - 1) * np.float32(0.1)     # x of the last triangle in BLAS space
    gap = 4
    xc, xb = 0, 2 * (d + 1) + gap
    xa = xb + (d + 1) + gap
    x0 = float(xa + (d + 1) + gap)
    T = [np.eye(4), np.eye(4), np.eye(4)]
    T[0][:3, 3] = [xa, 0, 0]
    T[1][:3, :3] = np.diag([1.0, -1.0, -1.0]); T[1][:3, 3] = [xb, 3, 3]
    T[2][:3, :3] = np.eye(3) * 2.0; T[2][:3, 3] = [xc, 0, 0]
    blas_idx = [use, use, use]
    for k in range(len(bounds)):
        if k != use:
            M = np.eye(4); M[:3, 3] = [0, 1000 + 10 * k, 0]
            T.append(M); blas_idx.append(k)
    inst = tb.make_instances(np.array(T, np.float32), np.array(blas_idx, np.uint32))
    fill_instances(inst, bounds)
    idx = np.arange(inst.shape[0], dtype=np.uint32)
    wald = hand_tlas(inst, idx, [(k, 1) for k in range(inst.shape[0])], "caterpillar")
    n = 128
    O = np.zeros((3 * n, 3), np.float32); O[:, 0] = x0
    O[:n, 1] = np.linspace(0.05, 0.6, n, dtype=np.float32); O[:n, 2] = 0.2
    O[n:2 * n, 1] = 2.5; O[n:2 * n, 2] = 2.5
    O[2 * n:, 1] = 1.5; O[2 * n:, 2] = 1.5
    D = np.zeros((3 * n, 3), np.float32); D[:, 0] = -1.0
    rays = tb.make_rays(O, D)
    t = np.repeat(np.array([x0 - (xa + float(length)), x0 - (xb + float(length)), x0 - (xc + 2.0 * float(length))], np.float32), n)
    tol = np.repeat(np.array([2e-3, 2e-3, 2e-3 * 2.0], np.float32), n)   # test_deep_tree.py's tolerance, scaled by the instance's scale
    return inst, wald, idx, rays, t, np.repeat(np.array([0, 1, 2], np.uint32), n), tol
