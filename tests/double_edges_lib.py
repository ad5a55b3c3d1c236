"""Shared pieces of the fp64 two-level edge-case tests (tests/test_double_edges_host.py, tests/test_double_edges_gpu.py): the fp64 twin of
tlas_edges_lib.py, written in float64 over RAYEX_DTYPE and INSTANCE_EX_DTYPE (nothing is cast from the fp32 records).

Two rows of BLASes, by the rule of capi_double.hip (launchDouble): a TLAS_Double with a sphere BLAS (tlas.blasSpheres, set by tbvh_upload_tlas_double)
is traced by the sphere form k_double<true, *, true>, every other by the triangle-only form k_double<false, *, true>.

    row  BLASes                            kernel
    T    BVH_Double + BVH_Double           k_double<false, *, true>    oracle_double.c
    M    SphereBVH_Double + BVH_Double     k_double<true, *, true>     oracle_custom_double.c

Meshes and spheres lie on a grid of 2^-16, the instances' centres on multiples of 5: under the axis-aligned families an axis ray through a vertex
keeps instance-space coordinates EQUAL to the vertex's, so (plane - O) is exactly 0 where rD is inf (closest hit) or 1e300 (any hit, guarded_rcp):
the NaN slab products of the closest-hit walk and the one place where guarded_rcp and a plain 1 / d give different answers.
"""
import numpy as np

import tinybvh_amd as tb

GRID = 2.0 ** -16
SPACING = 5.0
COLS = 5
FAR_OFFSET = 1.0e7
MASK_NONE, MASK_SOME, RAY_MASK_SOME = 0x0000, 0x0001 | (1 << 40), 0x00F0   # RAY_MASK_SOME shares no bit with MASK_SOME
RAY_MASK_HIGH = 1 << 40            # RayEx::mask and BLASInstanceEx::mask are uint64_t (tiny_bvh.h:758, 1472): a bit above bit 32, which only mask_some answers
N_DUP_TRIS = 50
GUARD = 1e-24                      # guarded_rcp's window (tiny_bvh.h:8336)


def _snap(a):
    return np.round(np.asarray(a, np.float64) / GRID) * GRID


# ---- BLASes ------------------------------------------------------------------------------------------------------------------------------
def bumpy(n_lon=20, n_lat=21, seed=3):
    """(3 n, 3): a closed lat-long surface around the origin, the radius modulated per vertex, 2 n_lon (n_lat - 1) = 800 triangles, at most 1.6 across.
    No vertex and no edge meets a coordinate axis (the poles are off the z axis, no ring lies in z = 0, no meridian in x = 0 or y = 0): the axis rays through an
    instance's centre tie nothing; the ties of axis_vertex are that group's own."""
    rng = np.random.default_rng(seed)
    lon = 0.37 + np.arange(n_lon) * (2 * np.pi / n_lon); lat = np.arange(1, n_lat) * (np.pi / n_lat)
    r = 0.55 + 0.2 * rng.random((n_lat - 1, n_lon))
    ring = np.stack([r * np.sin(lat)[:, None] * np.cos(lon)[None, :], r * np.sin(lat)[:, None] * np.sin(lon)[None, :], r * np.cos(lat)[:, None] * np.ones((1, n_lon))], -1)
    ring = _snap(ring) + 0.0
    top, bottom = _snap([0.013, -0.021, 0.75]), _snap([-0.017, 0.011, -0.75])
    tris = []
    for j in range(n_lon):
        k = (j + 1) % n_lon
        tris.append([top, ring[0, j], ring[0, k]])
        tris.append([bottom, ring[-1, k], ring[-1, j]])
        for i in range(n_lat - 2):
            tris.append([ring[i, j], ring[i + 1, j], ring[i + 1, k]])
            tris.append([ring[i, j], ring[i + 1, k], ring[i, k]])
    return np.ascontiguousarray(np.array(tris).reshape(-1, 3))


def soup(n=400, seed=9):
    """(3 (n + 50), 3): n random triangles in [-0.8, 0.8]^3, then the first 50 again as exact duplicates (prim ties inside one BLAS)"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-0.65, 0.65, (n, 1, 3))
    v = np.clip(_snap(c + rng.uniform(-0.15, 0.15, (n, 3, 3))), -0.8, 0.8)
    return np.ascontiguousarray(np.concatenate([v, v[:N_DUP_TRIS]]).reshape(-1, 3))


def sphere_set(n=200, seed=21):
    rng = np.random.default_rng(seed)
    return _snap(np.concatenate([rng.uniform(-0.7, 0.7, (n, 3)), rng.uniform(0.02, 0.1, (n, 1))], 1))


def tri_bounds(v):
    v = np.asarray(v).reshape(-1, 3)
    return np.concatenate([v.min(0), v.max(0)])


def sphere_bounds(s):
    return np.concatenate([(s[:, :3] - s[:, 3:4]).min(0), (s[:, :3] + s[:, 3:4]).max(0)])


# ---- instance families -------------------------------------------------------------------------------------------------------------------
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
    """(INSTANCE_EX_DTYPE records with transform / blasIdx / mask set, names): the family list of tlas_edges_lib.families, one instance each on a grid
    in the xy plane (the instance stretched by 1e3 is stretched along z, out of the plane), plus `far`, a pure translation by 1e7 along every axis,
    and `singular`, whose linear part has its z row zeroed: BLASInstanceEx::Update leaves the unscaled cofactors there (det == 0), a matrix of rank
    one that sends every ray to the same line."""
    rng = np.random.default_rng(seed)
    shear = np.eye(3); shear[0, 1] = 0.5; shear[2, 0] = -0.25
    fam = [("identity", np.eye(3)), ("translation", np.eye(3)), ("scale2", np.eye(3) * 2.0), ("scale0.5", np.eye(3) * 0.5),
           ("mirror", np.diag([-1.0, 1.0, 1.0]) @ _euler(*(rng.random(3) * 6.28)))]
    fam += [(f"rot90{'xyz'[a]}", _rot(a, 1)) for a in range(3)] + [(f"rot180{'xyz'[a]}", _rot(a, 2)) for a in range(3)]
    fam += [("thin", np.diag([1e-3, 1.0, 1.0])), ("long", np.diag([1.0, 1.0, 1e3])), ("shear", shear), ("projective", _euler(*(rng.random(3) * 6.28)) @ np.diag(0.6 + rng.random(3))),
            ("dup0", _euler(0.3, 0.5, 0.7)), ("dup1", None), ("mask_none", np.eye(3)), ("mask_some", np.eye(3) * 1.5), ("rotated", _euler(*(rng.random(3) * 6.28))),
            ("far", np.eye(3)), ("singular", np.diag([1.0, 1.0, 0.0]) @ _euler(0.4, 0.2, 0.9))]
    n = len(fam)
    T = np.zeros((n, 4, 4))
    names = [f[0] for f in fam]
    for k, (name, m) in enumerate(fam):
        if name == "dup1":
            T[k] = T[k - 1]
            continue
        T[k, :3, :3] = m; T[k, 3, 3] = 1.0
        T[k, :3, 3] = [0.0, 0.0, 0.0] if name == "identity" else [(k % COLS) * SPACING, (k // COLS) * SPACING, 0.0]
        if name == "projective":
            T[k, 3, :3] = rng.normal(0, 0.02, 3); T[k, 3, 3] = 1 + rng.normal(0, 0.05)
        if name == "far":
            T[k, :3, 3] = FAR_OFFSET
    idx = (np.arange(n) % n_blas).astype(np.uint64)
    idx[names.index("dup1")] = idx[names.index("dup0")]
    inst = tb.make_instances_ex(T, idx)
    inst["mask"][names.index("mask_none")] = MASK_NONE
    inst["mask"][names.index("mask_some")] = MASK_SOME
    return inst, names


def fill_instances(inst, bounds):
    """invTransform and the world boxes by the library's restated BLASInstanceEx::Update, in place; returns the host-built TLAS"""
    return tb.host_build_tlas_double(inst, np.ascontiguousarray(bounds, np.float64).reshape(-1, 6))


def grid_box(n):
    return np.array([-2.0, -2.0, -3.0]), np.array([(COLS - 1) * SPACING + 2, ((n - 1) // COLS) * SPACING + 2, 3.0])


def scene_diagonal(inst):
    """of the grid (the instance 1e7 away is not counted: a quarter of 1.7e7 would be no finite tmax worth the name)"""
    lo, hi = grid_box(inst.shape[0])
    return float(np.linalg.norm(hi - lo))


# ---- ray groups --------------------------------------------------------------------------------------------------------------------------
def _centres(inst):
    T = inst["transform"].reshape(-1, 4, 4)
    return T[:, :3, 3] / T[:, 3, 3:4]


def raw_rays(O, D, mask=0xFFFF):
    """records the normalising constructor cannot make: D as given, rD = 1 / D"""
    r = tb.make_rays_ex(O, np.ones_like(np.asarray(O, np.float64)), mask=mask)
    r["D"] = D
    with np.errstate(divide="ignore", invalid="ignore"):
        r["rD"] = 1.0 / r["D"]
    return r


def _world(inst, i, p):
    q = inst["transform"][i].reshape(4, 4) @ np.append(p, 1.0)
    return q[:3] / q[3]


def _surface_point(rng, prims):
    """a point on a random triangle ((3 n, 3) vertices) or the centre of a random sphere ((n, 4))"""
    if prims.shape[1] == 4:
        return prims[rng.integers(0, prims.shape[0]), :3]
    t = prims.reshape(-1, 3, 3)
    return rng.dirichlet((1.0, 1.0, 1.0)) @ t[rng.integers(0, t.shape[0])]


def nonfinite_rays(c):
    """one record each, aimed at the point c where that means anything: NaN in O, NaN in D, +inf and -inf in O, D = 0, t = NaN, +inf, 0, < 0"""
    O = np.tile(c - np.array([4.0, 0.0, 0.0]), (9, 1)); D = np.tile([1.0, 1e-3, -2e-3], (9, 1))
    O[0, 1] = np.nan; D[1, 2] = np.nan; O[2, 0] = np.inf; O[3, 2] = -np.inf; D[4] = 0.0
    r = raw_rays(O, D)
    r["t"][5:] = [np.nan, np.inf, 0.0, -1.0]
    return r


def ray_groups(inst, names, prims, seed=5, n_random=3000, n_aimed=150):
    """(rays, {group: slice}).  inst: records with the world boxes filled; prims: per blasIdx (3 n, 3) vertices or (n, 4) spheres.
      random        uniformly random rays through the grid, then n_aimed per instance from a random origin of the grid towards a point of its geometry;
                    every third ray carries RAY_MASK_SOME, which misses mask_some
      axis_outside, axis_inside    the six axis directions through every instance's centre, from 4 units outside and from the centre (D has exact zeros)
      axis_vertex   the same through a vertex (a sphere's centre) of every instance: origins on the planes of the BLAS's node boxes
      axis_tiny, axis_tiny23       axis_outside with the off-axis components -1e-25 (inside guarded_rcp's window, negative) and 1e-23 (just outside)
      inside_boxes  origins inside instance boxes
      bounce        a point of an instance's geometry carried to world space, then 1e-9 along the new direction
      mask0         ray mask 0
      mask_high     ray mask 1 << 40 alone, aimed at mask_some and at its neighbours
      nonfinite     nonfinite_rays at the identity instance"""
    rng = np.random.default_rng(seed)
    n = inst.shape[0]
    lo, hi = grid_box(n)
    parts = {}
    O = lo + rng.random((n_random, 3)) * (hi - lo)
    k = np.repeat(np.arange(n), n_aimed)
    tgt = np.array([_world(inst, i, _surface_point(rng, prims[int(inst["blasIdx"][i])])) for i in k])
    c = _centres(inst)
    Oa = np.where((names.index("far") == k)[:, None], c[k] + rng.uniform(-3, 3, (k.size, 3)), lo + rng.random((k.size, 3)) * (hi - lo))
    rnd = np.concatenate([tb.make_rays_ex(O, rng.normal(size=(n_random, 3))), tb.make_rays_ex(Oa, tgt - Oa)])
    rnd["mask"][::3] = RAY_MASK_SOME
    parts["random"] = rnd
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    D = np.tile(axes, (n, 1)); Cc = np.repeat(c, 6, 0)
    parts["axis_outside"] = raw_rays(Cc - D * 4.0, D)
    parts["axis_inside"] = raw_rays(Cc, D)
    V = np.repeat(np.array([_world(inst, i, prims[int(inst["blasIdx"][i])][(7 * i) % 50, :3]) for i in range(n)]), 6, 0)
    parts["axis_vertex"] = raw_rays(V - D * 4.0, D)
    parts["axis_tiny"] = raw_rays(Cc - D * 4.0, np.where(D == 0, -1e-25, D))
    parts["axis_tiny23"] = raw_rays(Cc - D * 4.0, np.where(D == 0, 1e-23, D))
    k = rng.integers(0, n, 1200)
    blo, bhi = inst["aabbMin"][k], inst["aabbMax"][k]
    parts["inside_boxes"] = tb.make_rays_ex(blo + (bhi - blo) * rng.random((1200, 3)), rng.normal(size=(1200, 3)))
    k = rng.integers(0, n, 1200)
    P = np.array([_world(inst, i, _surface_point(rng, prims[int(inst["blasIdx"][i])])) for i in k])
    d = rng.normal(size=(1200, 3)); d /= np.linalg.norm(d, axis=1)[:, None]
    parts["bounce"] = tb.make_rays_ex(P + d * 1e-9, d)
    m0 = tb.make_rays_ex(lo + rng.random((300, 3)) * (hi - lo), rng.normal(size=(300, 3)))
    m0["mask"] = 0
    parts["mask0"] = m0
    ms = names.index("mask_some")
    k = np.repeat([ms, ms, ms - 1, ms + 1], 50)
    tgt = np.array([_world(inst, i, _surface_point(rng, prims[int(inst["blasIdx"][i])])) for i in k])
    Oh = lo + rng.random((k.size, 3)) * (hi - lo)
    mh = tb.make_rays_ex(Oh, tgt - Oh)
    mh["mask"] = RAY_MASK_HIGH
    parts["mask_high"] = mh
    parts["nonfinite"] = nonfinite_rays(c[names.index("identity")])
    groups, at = {}, 0
    for name, r in parts.items():
        groups[name] = slice(at, at + r.shape[0]); at += r.shape[0]
    return np.concatenate(list(parts.values())), groups


def carried(rays, tmax):
    """records that carry a hit in: t = tmax (a scalar or one value per ray), u = 7, v = 9, prim = 12345, inst = 0xDEAD"""
    r = rays.copy()
    r["t"] = tmax; r["u"] = 7.0; r["v"] = 9.0; r["prim"] = 12345; r["inst"] = 0xDEAD
    return r


def bytes_of(r):
    return np.ascontiguousarray(r).view(np.uint8).reshape(-1, 128)


def differing(a, b):
    """rays whose 128-byte records differ"""
    return np.flatnonzero((bytes_of(a) != bytes_of(b)).any(1))


def changed(out, rays):
    """records a query wrote to"""
    return (bytes_of(out) != bytes_of(rays)).any(1)


def same_records(got, want, what):
    bad = differing(got, want)
    assert bad.size == 0, f"{what}: {bad.size} of {got.shape[0]} records differ, first {bad[:8].tolist()}: got {got[bad[:2]]} want {want[bad[:2]]}"


def same_bytes(got, want, what):
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    assert bad.size == 0, f"{what}: {bad.size} of {len(got)} occlusion bytes differ, first {bad[:8].tolist()}: got {got[bad[:8]]} want {want[bad[:8]]}"


def enters(inst, i, rays):
    """rays that share a mask bit with instance i and meet its world box at some t >= 0, by the reference's slab test (NaN products aside)"""
    with np.errstate(all="ignore"):
        t1 = (inst["aabbMin"][i] - rays["O"]) * rays["rD"]; t2 = (inst["aabbMax"][i] - rays["O"]) * rays["rD"]
        tmin = np.where(t1 < t2, t1, t2); tmax = np.where(t1 > t2, t1, t2)
        return (np.nanmin(tmax, 1) >= np.nanmax(tmin, 1)) & (np.nanmin(tmax, 1) >= 0) & ((rays["mask"] & inst["mask"][i]) != 0)


def guard_reached(inst, rays):
    """per ray: some instance it could enter (enters) gives an instance-space D (tinybvh_transform_vector through invTransform) with a component
    |d| <= 1e-24, the window in which guarded_rcp answers 1e300"""
    out = np.zeros(rays.shape[0], bool)
    for i in range(inst.shape[0]):
        d = rays["D"] @ inst["invTransform"][i].reshape(4, 4)[:3, :3].T
        out |= enters(inst, i, rays) & (np.abs(d) <= GUARD).any(1)
    return out


# ---- hand-made trees ---------------------------------------------------------------------------------------------------------------------
def hand_tlas(inst, leaves, shape):
    """(NODE_DBL_DTYPE nodes, uint64 instance indices) of a hand-made TLAS: leaves = [[instance, ...], ...] in order; shape "balanced" (halve the list of
    leaves) or "chain" (node = { first leaf, the rest }: custom_double_lib.chain_tree with leaves of any size).  Children are allocated in pairs and node 1
    stays unused, as in the reference's blobs; a box is the union of the instances' world boxes."""
    idx = np.array([i for leaf in leaves for i in leaf], np.uint64)
    first = np.cumsum([0] + [len(leaf) for leaf in leaves])
    if len(leaves) == 1:
        nodes = np.zeros(1, tb.NODE_DBL_DTYPE)
        nodes[0]["aabbMin"], nodes[0]["aabbMax"] = inst["aabbMin"][idx.astype(np.int64)].min(0), inst["aabbMax"][idx.astype(np.int64)].max(0)
        nodes[0]["leftFirst"], nodes[0]["triCount"] = 0, idx.size
        return nodes, idx
    recs = [[0, 0], [0, 0]]          # leftFirst, triCount
    todo = [(0, 0, len(leaves))]
    while todo:
        me, a, b = todo.pop()
        if b - a == 1:
            recs[me] = [int(first[a]), len(leaves[a])]
            continue
        c = len(recs)
        recs += [[0, 0], [0, 0]]
        recs[me] = [c, 0]
        mid = a + 1 if shape == "chain" else (a + b) // 2
        todo += [(c, a, mid), (c + 1, mid, b)]
    nodes = np.zeros(len(recs), tb.NODE_DBL_DTYPE)
    for k in range(len(recs) - 1, -1, -1):       # children have larger indices than their parent
        if k == 1:
            continue
        lf, cnt = recs[k]
        nodes[k]["leftFirst"], nodes[k]["triCount"] = lf, cnt
        if cnt:
            ii = idx[lf:lf + cnt].astype(np.int64)
            nodes[k]["aabbMin"], nodes[k]["aabbMax"] = inst["aabbMin"][ii].min(0), inst["aabbMax"][ii].max(0)
        else:
            nodes[k]["aabbMin"] = np.minimum(nodes[lf]["aabbMin"], nodes[lf + 1]["aabbMin"]); nodes[k]["aabbMax"] = np.maximum(nodes[lf]["aabbMax"], nodes[lf + 1]["aabbMax"])
    return nodes, idx


# ---- a scene per row ---------------------------------------------------------------------------------------------------------------------
class HostScene:
    """Everything of a row that needs no GPU: prims (per blasIdx), the host builders' BLAS trees, the instances after the host's Update, the host-built
    TLAS, the rays, and the oracle calls over a given tree.  row "T": bumpy + soup; row "M": spheres + soup."""

    def __init__(self, row):
        self.row = row
        self.prims = [sphere_set() if row == "M" else bumpy(), soup()]
        self.kinds = ["sph" if row == "M" else "tri", "tri"]
        self.host = [tb.host_build_custom_spheres_double(p) if k == "sph" else tb.host_build_double(p) for k, p in zip(self.kinds, self.prims)]
        self.bounds = np.stack([sphere_bounds(p) if k == "sph" else tri_bounds(p) for k, p in zip(self.kinds, self.prims)])
        self.raw_inst, self.names = families()
        self.inst = self.raw_inst.copy()
        self.tlas = fill_instances(self.inst, self.bounds)
        self.tn, self.ti = self.tlas.nodes().copy(), self.tlas.prim_idx().copy()
        self.rays, self.groups = ray_groups(self.inst, self.names, self.prims)
        self.rays.flags.writeable = False
        self.blas = [(k, h.nodes(), h.prim_idx(), p) for k, h, p in zip(self.kinds, self.host, self.prims)]
        self.tmax = (1e-9, 0.25 * scene_diagonal(self.inst))

    def fam(self, name):
        return self.names.index(name)

    def intersect(self, oracle, rays, tree=None, inst=None, rule=1):
        """oracle: OracleDouble for row T, OracleCustomDouble for row M"""
        tn, ti = tree or (self.tn, self.ti)
        inst = self.inst if inst is None else inst
        if self.row == "M":
            return oracle.tlas_intersect(tn, ti, inst, self.blas, rays, rule=rule)
        return oracle.intersect_tlas(tn, ti, inst, [b[1:] for b in self.blas], rays, rule=rule)

    def occluded(self, oracle, rays, tree=None, inst=None, rule=1):
        tn, ti = tree or (self.tn, self.ti)
        inst = self.inst if inst is None else inst
        if self.row == "M":
            return oracle.tlas_occluded(tn, ti, inst, self.blas, rays, rule=rule)
        return oracle.occluded_tlas(tn, ti, inst, [b[1:] for b in self.blas], rays, rule=rule)

    def on_sphere(self, traced):
        """records whose inst names an instance of a sphere BLAS"""
        ok = traced["inst"] < self.inst.shape[0]
        kind = np.array([k == "sph" for k in self.kinds])[self.inst["blasIdx"][np.where(ok, traced["inst"], 0).astype(np.int64)].astype(np.int64)]
        return ok & kind

    def dup_prim_hit(self, traced):
        """records whose hit lies on one of the 50 duplicated triangles of the soup (either copy)"""
        n_soup = self.prims[1].shape[0] // 3 - N_DUP_TRIS
        on_soup = self.inst["blasIdx"][np.minimum(traced["inst"], self.inst.shape[0] - 1).astype(np.int64)] == 1
        return (traced["inst"] < self.inst.shape[0]) & on_soup & ((traced["prim"] < N_DUP_TRIS) | ((traced["prim"] >= n_soup) & (traced["prim"] < n_soup + N_DUP_TRIS)))
