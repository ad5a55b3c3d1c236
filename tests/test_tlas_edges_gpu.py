"""The two-level (TLAS) kernels held to the edge cases the single-level kernels are held to (tests/test_gpu_parity.py, tests/test_deep_tree.py):
finite tmax and carried-in hits with misses left untouched over all 64 bytes, hostile instance transforms (mirrored, exact quarter and half turns,
strong anisotropy, shear, the projective w != 1 divide), exact ties between instances, instance and ray masks, ragged and empty batches, non-finite
rays, BLAS stacks that spill while TLAS entries lie beneath them, and hand-made TLAS shapes through TLAS.Upload.

Every test runs over the rows of tests/tlas_edges_lib.py (CONFIGS), one per class of two-level kernel and kind of query:

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

(the rule is tinybvh_amd/csrc/tlas_plan.h; tests/test_tlas_plan_host.py holds these rows to it on the CPU).  The scene fixture asserts through
TLAS.debug_plan() that each row's TLAS has stored the kernel family and views the table names, for Intersect at the upload and for IsOccluded after the first
one, and, where a copy decides the class, that device_bytes of the BLAS grows exactly when that copy is made, as tests/test_bvh_gpu_wide_copy.py does.

The expectation is the restated BVH::IntersectTLAS under the library's tie rule (oracle/tbvh_oracle.c), pinned on these very instances and rays
against the real reference by test_restated_tlas_traversal_equals_the_reference_on_hostile_instances.  Row h takes the TLAS restatement of
tests/oracle_custom.c instead, which walks records as given, so finite tmax and carried-in records run on row h too, in every test; its triangle
arithmetic is compiled without contraction, so row h is compared the way tests/test_custom_gpu.py compares a mixed TLAS: sphere hits byte for byte,
triangle hits under compare_hits with at most 2 hit / miss differences.

A finding these tests made, which is the reference's and not a kernel's: under a PROJECTIVE instance transform BVH::IntersectTLAS carries the origin
through the divide by w and the direction through the linear part alone (tiny_bvh.h:3329-3330), so the instance-space ray is not the preimage of the world
ray and can meet geometry although the world ray misses the instance's world box.  Whether such a hit is reported then depends on how tight the culling
boxes above the instance are: the oracle on the exact boxes of the host-built tree culls it, a kernel walking the outward-quantised boxes of a wide TLAS
may enter the instance and report it (seen in rows c and f after RebuildOnDevice, on 2 of 9860 rays grazing the box within 0.03).  Both records are
BVH::IntersectTLAS's, on different but equally valid trees.  So on the hostile-instance scene a ray's expectation is the oracle's record on the tree
the test names, or, where that differs BECAUSE OF THE PROJECTIVE INSTANCE, the oracle's record with no TLAS box in the way (Scene.loose: one leaf
listing every instance) if the kernel reports exactly that record.  Nothing else is admitted, and every affine family is held to the one record."""
import numpy as np
import pytest

import tinybvh_amd as tb
from tinybvh_amd import rays as R
from oracle_lib import compare_hits, tlas_intersect
from custom_lib import cu_oracle  # noqa: F401  (fixture)
from test_tlas import check, grid_instances
import tlas_edges_lib as E

pytestmark = pytest.mark.gpu

ROWS = list(E.CONFIGS)


class Scene:
    """The BLASes of one row, the hostile-instance TLAS over them, its rays and the oracle's records for them (computed once)."""

    def __init__(self, ctx, oracle, cu, key, on_upload=None):
        """on_upload(scene): called once the TLAS is uploaded and the expectation computed, before the TLAS's first query (tests/test_tlas_plan_gpu.py)"""
        self.key, self.row, self.ctx, self.oracle, self.cu = key, E.CONFIGS[key], ctx, oracle, cu
        row = self.row
        vs = E.meshes()
        self.blas, self.desc, self.tri_meshes = [], [], {}
        for k, (lay, var) in enumerate(zip(row.layouts, row.variants)):
            if lay == E.LS:
                sph = E.sphere_set()
                b = tb.SphereBVH(ctx).Build(sph)
                self.desc.append(("sph", b.nodes, b.prim_idx, sph))
            else:
                b = tb.LAYOUT_CLASSES[lay](ctx).Build(vs[k])
                if var:
                    b.set_variant(var)          # before any TLAS: no copy is ever made of a pinned BLAS
                self.tri_meshes[k] = vs[k]
                self.desc.append(("tri", b.host.bvh2_nodes(), b.host.bvh2_prim_idx(), vs[k]))
            self.blas.append(b)
        self.spheres = E.LS in row.layouts
        self.inst, self.names = E.families(len(self.blas))
        self.projective, self._loose = self.names.index("projective"), {}
        before = [b.device_bytes for b in self.blas]
        self.tlas = tb.TLAS(ctx).Build(self.inst, self.blas)
        self.bounds = self.tlas._blas_bounds(self.blas)
        after_build = [b.device_bytes for b in self.blas]
        E.assert_kernel(self.tlas.debug_plan()[1]["closest"], row.intersect)      # the row reaches the kernel it is named after (tlas_plan.h)
        self.rays, self.groups = E.ray_groups(self.inst, self.tri_meshes)
        self.diag = E.scene_diagonal(self.inst)
        self.want = self.expect(self.rays)
        if on_upload:
            on_upload(self)
        self.tlas.IsOccluded(self.rays[:64])     # the TLAS's first any-hit query makes the 8-wide copies
        after_occ = [b.device_bytes for b in self.blas]
        plan = self.tlas.debug_plan()[1]
        E.assert_kernel(plan["closest"], row.intersect); E.assert_kernel(plan["any"], row.occluded)
        for k, (at_build, at_occ) in enumerate(row.grows):   # the observable for the kernel class (module docstring)
            assert (after_build[k] > before[k]) == at_build, (key, k, "4-wide copy at the TLAS upload", before[k], after_build[k])
            assert (after_occ[k] > after_build[k]) == at_occ, (key, k, "8-wide copy at the first IsOccluded", after_build[k], after_occ[k])

    def host_tree(self):
        h = self.tlas.host
        return h.blob(2, np.uint32, 8), h.blob(1, np.uint32, 1)

    def expect(self, rays, nodes32=None, idx=None, inst=None):
        if nodes32 is None:
            nodes32, idx = self.host_tree()
        inst = self.inst if inst is None else inst
        with np.errstate(all="ignore"):
            if self.spheres:
                return self.cu.tlas_intersect(nodes32, idx, inst, self.desc, rays, rule=1)
            return tlas_intersect(self.oracle, nodes32, idx, inst, [(n, p, v) for _, n, p, v in self.desc], rays)

    def loose(self, batch):
        """The oracle's records with no TLAS box in the way: one leaf listing every instance (a root leaf is entered untested)."""
        key = hash(batch.tobytes())
        if key not in self._loose:
            n = self.inst.shape[0]
            idx = np.arange(n, dtype=np.uint32)
            self._loose[key] = self.expect(batch, E.hand_tlas(self.inst, idx, [(0, n)], "balanced"), idx)
        return self._loose[key]

    def effective(self, got, want, batch):
        """`want`, with the box-free records (loose) for the rays on which the PROJECTIVE instance makes the reference's own answer depend on the
        culling boxes (module docstring) and the kernel reports exactly the box-free record."""
        lo = self.loose(batch)
        cand = E.differing(lo, want)
        cand = cand[lo["inst"][cand] == self.projective]
        take = cand[(E.bytes_of(got[cand]) == E.bytes_of(lo[cand])).all(1)] if cand.size else cand
        if take.size:
            print(f"row {self.key}: {take.size} of {cand.size} rays whose record depends on the projective instance's box take the box-free record")
            want = want.copy(); want[take] = lo[take]
        return want

    def compare(self, got, want, batch, inst=None):
        """got against the oracle's records for `batch`: the records the oracle changed under check() of tests/test_tlas.py (row h: see the module
        docstring), the ones it left alone byte-identical to the input.  Returns (rays the oracle changed, rays it left alone, the records compared with)."""
        if inst is None:
            want = self.effective(got, want, batch)
        inst = self.inst if inst is None else inst
        hit, miss = self._compare(got, want, batch, inst)
        return hit, miss, want

    def _compare(self, got, want, batch, inst):
        hit, changed_got = E.differing(want, batch), E.differing(got, batch)
        miss = np.setdiff1d(np.arange(batch.shape[0]), hit)
        false_hits = np.intersect1d(miss, changed_got)
        if self.spheres:
            sph = want["inst"][hit] < 0xFFFFFFFF
            sph &= inst["blasIdx"][np.minimum(want["inst"][hit], inst.shape[0] - 1)] == self.row.layouts.index(E.LS)
            assert E.differing(got[hit][sph], want[hit][sph]).size == 0
            c = compare_hits(got[hit], want[hit])
            assert c["hitmiss"] + false_hits.size <= 2 and c["prim_real"] == 0 and c["t_bad"] == 0, (c, false_hits)
            return hit, miss
        # a ray the oracle leaves alone and the kernel reports at t == 0 is check()'s onsurf class: within the same cap of 4
        onsurf = false_hits[got["t"][false_hits] == 0]
        assert false_hits.size == onsurf.size, ("records of missed rays changed", false_hits[:8], got[false_hits[:8]])
        c = check(got[hit], want[hit]) if hit.size else {"onsurf": 0}
        assert c["onsurf"] + onsurf.size <= 4, (c, onsurf)
        return hit, miss

    def occluded_differs(self, occ, want, batch, inst=None):
        """rays whose IsOccluded differs from "the oracle's closest hit lies within tmax" (with or without the projective instance's box in the way,
        where that changes the answer)"""
        ok = occ.astype(bool) == (want["t"] < batch["t"])
        if inst is None:
            lo = self.loose(batch)
            ok |= (lo["inst"] == self.projective) & (occ.astype(bool) == (lo["t"] < batch["t"]))
        return int((~ok).sum())

    def close(self):
        self.tlas.free()
        for b in self.blas:
            b.free()


@pytest.fixture(scope="module", params=ROWS)
def scene(request, ctx, oracle_ties, cu_oracle):
    s = Scene(ctx, oracle_ties, cu_oracle, request.param)
    yield s
    s.close()


def test_hostile_instances(scene):
    s = scene
    rays, want, names = s.rays, s.want, s.names
    assert int((want["t"] == 0).sum()) <= 4                      # the oracle alone: rays that start exactly on a triangle (check()'s onsurf cap)
    got = s.tlas.Intersect(rays.copy())
    hit, miss, want = s.compare(got, want, rays)
    assert hit.size > 2000 and miss.size > 2000
    if not s.spheres:
        check(got, want)
    occ = s.tlas.IsOccluded(rays.copy())
    assert s.occluded_differs(occ, want, rays) <= 2
    hit_inst = set(got["inst"][hit].tolist())
    n = s.inst.shape[0]
    none, d0, d1 = names.index("mask_none"), names.index("dup0"), names.index("dup1")
    assert hit_inst >= set(range(n)) - {none, d1}, sorted(set(range(n)) - hit_inst)   # every family is hit, the projective one included
    assert none not in hit_inst                                   # mask 0: never entered
    assert d1 not in hit_inst and int((got["inst"][hit] == d0).sum()) > 20   # an exact tie between instances: the smaller index wins
    g = s.groups["mask0"]
    assert np.array_equal(E.bytes_of(got[g]), E.bytes_of(rays[g])) and not occ[g].any()
    some = names.index("mask_some")                               # rays sharing no mask bit with it never report it; the others do
    masked = rays["mask"] == E.RAY_MASK_SOME
    assert not np.any(got["inst"][hit][masked[hit]] == some) and np.any(got["inst"][hit][~masked[hit]] == some)
    for name in ("axis_outside", "axis_inside", "axis_tiny", "inside_boxes", "bounce"):
        g = s.groups[name]
        assert int((want["t"][g] < 1e30).sum()) > 20, name       # every group meets geometry


def test_device_rebuild(scene):
    s = scene
    host_records = s.inst.copy()
    try:
        s.tlas.RebuildOnDevice()
        nodes, idx, dev = s.tlas.Download()
        for f in ("transform", "invTransform", "aabbMin", "aabbMax", "blasIdx", "mask"):
            assert np.array_equal(dev[f].view(np.uint32), host_records[f].view(np.uint32)), f
        got = s.tlas.Intersect(s.rays.copy())
        s.compare(got, s.want, s.rays)                            # the TLAS's shape does not change a record
        assert s.occluded_differs(s.tlas.IsOccluded(s.rays.copy()), s.want, s.rays) <= 2
    finally:
        s.tlas.Build(s.inst, s.blas)                              # the host-built tree again for the other tests


def test_finite_tmax_and_carried_in_records(scene):
    s, ctx = scene, scene.ctx
    tmax = np.float32(0.3 * s.diag)
    batch = E.carried(s.rays, tmax)
    want = s.expect(batch)
    got = s.tlas.Intersect(batch.copy())
    hit, miss, want = s.compare(got, want, batch)
    assert hit.size > 300 and miss.size > 300
    assert np.all(got["inst"][miss] == 0xDEAD) and np.all(got["u"][miss] == 7.0) and np.all(got["prim"][miss] == 12345)
    assert s.occluded_differs(s.tlas.IsOccluded(batch.copy()), want, batch) <= 2
    # the hit distance found as tmax, the rest of the record junk
    again = got.copy()
    again["u"] = 7.0; again["v"] = -3.0; again["prim"] = 12345; again["inst"] = 0xDEAD
    s.compare(s.tlas.Intersect(again.copy()), s.expect(again), again)
    # tmax = 0: nothing can be closer
    zero = E.carried(s.rays, 0.0)
    s.compare(s.tlas.Intersect(zero.copy()), s.expect(zero), zero)
    # intersect_device_fresh( tmax ) = tmax written into the records (tbvh_reset_hits_device), then intersect_device
    n = batch.shape[0]
    d = ctx.malloc(n * 64)
    try:
        a, b = np.zeros_like(batch), np.zeros_like(batch)
        ctx.to_device(d, batch); ctx.reset_hits(d, n, float(tmax)); s.tlas.intersect_device(d, n); ctx.synchronize(); ctx.from_device(a, d)
        ctx.to_device(d, batch); s.tlas.intersect_device_fresh(d, n, float(tmax)); ctx.synchronize(); ctx.from_device(b, d)
    finally:
        ctx.free(d)
    assert np.array_equal(E.bytes_of(a), E.bytes_of(b))
    fresh = batch.copy(); fresh["u"] = 0; fresh["v"] = 0; fresh["prim"] = 0
    s.compare(a, s.expect(fresh), fresh)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 127, 1000])
def test_batch_shapes(scene, n):
    s = scene
    pool = np.flatnonzero(s.want["t"] != 0)                       # (a ray that starts exactly on a triangle is check()'s onsurf class, not a byte-for-byte one)
    pick = pool[:: max(1, pool.size // 1000)][:n]
    batch = np.ascontiguousarray(s.rays[pick])
    got = s.tlas.Intersect(batch.copy())
    occ = s.tlas.IsOccluded(batch.copy())
    assert got.shape[0] == n and occ.shape[0] == n
    if n == 0:
        return
    _, _, want = s.compare(got, s.want[pick], batch)
    if not s.spheres:
        assert np.array_equal(E.bytes_of(got), E.bytes_of(want)), E.differing(got, want)
    assert s.occluded_differs(occ, want, batch) <= 2
    if n >= 63:
        assert 0 < int((want["t"] < 1e30).sum()) < n              # both kinds of ray in the batch


def test_non_finite_rays(scene):
    """The classes of test_hostile_geometry_and_rays (tests/test_gpu_parity.py) mixed into a batch of finite rays: the launch returns, the finite rays
    are not disturbed, zero-length directions (rD = 1e30) and infinite origins give the oracle's records; NaN components and infinite direction
    components are unspecified (include/tinybvh_amd.h): their differences are printed."""
    s = scene
    lo, hi = (-2, -2, -3), ((E.COLS - 1) * E.SPACING + 2, 3 * E.SPACING + 2, 3)
    bad = R.random_rays(640, lo, hi, seed=6)
    bad["D"][0:128, :3] = 0.0; bad["rD"][0:128, :3] = np.float32(1e30)
    bad["D"][128:256, 0] = np.nan; bad["rD"][128:256, 0] = np.nan
    bad["O"][256:384, 1] = np.nan
    bad["O"][384:512, 2] = np.inf
    bad["D"][512:640, 1] = np.inf; bad["rD"][512:640, 1] = 0.0
    finite = s.rays[:3200]
    mixed = np.concatenate([bad, finite])
    alone = s.tlas.Intersect(finite.copy())
    got = s.tlas.Intersect(mixed.copy())                          # returns
    assert np.array_equal(E.bytes_of(got[640:]), E.bytes_of(alone))
    want = s.expect(mixed)
    same = (got["prim"][:640] == want["prim"][:640]) & ((got["t"][:640] == want["t"][:640]) | (np.isnan(got["t"][:640]) & np.isnan(want["t"][:640])))
    per_class = [int((~same[k:k + 128]).sum()) for k in range(0, 640, 128)]
    print("non-finite rays that differ from the restated reference, per class (zero D, NaN D, NaN O, inf O, inf D):", per_class)
    assert per_class[0] == 0 and per_class[3] == 0, per_class
    assert s.tlas.IsOccluded(mixed.copy()).shape[0] == mixed.shape[0]


# ---- hand-made TLAS shapes through TLAS.Upload -------------------------------------------------------------------------------------------------
def _upload_and_check(s, inst, idx, wald, rays):
    tl = tb.TLAS(s.ctx).Upload(E.wald_to_al(wald), idx, inst, s.blas)
    try:
        want = s.expect(rays, wald, idx, inst)
        got = tl.Intersect(rays.copy())
        hit, _, _ = s.compare(got, want, rays, inst)
        if not s.spheres:
            check(got, want)
        assert s.occluded_differs(tl.IsOccluded(rays.copy()), want, rays, inst) <= 2
        return got, hit
    finally:
        tl.free()


@pytest.mark.parametrize("shape", ["one_leaf", "leaves_1_2_5_64", "permuted"])
def test_tlas_shapes(scene, shape):
    """343 small instances under a TLAS no builder of the library makes: one leaf listing all of them; leaves of 1, 2, 5 and 64 instances; the same
    with a tlasIdx that is a random permutation (so a leaf's instances lie all over the scene).  The oracle walks the same nodes and index array."""
    s = scene
    inst = E.fill_instances(grid_instances(7, 0.3, 4, n_blas=len(s.blas)), s.bounds)
    n = inst.shape[0]
    idx = np.arange(n, dtype=np.uint32)
    if shape == "one_leaf":
        leaves = [(0, n)]
    else:
        leaves, at = [], 0
        while at < n:
            c = min((1, 2, 5, 64)[len(leaves) % 4], n - at)
            leaves.append((at, c)); at += c
        if shape == "permuted":
            idx = np.random.default_rng(3).permutation(n).astype(np.uint32)
    wald = E.hand_tlas(inst, idx, leaves, "balanced")
    rays = R.random_rays(4000, (-1, -1, -1), (13, 13, 13), seed=12)
    got, hit = _upload_and_check(s, inst, idx, wald, rays)
    assert hit.size > 500 and len(np.unique(got["inst"][hit])) > 150


# instances on a line, the TLAS a caterpillar with one instance per level whose near child (for rays travelling in -x) is the rest of the chain: every level
# leaves its instance pending.  Entries per level: k_tlas4 1 (the 4-wide TLAS lists 3 instances and the rest per node, one entry each), k_tlas2 and the flat
# loops 1, k_tlas8 at most 2 per 7 levels (a node's parked instance group and its interior child).  Windows as for DEEP_DEPTH in the helper:
#   k_tlas4 24 .. 174, k_tlas2 32 .. 174, k_tlas8 24 .. 87, flat loops 24 .. 87 (8-byte entries).
# Rows whose two queries walk different TLAS forms (k_tlas4 and k_tlas8) need a length inside both windows: 170 -> 170 and 24 .. 49.
CATERPILLAR = {"a": 170, "b": 170, "d": 170, "a1": 100, "e": 100, "c": 250, "f": 250, "g": 60, "h": 60}


def test_caterpillar_tlas(scene):
    s = scene
    n = CATERPILLAR[s.key]
    T = np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))
    T[:, :3, :3] *= np.float32(0.5)
    T[:, 0, 3] = 2.0 * np.arange(n)
    inst = E.fill_instances(tb.make_instances(T, (np.arange(n) % len(s.blas)).astype(np.uint32)), s.bounds)
    idx = np.arange(n, dtype=np.uint32)
    wald = E.hand_tlas(inst, idx, [(k, 1) for k in range(n)], "caterpillar")
    rng = np.random.default_rng(8)
    m = 512
    O = np.zeros((m, 3), np.float32); D = np.zeros((m, 3), np.float32)
    O[:, 0] = np.where(np.arange(m) % 2 == 0, 2.0 * n + 3, -3.0); D[:, 0] = np.where(np.arange(m) % 2 == 0, -1.0, 1.0)
    O[:, 1:] = rng.uniform(-0.3, 0.3, (m, 2)); D[:, 1:] = rng.uniform(-1e-3, 1e-3, (m, 2))
    rays = tb.make_rays(O, D)
    got, hit = _upload_and_check(s, inst, idx, wald, rays)
    assert hit.size > m // 2


# ---- a BLAS deeper than the LDS part of the stack, under a TLAS ------------------------------------------------------------------------------------
@pytest.mark.parametrize("query", ["intersect", "occluded"])
@pytest.mark.parametrize("key", ROWS)
def test_deep_blas_under_a_tlas(ctx, key, query):
    """chain_bvh2 (tests/test_deep_tree.py) as the BLAS of instances lined up along the rays (tlas_edges_lib.deep_scene): the BLAS part of the stack
    spills while TLAS entries lie beneath it (base >= 1), and rays that cross a whole chain without touching a triangle return to the TLAS level from a
    spilled stack and hit in the next instance.  Exact transforms, analytic expectations.  The chain's depth is chosen per kernel (DEEP_DEPTH)."""
    from test_deep_tree import CLUMP
    row = E.CONFIGS[key]
    kernel = row.intersect if query == "intersect" else row.occluded
    blas, bounds, chains = [], [], []
    for k, (lay, var) in enumerate(zip(row.layouts, row.variants)):
        if lay == E.LS:
            b = tb.SphereBVH(ctx).Build(E.sphere_set())
            bounds.append(b._bounds)
        else:
            d = E.DEEP_DEPTH[(kernel, lay)]
            b = E.deep_blas(ctx, lay, var, d)
            bounds.append(E.chain_bounds(d)); chains.append((k, d))
        blas.append(b)
    try:
        for use, d in chains:
            inst, wald, idx, rays, t, want_inst, tol = E.deep_scene(np.array(bounds, np.float32), use, d)
            tl = tb.TLAS(ctx).Upload(E.wald_to_al(wald), idx, inst, blas)
            try:
                if query == "occluded":
                    assert tl.IsOccluded(rays.copy()).all()
                    short = rays.copy(); short["t"] = (t - 4 * tol).astype(np.float32)      # ends just before the triangle: crosses the chains, meets nothing
                    assert not tl.IsOccluded(short).any()
                else:
                    got = tl.Intersect(rays.copy())
                    assert np.all(got["prim"] == CLUMP * (d + 1) - 1), (key, use, np.unique(got["prim"]))
                    assert np.array_equal(got["inst"], want_inst), (key, use)
                    assert np.all(np.abs(got["t"] - t) <= tol), (key, use, float(np.abs(got["t"] - t).max()))
            finally:
                tl.free()
    finally:
        for b in blas:
            b.free()
