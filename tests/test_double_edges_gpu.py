"""The fp64 two-level kernels against the hostile instances of double_edges_lib.py: every record of Intersect byte-identical (all 128 bytes) and every byte of
IsOccluded equal to the restated oracle under the library's rule (rule 1), which tests/test_double_edges_host.py pins to the real reference.

Two rows, picked by the rule of capi_double.hip (launchDouble): a TLAS_Double one of whose BLASes is a sphere BLAS (tlas.blasSpheres, set by
tbvh_upload_tlas_double) is traced by the sphere form of the one kernel, k_double<true, *, true>, which reads the tag bit of every BLAS descriptor; every
other by the triangle-only form k_double<false, *, true>, which reads plain pointers.

    T   BVH_Double + BVH_Double          k_double<false, *, true>   oracle_double.c
    M   SphereBVH_Double + BVH_Double    k_double<true, *, true>    oracle_custom_double.c

The library has no call that names the kernel of an fp64 TLAS.  What row M shows of it: a hit on a sphere instance comes back with the u, v the record went in
with, which only the sphere form does (test_fresh_rays asserts it).  Row T's scene goes through BOTH forms in
test_triangle_scene_answers_the_same_through_both_forms: listing a sphere BLAS that no instance references is enough to pick the sphere form.

Two trees per row: the host-built TLAS as uploaded, and the same TLAS after RebuildOnDevice(), whose expectation is the oracle on Download() and whose
instance records equal the host's Update bit for bit.

Projective and singular instances: ONE record per ray is expected (test_double_edges_host.py says why); there is no loose alternative.

Findings: none.  On the first run every comparison of this file held: no family, group, tree or batch size showed a record or an occlusion byte that
differs from the oracle's.
"""
import numpy as np
import pytest

import double_edges_lib as E
import tinybvh_amd as tb
from custom_double_lib import chain_spheres, chain_tree, ocd   # noqa: F401 (ocd: fixture)
from double_lib import odbl                                      # noqa: F401 (fixture)
from test_double_anim_gpu import same_instances
from test_double_edges_host import batches, check_ties_and_masks, hand_trees, oracle_of, reversed_root_leaf
from test_double_gpu import chain_scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = tb.Context(0)
    yield c
    c.close()


class Row:
    """a row's host scene and its BLASes on the device (the trees are the host scene's: the oracle walks what the kernel walks)"""

    def __init__(self, ctx, row):
        self.host = E.HostScene(row)
        self.blases = [(tb.SphereBVH_Double if kind == "sph" else tb.BVH_Double)(ctx).Upload(nodes, idx, prims) for kind, nodes, idx, prims in self.host.blas]


@pytest.fixture(scope="module")
def rows(ctx):
    """the rows made so far, by name: row T serves its own tests and the test of both forms"""
    return {}


def row_of(rows, ctx, name):
    if name not in rows:
        rows[name] = Row(ctx, name)
    return rows[name]


@pytest.fixture(scope="module", params=["T", "M"])
def row(request, ctx, rows):
    return row_of(rows, ctx, request.param)


class Live:
    """a TLAS on the device, the tree and the instance records it holds, and the oracle's fresh records over them"""

    def __init__(self, row, tl, tree, inst, oracle):
        self.row, self.sc, self.tl, self.tree, self.inst, self.oracle = row, row.host, tl, tree, inst, oracle
        self.fresh = self.want(self.sc.rays)

    def want(self, rays):
        return self.sc.intersect(self.oracle, rays, tree=self.tree, inst=self.inst, rule=1)

    def want_occ(self, rays):
        return self.sc.occluded(self.oracle, rays, tree=self.tree, inst=self.inst, rule=1)

    def check(self, rays, what):
        got = self.tl.Intersect(rays.copy())
        want = self.want(rays)
        E.same_records(got, want, f"{self.sc.row} {what} Intersect")
        return got

    def check_occ(self, rays, what):
        got, want = self.tl.IsOccluded(rays), self.want_occ(rays)
        E.same_bytes(got, want, f"{self.sc.row} {what} IsOccluded")
        return got


def make_live(kind, ctx, row, odbl, ocd, blases=None):
    """the row's TLAS over `blases` (the row's own list by default), as uploaded or after RebuildOnDevice()"""
    sc = row.host
    blases = row.blases if blases is None else blases
    if kind == "uploaded":
        tl = tb.TLAS_Double(ctx).Upload(sc.tn, sc.ti, sc.inst, blases)
        return Live(row, tl, (sc.tn, sc.ti), sc.inst, oracle_of(sc, odbl, ocd))
    tl = tb.TLAS_Double(ctx).Upload(sc.tn, sc.ti, sc.raw_inst, blases)   # the records go up WITHOUT inverse and bounds
    tl.RebuildOnDevice()
    tn, ti, inst = tl.Download()
    same_instances(inst, sc.inst, "device instance update")
    return Live(row, tl, (tn, ti), inst, oracle_of(sc, odbl, ocd))


@pytest.fixture(scope="module", params=["uploaded", "rebuilt"])
def live(request, ctx, row, odbl, ocd):
    return make_live(request.param, ctx, row, odbl, ocd)


# ---- 1 -----------------------------------------------------------------------------------------------------------------------------------
def test_fresh_rays(live):
    sc = live.sc
    got = live.check(sc.rays, "fresh")
    hit = E.changed(got, sc.rays)
    for g, s in sc.groups.items():
        assert g in ("mask0", "nonfinite") or hit[s].any(), g
    if sc.row == "M":
        on_sphere = hit & sc.on_sphere(got)
        assert on_sphere.sum() > 1000 and np.array_equal(got["u"][on_sphere], sc.rays["u"][on_sphere]) and np.array_equal(got["v"][on_sphere], sc.rays["v"][on_sphere])
        dec = E.carried(sc.rays, 1e300)   # u = 7, v = 9 going in: a sphere that wins leaves them, a triangle that wins replaces them
        got = live.check(dec, "decorated")
        on_sphere = E.changed(got, dec) & sc.on_sphere(got)
        assert (got["u"][on_sphere] == 7.0).all() and (got["v"][on_sphere] == 9.0).all() and (got["u"][E.changed(got, dec) & ~on_sphere] != 7.0).all()


@pytest.mark.parametrize("kind", ["uploaded", "rebuilt"])
def test_triangle_scene_answers_the_same_through_both_forms(kind, ctx, rows, odbl, ocd):
    """Row T's scene twice: as it is (the triangle-only form), and with a one-sphere SphereBVH_Double added to the BLAS list, which no instance references and
    no ray can reach (the sphere form: every descriptor carries the tag bit's place, and both triangle BLASes have it clear).  Each upload's records and
    occlusion bytes are oracle_double.c's over the tree it holds, and the two uploads answer alike."""
    row = row_of(rows, ctx, "T")
    sc = row.host
    one = np.array([[0.25, -0.5, 0.125, 0.75]])
    h = tb.host_build_custom_spheres_double(one)
    sphere = tb.SphereBVH_Double(ctx).Upload(h.nodes(), h.prim_idx(), one)
    plain = make_live(kind, ctx, row, odbl, ocd)
    tagged = make_live(kind, ctx, row, odbl, ocd, row.blases + [sphere])
    assert (sc.inst["blasIdx"] < len(row.blases)).all()
    a, b = plain.check(sc.rays, f"{kind}, triangle BLASes only"), tagged.check(sc.rays, f"{kind}, a sphere BLAS listed")
    E.same_records(a, b, f"{kind}: the two forms, Intersect")
    assert E.changed(a, sc.rays).sum() > 4000
    for name, rays in batches(sc, plain.fresh).items():
        a, b = plain.check_occ(rays, f"{kind}, triangle BLASes only, {name}"), tagged.check_occ(rays, f"{kind}, a sphere BLAS listed, {name}")
        E.same_bytes(a, b, f"{kind}: the two forms, IsOccluded, {name}")


# ---- 2 -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", ["carried 1e-9", "carried quarter", "carried equal", "carried next"])
def test_finite_tmax_and_carried_hits(live, batch):
    sc = live.sc
    rays = batches(sc, live.fresh)[batch]
    got = live.check(rays, batch)
    miss = ~E.changed(got, rays)        # (same_records has compared all 128 bytes of the misses with the oracle's, which leaves them alone)
    assert miss.mean() >= 0.3
    hit = E.changed(live.fresh, sc.rays)
    tri = ~sc.on_sphere(live.fresh)     # (a sphere is a candidate iff dist < tmax |D|, a product that may round either way AT the recorded distance)
    world_t = live.fresh["inst"] != sc.fam("projective")   # (a projective instance's t is no world distance: the TLAS's culls may not reach the hit)
    if batch == "carried equal":
        assert miss[tri].all() and hit.sum() > 4000            # `found` starts false: a hit AT the carried t is no hit
    if batch == "carried next":
        assert np.array_equal(~miss[tri & world_t], hit[tri & world_t])
        assert np.array_equal(got["t"][hit & tri & world_t].view(np.uint64), live.fresh["t"][hit & tri & world_t].view(np.uint64))


# ---- 3 -----------------------------------------------------------------------------------------------------------------------------------
def test_occluded(live):
    """the guard-window groups (axis_*: instance-space D components of exactly 0, -1e-25 and 1e-23) make this the guarded_rcp test: test_double_edges_host.py shows
    that an oracle with 1.0 / d in its place fails against the reference on this batch"""
    sc = live.sc
    g = E.guard_reached(live.inst, sc.rays)
    assert g.sum() >= 200
    for name, rays in batches(sc, live.fresh).items():
        occ = live.check_occ(rays, name)
        assert name != "fresh" or (20 <= occ[g].sum() <= g.sum() - 20), int(occ[g].sum())


# ---- 4, 5 --------------------------------------------------------------------------------------------------------------------------------
def test_ties_and_masks(live, ctx):
    sc = live.sc
    got = live.tl.Intersect(sc.rays.copy())
    check_ties_and_masks(sc, sc.rays, got)
    # the root leaf that lists the instances backwards meets dup1 before dup0: the equal t, the equal prim, then the smaller instance
    tn, ti = reversed_root_leaf(sc)
    back = Live(live.row, tb.TLAS_Double(ctx).Upload(tn, ti, sc.inst, live.row.blases), (tn, ti), sc.inst, live.oracle)
    got = back.check(sc.rays, "reversed root leaf")
    check_ties_and_masks(sc, sc.rays, got)
    r0 = sc.intersect(live.oracle, sc.rays, tree=(tn, ti), rule=0)
    assert ((r0["inst"] == sc.fam("dup1")) & (got["inst"] == sc.fam("dup0"))).sum() >= 50


# ---- 6 -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["root leaf", "chain", "leaves of three"])
def test_hand_made_tlas(row, ctx, odbl, ocd, shape):
    sc = row.host
    tn, ti = hand_trees(sc)[shape]
    lv = Live(row, tb.TLAS_Double(ctx).Upload(tn, ti, sc.inst, row.blases), (tn, ti), sc.inst, oracle_of(sc, odbl, ocd))
    got = lv.check(sc.rays, shape)
    check_ties_and_masks(sc, sc.rays, got)
    for name in ("fresh", "carried quarter"):
        lv.check_occ(batches(sc, lv.fresh)[name], f"{shape}, {name}")


def test_one_instance_of_one_primitive(row, ctx, odbl, ocd):
    """a leaf root over a leaf root"""
    sc = row.host
    if sc.row == "M":
        prim = np.array([[0.25, -0.5, 0.125, 0.75]])
        h = tb.host_build_custom_spheres_double(prim)
        blas = tb.SphereBVH_Double(ctx).Upload(h.nodes(), h.prim_idx(), prim)
        desc, bounds = ("sph", h.nodes(), h.prim_idx(), prim), E.sphere_bounds(prim)
    else:
        prim = np.array([[-1.0, -0.5, 0.25], [1.0, -0.75, 0.0], [0.125, 1.0, -0.25]])
        h = tb.host_build_double(prim)
        blas = tb.BVH_Double(ctx).Upload(h.nodes(), h.prim_idx(), prim)
        desc, bounds = ("tri", h.nodes(), h.prim_idx(), prim), E.tri_bounds(prim)
    assert len(h.nodes()) == 1 and h.nodes()[0]["triCount"] == 1
    T = np.eye(4); T[:3, :3] = E._euler(0.3, 0.5, 0.7) * 1.5; T[:3, 3] = [3.0, -2.0, 1.0]
    inst = tb.make_instances_ex(T[None], 0)
    th = E.fill_instances(inst, bounds)
    tn, ti = th.nodes().copy(), th.prim_idx().copy()
    assert len(tn) == 1 and tn[0]["triCount"] == 1
    tl = tb.TLAS_Double(ctx).Upload(tn, ti, inst, [blas])
    rng = np.random.default_rng(2)
    O = T[:3, 3] + rng.normal(size=(512, 3)) * 4.0
    rays = tb.make_rays_ex(O, T[:3, 3] + rng.uniform(-1, 1, (512, 3)) - O)
    rays = np.concatenate([rays, E.carried(rays, 3.0), E.nonfinite_rays(T[:3, 3])])
    o = oracle_of(sc, odbl, ocd)
    if sc.row == "M":
        want, want_occ = o.tlas_intersect(tn, ti, inst, [desc], rays, rule=1), o.tlas_occluded(tn, ti, inst, [desc], rays, rule=1)
    else:
        want, want_occ = o.intersect_tlas(tn, ti, inst, [desc[1:]], rays, rule=1), o.occluded_tlas(tn, ti, inst, [desc[1:]], rays, rule=1)
    E.same_records(tl.Intersect(rays.copy()), want, "one instance of one primitive")
    E.same_bytes(tl.IsOccluded(rays), want_occ, "one instance of one primitive")
    assert 100 < E.changed(want, rays).sum() < rays.shape[0] - 100 and 0 < want_occ.sum() < rays.shape[0]


# ---- 7 -----------------------------------------------------------------------------------------------------------------------------------
def test_spill_with_tlas_entries_beneath(row, ctx, odbl, ocd):
    """the geometry of test_tlas_stack_overflow_is_an_error_not_a_wild_access (41 instances in a chain over a BLAS chain 30 levels deep) in a DEFAULT context:
    rays travelling in -z enter the instances with one pending TLAS entry per level (blasBase up to 40) and push the BLAS's leaves on top, past the 16 entries of
    the LDS part and into the spill area.  No error, and the oracle's records."""
    sc = row.host
    if sc.row == "M":
        bn, bi, prims = chain_spheres(30)
        blas, desc, span = tb.SphereBVH_Double(ctx).Upload(bn, bi, prims), [("sph", bn, bi, prims)], (-0.5, 0.5)
    else:
        bn, bi, prims = chain_scene(30)
        blas, desc, span = tb.BVH_Double(ctx).Upload(bn, bi, prims), [(bn, bi, prims)], (-1.5, 0.5)
    n_inst = 41
    T = np.tile(np.eye(4), (n_inst, 1, 1))
    T[:, 2, 3] = 100.0 * np.arange(n_inst)
    inst = tb.make_instances_ex(T, 0)
    tb.host_build_tlas_double(inst, blas.bounds[None, :])
    tn, ti = chain_tree(inst["aabbMin"], inst["aabbMax"]), np.arange(n_inst, dtype=np.uint64)
    tl = tb.TLAS_Double(ctx).Upload(tn, ti, inst, [blas])
    rng = np.random.default_rng(8)
    n = 256
    xy = np.stack([rng.uniform(*span, n), rng.uniform(*span, n)], 1)
    o = oracle_of(sc, odbl, ocd)
    for z0, dz in ((100.0 * n_inst + 50.0, -1.0), (-50.0, 1.0)):
        rays = tb.make_rays_ex(np.concatenate([xy, np.full((n, 1), z0)], 1), np.tile([1e-5, 2e-5, dz], (n, 1)))
        if sc.row == "M":
            want, want_occ = o.tlas_intersect(tn, ti, inst, desc, rays, rule=1), o.tlas_occluded(tn, ti, inst, desc, rays, rule=1)
        else:
            want, want_occ = o.intersect_tlas(tn, ti, inst, desc, rays, rule=1), o.occluded_tlas(tn, ti, inst, desc, rays, rule=1)
        assert (want["inst"] == (n_inst - 1 if dz < 0 else 0)).all() and want_occ.all()
        E.same_records(tl.Intersect(rays.copy()), want, f"dz {dz} Intersect")
        E.same_bytes(tl.IsOccluded(rays), want_occ, f"dz {dz}")


# ---- 8 -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000])
def test_ragged_batches(live, ctx, n):
    """the nonfinite records spread among ordinary rays, so that they share waves with them; n = 1000 also through the device-resident entry points"""
    sc = live.sc
    bad = sc.rays[sc.groups["nonfinite"]]
    rng = np.random.default_rng(n)
    rays = sc.rays[rng.choice(sc.groups["nonfinite"].start, max(n, 1), replace=False)][:n].copy()
    if n:
        at = np.arange(0, n, 7)[: bad.shape[0]]
        rays[at] = bad[: at.size]
    got, occ = live.tl.Intersect(rays.copy()), live.tl.IsOccluded(rays)
    assert got.shape[0] == n and occ.shape[0] == n
    if n == 0:
        return
    want, want_occ = live.want(rays), live.want_occ(rays)
    E.same_records(got, want, f"batch of {n}")
    E.same_bytes(occ, want_occ, f"batch of {n}")
    if n == 1000:
        d = ctx.malloc(rays.nbytes); docc = ctx.malloc(n)
        try:
            ctx.to_device(d, rays)
            live.tl.occluded_device(d, n, docc)
            live.tl.intersect_device(d, n)
            out = np.zeros_like(rays); o2 = np.zeros(n, np.uint8)
            ctx.from_device(out, d); ctx.from_device(o2, docc)
        finally:
            ctx.free(d); ctx.free(docc)
        E.same_records(out, want, "device-resident Intersect")
        E.same_bytes(o2, want_occ, "device-resident IsOccluded")
