"""BVH_Double scenes that move, on the GPU: the device TLAS rebuild (tbvh_rebuild_tlas_double_device), the in-place update and the downloads,
and the BLAS refit (tbvh_refit_double), against the restated oracle (tests/oracle_double.c, rule 1) walking the trees the device made:
every record byte-identical, every occlusion bit equal, every box exact."""
import ctypes as C

import numpy as np
import pytest

import tinybvh_amd as tb
from tinybvh_amd import lib, rays as R, scenes
from double_lib import bounce_rays_dbl, camera_rays_dbl, instance_scene, odbl, random_rays_dbl, rot_matrix, rotated_soup, to_dbl  # noqa: F401 (odbl: fixture)
from test_double_gpu import chain_scene, same_records
from double_anim_lib import CENTRE, TREE_SHAPE_CAP, bounds_of, check_tlas_tree, karras_tlas, refit_boxes, tlas_rays, tlas_scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = tb.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def blas_verts():
    return tlas_scene()[0]


@pytest.fixture(scope="module")
def blases(ctx, blas_verts):
    """The BLASes of instance_scene, shared and never refitted (the tests that refit build their own)."""
    return [tb.BVH_Double(ctx).Build(v) for v in blas_verts]


@pytest.fixture(scope="module")
def rays():
    r = tlas_rays()
    r.flags.writeable = False
    return r


@pytest.fixture(scope="module")
def scene500(ctx, blases):
    """instance_scene(500): the host-built TLAS as uploaded, then rebuilt on the device; (tlas, instances after the host's Update, host nodes, host idx)."""
    _, inst = tlas_scene()
    tl = tb.TLAS_Double(ctx).Build(inst, blases)
    hn, hi = tl.host.nodes().copy(), tl.host.prim_idx().copy()
    tl.RebuildOnDevice()
    return tl, inst, hn, hi


def blobs(blases):
    return [(b.host.nodes(), b.host.prim_idx(), b.verts) for b in blases]


def as_u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same_instances(got, want, what):
    for f in ("transform", "invTransform", "aabbMin", "aabbMax", "blasIdx", "mask"):
        assert np.array_equal(as_u64(got[f]), as_u64(want[f])), f"{what}: {f} differs in instances {np.nonzero((as_u64(got[f]) != as_u64(want[f])).reshape(got.shape[0], -1).any(1))[0][:8].tolist()}"


def check_queries(tl, blases, odbl, rays, what, occ_t=40.0):
    """Intersect and IsOccluded of tl against the oracle walking the tree downloaded from it; returns the traced records and the download."""
    tn, ti, inst = tl.Download()
    want = odbl.intersect_tlas(tn, ti, inst, blobs(blases), rays, rule=1)
    got = tl.Intersect(rays.copy())
    same_records(got, want, what + " Intersect")
    sh = rays.copy(); sh["t"] = occ_t
    occ = tl.IsOccluded(sh)
    occ_want = odbl.occluded_tlas(tn, ti, inst, blobs(blases), sh, rule=1)
    assert np.array_equal(occ, occ_want), f"{what} IsOccluded: {int((occ != occ_want).sum())} differ"
    return got, occ, (tn, ti, inst)


def moved(T: np.ndarray) -> np.ndarray:
    """The next frame: everything translated, every 7th instance scaled, every 5th rotated."""
    T = T.reshape(-1, 4, 4).copy()
    T[:, :3, 3] += np.array([0.37, 0.0, -0.21])
    T[::7, :3, :3] *= 1.3
    T[::5, :3, :3] = rot_matrix(0.2, -0.4, 0.9) @ T[::5, :3, :3]
    return np.ascontiguousarray(T)


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------------

def test_instance_records(ctx, blases, blas_verts):
    _, inst = tlas_scene()
    T = inst["transform"].reshape(-1, 4, 4).copy()
    T[10, 3] = [0.0, 0.0, 1e-3, 1.5]                 # a perspective row: w != 1
    T[20, 2, :3] = 0.0                               # a singular matrix: everything flattened into a plane, det == 0 exactly
    T[30] = np.eye(4); T[30, :3, 3] = 1e7            # a pure translation by 1e7
    inst["transform"] = T.reshape(-1, 16)
    raw = inst.copy()
    host = tb.host_build_tlas_double(inst, bounds_of(blas_verts))   # (fills inst in place: what the device must reproduce)
    assert np.isfinite(inst["invTransform"][20]).all() and not np.array_equal(inst["invTransform"][20], np.eye(4).reshape(16))   # unscaled cofactors, not a division by 0
    tl = tb.TLAS_Double(ctx).Upload(host.nodes(), host.prim_idx(), raw, blases)   # the records go up WITHOUT inverse and bounds
    tl.RebuildOnDevice()
    nodes, idx, got = tl.Download()
    same_instances(got, inst, "device instance update")
    check_tlas_tree(nodes, idx, got)


# ---- 2, 3 -------------------------------------------------------------------------------------------------------------------------------

def rebuilt(ctx, blases, inst):
    tl = tb.TLAS_Double(ctx).Build(inst, blases)
    before = tl.device_bytes
    tl.RebuildOnDevice()
    assert tl.device_bytes >= before
    return tl


@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 1000])
def test_tree_validity(ctx, blases, n):
    _, inst = instance_scene(n)
    tl = rebuilt(ctx, blases, inst)
    nodes, idx, got = tl.Download()
    same_instances(got, inst, f"n = {n}")
    check_tlas_tree(nodes, idx, got)
    kn, ki = karras_tlas(got)   # the same keys, a stable sort and the same numbering: the same blob
    assert np.array_equal(idx, ki) and nodes.tobytes() == kn.tobytes()
    bytes_once = tl.device_bytes
    tl.RebuildOnDevice()        # a later rebuild allocates nothing and gives the same tree
    n2, i2, _ = tl.Download()
    assert tl.device_bytes == bytes_once and n2.tobytes() == nodes.tobytes() and np.array_equal(i2, idx)
    second = tb.TLAS_Double(ctx).Upload(nodes, idx, got, blases)   # validateDouble is the judge
    assert second.device_bytes > 0


def test_equal_keys(ctx, blases, odbl):
    _, inst = instance_scene(27)
    inst[1::2] = inst[0:26:2]   # the odd instances are exact copies of the even ones: equal boxes, equal keys
    tl = rebuilt(ctx, blases, inst)
    nodes, idx, got = tl.Download()
    check_tlas_tree(nodes, idx, got)
    r = tlas_rays(8192, seed=5)
    traced, _, _ = check_queries(tl, blases, odbl, r, "equal keys")
    hit = traced["t"] < 1e299
    assert hit.sum() > 50 and (traced["inst"][hit] % 2 == 0).all()   # of two copies the smaller instance (an even one) wins


# ---- 4, 5 -------------------------------------------------------------------------------------------------------------------------------

def test_queries_on_the_device_tree(scene500, blases, odbl, rays):
    tl, inst, _, _ = scene500
    got, occ, _ = check_queries(tl, blases, odbl, rays, "device tree")
    assert 0 < occ.sum() < occ.size
    hit = got["t"] < 1e299
    assert hit.sum() > 1000 and np.unique(got["inst"][hit]).size > 100


def test_queries_do_not_depend_on_the_tree(scene500, blases, odbl, rays):
    """The device-built tree's answers against the oracle on the HOST-built tree: identical up to TREE_SHAPE_CAP records (1e-4 of the batch;
    test_double_anim_host.py checks the two host-side walks against that cap for this scene and batch)."""
    tl, inst, hn, hi = scene500
    want = odbl.intersect_tlas(hn, hi, inst, blobs(blases), rays, rule=1)
    got = tl.Intersect(rays.copy())
    a = got.view(np.uint8).reshape(-1, 128); b = want.view(np.uint8).reshape(-1, 128)
    differ = int((a != b).any(1).sum())
    assert differ <= TREE_SHAPE_CAP, f"{differ} of {rays.shape[0]} records differ between the device-built and the host-built tree"


# ---- 6 ----------------------------------------------------------------------------------------------------------------------------------

def test_frames(ctx, blases, blas_verts, odbl, rays):
    _, inst = tlas_scene()
    tl = tb.TLAS_Double(ctx).Build(inst, blases)
    tl.RebuildOnDevice()
    frame0 = tl.Intersect(rays.copy())
    T1 = moved(inst["transform"])
    fresh = inst.copy(); fresh["transform"] = T1.reshape(-1, 16)
    tb.host_build_tlas_double(fresh, bounds_of(blas_verts))
    tl.RebuildOnDevice(T1)
    assert ctx.time_last_ms() > 0
    frame1, _, (_, _, got1) = check_queries(tl, blases, odbl, rays, "frame 1 (host transforms)")
    same_instances(got1, fresh, "frame 1")
    assert (frame1["t"] != frame0["t"]).any()
    d = ctx.malloc(T1.nbytes)
    try:
        ctx.to_device(d, T1)
        tl.RebuildOnDevice(inst["transform"].reshape(-1, 4, 4))   # back to frame 0 in between, so frame 2 has something to do
        tl.RebuildOnDevice(d, on_device=True)
        frame2, _, (_, _, got2) = check_queries(tl, blases, odbl, rays, "frame 2 (device transforms)")
    finally:
        ctx.free(d)
    same_instances(got2, fresh, "frame 2")
    same_records(frame2, frame1, "frame 2 against frame 1")


# ---- 7 ----------------------------------------------------------------------------------------------------------------------------------

def test_grown_tlas(ctx, blases, blas_verts, odbl):
    _, small = instance_scene(27)
    tl = rebuilt(ctx, blases, small)
    r = tlas_rays(8192, seed=9)
    check_queries(tl, blases, odbl, r, "27 instances")
    _, big = instance_scene(216, seed=4)
    host = tb.host_build_tlas_double(big, bounds_of(blas_verts))
    tl.Update(host.nodes(), host.prim_idx(), big)
    want = odbl.intersect_tlas(host.nodes(), host.prim_idx(), big, blobs(blases), r, rule=1)
    same_records(tl.Intersect(r.copy()), want, "216 instances, host blobs")
    assert (want["t"] < 1e299).sum() > 100
    dn, di, dinst = tl.Download()
    assert dn.tobytes() == host.nodes().tobytes() and np.array_equal(di, host.prim_idx()) and dinst.tobytes() == big.tobytes()
    tl.RebuildOnDevice(moved(big["transform"]))
    got, _, (tn, ti, tinst) = check_queries(tl, blases, odbl, r, "216 instances, device rebuild")
    check_tlas_tree(tn, ti, tinst)
    assert (got["t"] != want["t"]).any()


# ---- 8 ----------------------------------------------------------------------------------------------------------------------------------

def refit_cases():
    soup = rotated_soup(300) + 1e7
    h = tb.host_build_double(soup)
    yield "soup at 1e7", h.nodes().copy(), h.prim_idx().copy(), soup
    for n in (1, 2):
        v = rotated_soup(n, seed=3)
        h = tb.host_build_double(v)
        yield f"{n} triangle(s)", h.nodes().copy(), h.prim_idx().copy(), v
    yield ("chain of 220",) + chain_scene(220)


@pytest.mark.parametrize("case", range(4))
def test_refit_boxes(ctx, case):
    what, nodes, idx, verts = list(refit_cases())[case]
    assert (what != "1 triangle(s)" or (len(nodes) == 1 and nodes[0]["triCount"] == 1)) and (what != "chain of 220" or len(nodes) == 441)
    sc = tb.BVH_Double(ctx).Upload(nodes, idx, verts)
    rng = np.random.default_rng(case)
    new = verts * 1.25 + rng.normal(0, 0.3, verts.shape) + np.array([0.5, -0.25, 2.0])
    before = sc.device_bytes
    sc.Refit(new)
    got = sc.Download()
    assert sc.device_bytes > before   # the parent array and the leaf list are the scene's now
    assert np.array_equal(got["leftFirst"], nodes["leftFirst"]) and np.array_equal(got["triCount"], nodes["triCount"]), what
    want = refit_boxes(nodes, idx, new)
    assert np.array_equal(got["aabbMin"], want["aabbMin"]) and np.array_equal(got["aabbMax"], want["aabbMax"]), what
    assert np.array_equal(sc.bounds, np.concatenate([new.min(0), new.max(0)]))
    grown = sc.device_bytes
    sc.Refit(verts)
    assert sc.device_bytes == grown and sc.Download().tobytes() == refit_boxes(nodes, idx, verts).tobytes(), what


# ---- 9 ----------------------------------------------------------------------------------------------------------------------------------

def test_refit_queries(ctx, odbl):
    off = np.array([1e7, 0.0, -1e7])
    verts = to_dbl(scenes.atrium(6000)) + off
    sc = tb.BVH_Double(ctx).Build(verts)
    idx = sc.host.prim_idx().copy()
    eye, view = scenes.SPONZA_CAMERAS[0]
    cam = camera_rays_dbl(eye, view, 65, 63, offset=off)
    assert cam.shape[0] == 65 * 63
    local = verts - off
    new = verts + 0.28 * np.stack([np.sin(0.31 * local[:, 1]), np.sin(0.23 * local[:, 2] + 1.0), np.cos(0.17 * local[:, 0])], 1)   # smooth, at most 0.5 units long
    new[::3] += 1e-3

    def trace(v, what):
        nodes = sc.Download()
        out = []
        first = odbl.intersect(nodes, idx, v, cam, rule=1)
        for name, r, occ_t in (("camera", cam, 30.0), ("bounce", bounce_rays_dbl(first), 8.0)):
            want = odbl.intersect(nodes, idx, v, r, rule=1)
            got = sc.Intersect(r.copy())
            same_records(got, want, f"{what} {name} Intersect")
            sh = r.copy(); sh["t"] = occ_t
            assert np.array_equal(sc.IsOccluded(sh), odbl.occluded(nodes, idx, v, sh, rule=1)), f"{what} {name} IsOccluded"
            assert (want["t"] < 1e299).sum() > r.shape[0] // 20   # (the oracle alone: 820 camera and 379 bounce rays of 4095 hit)
            out.append(got)
        return out

    before = trace(verts, "as uploaded")
    sc.Refit(new)
    after = trace(new, "refitted")
    assert after[0].tobytes() != before[0].tobytes()
    sc.Refit(verts)
    assert sc.Download().tobytes() == sc.host.nodes().tobytes()
    again = trace(verts, "refitted back")
    for a, b in zip(again, before):
        same_records(a, b, "back to the original vertices")


# ---- 10, 11 -----------------------------------------------------------------------------------------------------------------------------

def test_refit_under_a_tlas(ctx, blas_verts, odbl, rays):
    own = [tb.BVH_Double(ctx).Build(v) for v in blas_verts]
    _, inst = tlas_scene()
    tl = tb.TLAS_Double(ctx).Build(inst, own)
    tl.RebuildOnDevice()
    new0 = blas_verts[0] * 1.5
    own[0].Refit(new0)
    tl.RebuildOnDevice()   # reads the refitted root box
    want_inst = inst.copy()
    tb.host_build_tlas_double(want_inst, bounds_of([new0, blas_verts[1], blas_verts[2]]))
    assert not np.array_equal(want_inst["aabbMax"], inst["aabbMax"])
    tn, ti, got_inst = tl.Download()
    same_instances(got_inst, want_inst, "after the BLAS refit")
    bl = [(own[0].Download(), own[0].host.prim_idx(), new0)] + blobs(own[1:])
    want = odbl.intersect_tlas(tn, ti, got_inst, bl, rays, rule=1)
    same_records(tl.Intersect(rays.copy()), want, "TLAS over a refitted BLAS")
    assert (want["t"] < 1e299).sum() > 1000


def test_device_resident_vertices(ctx):
    verts = rotated_soup(300) + 1e7
    new = verts * 0.75 + 3.0
    a = tb.BVH_Double(ctx).Build(verts); b = tb.BVH_Double(ctx).Build(verts)
    a.Refit(new)
    d = ctx.malloc(new.nbytes)
    try:
        ctx.to_device(d, new)
        b.Refit(d, on_device=True)
        got = b.Download()
    finally:
        ctx.free(d)
    assert got.tobytes() == a.Download().tobytes() and got.tobytes() != a.host.nodes().tobytes()
    assert np.array_equal(b.bounds, a.bounds)
    r = random_rays_dbl(2048, new.min(0) - 2, new.max(0) + 2, seed=2)
    same_records(b.Intersect(r.copy()), a.Intersect(r.copy()), "device-resident against host-staged vertices")


# ---- 12 ---------------------------------------------------------------------------------------------------------------------------------

def test_refusals(ctx, blases, blas_verts):
    verts = rotated_soup(300, seed=2)
    sc = tb.BVH_Double(ctx).Build(verts)
    _, inst = instance_scene(27)
    tl = tb.TLAS_Double(ctx).Build(inst, blases)
    tl.RebuildOnDevice()
    g = tb.BVH_GPU(ctx).Build(scenes.soup(100))
    t32 = tb.TLAS(ctx).Build(tb.make_instances(np.eye(4, dtype=np.float32)[None], 0), [g])
    r_b = random_rays_dbl(512, (-12, -12, -12), (12, 12, 12)); r_t = tlas_rays(2048, seed=6)
    sc_before = sc.Intersect(r_b.copy()); tl_before = tl.Intersect(r_t.copy())
    r32 = R.random_rays(256, (0, 0, 0), (1, 1, 1))
    g_before = g.Intersect(r32.copy()); t32_before = t32.Intersect(r32.copy())
    assert (sc_before["t"] < 1e299).any() and (tl_before["t"] < 1e299).any()
    nb = C.c_uint64(0)
    buf = np.zeros(1 << 16, np.uint8)
    hn, hi, hinst = tl.Download()
    p = lambda a: a.ctypes.data
    n_tris = verts.shape[0] // 3
    tlas_calls = {
        "tbvh_rebuild_tlas_double_device": lambda h: lib.tbvh_rebuild_tlas_double_device(h, None, 0),
        "tbvh_update_tlas_double": lambda h: lib.tbvh_update_tlas_double(h, p(hn), len(hn), p(hi), hi.size, p(hinst), hinst.shape[0]),
        "tbvh_tlas_double_download": lambda h: lib.tbvh_tlas_double_download(h, None, 0, None, 0, None, 0, C.byref(nb)),
    }
    blas_calls = {
        "tbvh_refit_double": lambda h: lib.tbvh_refit_double(h, p(verts), n_tris, 0),
        "tbvh_double_download": lambda h: lib.tbvh_double_download(h, None, 0, C.byref(nb)),
    }

    def refused(name, rc):
        err = lib.tbvh_last_error().decode()
        assert rc == -1 and name in err, (name, rc, err)

    for name, call in tlas_calls.items():
        for h in (sc._h, g._h, t32._h):   # a double BLAS, an fp32 BLAS, an fp32 TLAS
            refused(name, call(h))
    for name, call in blas_calls.items():
        for h in (tl._h, g._h, t32._h):
            refused(name, call(h))
    for n in (n_tris - 1, n_tris + 1):
        refused("tbvh_refit_double", lib.tbvh_refit_double(sc._h, p(verts), n, 0))
    bad = hinst.copy(); bad["blasIdx"][3] = len(blases)
    refused("tbvh_update_tlas_double", lib.tbvh_update_tlas_double(tl._h, p(hn), len(hn), p(hi), hi.size, p(bad), bad.shape[0]))
    assert "instance 3: blasIdx 3" in lib.tbvh_last_error().decode()
    bi = hi.copy(); bi[0] = hinst.shape[0]
    refused("tbvh_update_tlas_double", lib.tbvh_update_tlas_double(tl._h, p(hn), len(hn), p(bi), bi.size, p(hinst), hinst.shape[0]))
    assert "primIdx[0]" in lib.tbvh_last_error().decode()
    bn = hn.copy(); bn[0]["leftFirst"] = len(hn) - 1
    refused("tbvh_update_tlas_double", lib.tbvh_update_tlas_double(tl._h, p(bn), len(bn), p(hi), hi.size, p(hinst), hinst.shape[0]))
    assert "node 0: child index" in lib.tbvh_last_error().decode()
    # every scene still returns its previous records
    same_records(sc.Intersect(r_b.copy()), sc_before, "BLAS after the refusals")
    same_records(tl.Intersect(r_t.copy()), tl_before, "TLAS after the refusals")
    assert sc.Download().tobytes() == sc.host.nodes().tobytes()
    assert g.Intersect(r32.copy()).tobytes() == g_before.tobytes() and t32.Intersect(r32.copy()).tobytes() == t32_before.tobytes()


# ---- 13 ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 63, 65])
def test_batch_edges(scene500, blases, odbl, n):
    tl, _, _, _ = scene500
    r = random_rays_dbl(n, CENTRE - 80, CENTRE + 80, seed=n + 1)
    got = tl.Intersect(r.copy())
    occ = tl.IsOccluded(r)
    assert got.shape[0] == n and occ.shape[0] == n
    if n == 0:
        return
    tn, ti, inst = tl.Download()
    same_records(got, odbl.intersect_tlas(tn, ti, inst, blobs(blases), r, rule=1), f"batch {n}")
    assert np.array_equal(occ, odbl.occluded_tlas(tn, ti, inst, blobs(blases), r, rule=1))
