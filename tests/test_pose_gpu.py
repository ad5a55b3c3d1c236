"""Mesh::SetPose on the device (tbvh_pose_*; DESIGN.md par. 14): the posed vertices equal the real reference's (the goldens under tests/golden/pose) byte
for byte, w included, at the sizes where a one-vertex-per-lane kernel can go wrong (1, one short of a wave, a wave, one more, several blocks with a
ragged end, the whole golden); posing and refitting on the device leaves a scene that answers exactly as the same scene refitted from host-posed
vertices, alone and under a TLAS; a bad device-resident joint index is reported and never used."""
import numpy as np
import pytest

import tinybvh_amd as tb
from tinybvh_amd import rays as R
from oracle_lib import compare_hits
import pose_lib as P
from pose_lib import pose_oracle  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, P.SMALL, None]   # None: the whole golden (13056 vertices: 51 blocks)


def same_bytes(a, b):
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope="module")
def g_skin():
    return P.golden("skin_bunny16")


@pytest.fixture(scope="module")
def g_morph():
    return P.golden("morph_bunny16")


class _Param:
    """joint matrices / morph weights where the case wants them: the host array itself, or a device copy"""

    def __init__(self, ctx, on_device):
        self.ctx, self.on_device, self.ptrs = ctx, on_device, []

    def __call__(self, a):
        if not self.on_device:
            return a
        a = np.ascontiguousarray(a, np.float32)
        d = self.ctx.malloc(max(a.nbytes, 16)); self.ctx.to_device(d, a)
        self.ptrs.append(d)
        return d

    def free(self):
        self.ctx.synchronize()
        for d in self.ptrs:
            self.ctx.free(d)


@pytest.mark.parametrize("on_device", [False, True], ids=["host_mats", "device_mats"])
@pytest.mark.parametrize("n_joints", [1, P.N_JOINTS])
@pytest.mark.parametrize("n", SIZES)
def test_skin_equals_the_golden(ctx, g_skin, pose_oracle, n, n_joints, on_device):
    g = g_skin
    rest = P.rest4(g)
    n = n or rest.shape[0]
    joints = g["joints"][:n] if n_joints > 1 else np.zeros((n, 4), np.uint32)
    pose = tb.Pose(ctx).Skin(rest[:n], joints, g["weights"][:n], n_joints)
    param = _Param(ctx, on_device)
    try:
        if n_joints > 1:
            # frame 1 first (the non-uniform scale), then frame 0: nothing of the first call may be left in the second one's output
            got = pose.SetPose(param(g["mats"][1]), on_device=on_device).Download()
            m = min(n, P.SMALL)
            assert same_bytes(got[:m], g["out_b"][:m])
            assert same_bytes(got, pose_oracle.skin(rest[:n], joints, g["weights"][:n], g["mats"][1]))
            got = pose.SetPose(param(g["mats"][0]), on_device=on_device).Download()
            assert same_bytes(got, g["out"][:n])
        else:
            other = g["mats"][1][5:6]
            got = pose.SetPose(param(other), on_device=on_device).Download()
            assert same_bytes(got, pose_oracle.skin(rest[:n], joints, g["weights"][:n], other))
            got = pose.SetPose(param(g["mats1"]), on_device=on_device).Download()
            assert same_bytes(got, g["out1"][:n])
        assert not got[:, 3].view(np.uint32).any()
        d, count = pose.Vertices()
        assert d and count == n
    finally:
        pose.free()
        param.free()


@pytest.mark.parametrize("on_device", [False, True], ids=["host_weights", "device_weights"])
@pytest.mark.parametrize("n", SIZES)
def test_morph_equals_the_golden(ctx, g_morph, pose_oracle, n, on_device):
    g = g_morph
    n = n or g["positions"].shape[1]
    pos = np.ascontiguousarray(g["positions"][:, :n])
    pose = tb.Pose(ctx).Morph(pos)
    param = _Param(ctx, on_device)
    try:
        got = pose.SetPose(param(g["weights"][1]), on_device=on_device).Download()
        m = min(n, P.SMALL)
        assert same_bytes(got[:m], g["out_b"][:m])
        assert same_bytes(got, pose_oracle.morph(pos, g["weights"][1]))
        got = pose.SetPose(param(g["weights"][0]), on_device=on_device).Download()
        assert same_bytes(got, g["out"][:n])
        assert (got[:, 3].view(np.uint32) == np.float32(1).view(np.uint32)).all()
    finally:
        pose.free()
        param.free()


def test_morph_without_targets_copies_the_base(ctx, g_morph):
    base = np.ascontiguousarray(g_morph["positions"][:1, :65])
    pose = tb.Pose(ctx).Morph(base)
    got = pose.SetPose(np.zeros(0, np.float32)).Download()
    assert same_bytes(got[:, :3], base[0]) and (got[:, 3] == 1).all()
    pose.free()


def test_set_pose_refuses_wrong_counts_and_kinds(ctx, g_skin, g_morph):
    rest = P.rest4(g_skin)[:64]
    skin = tb.Pose(ctx).Skin(rest, g_skin["joints"][:64], g_skin["weights"][:64], P.N_JOINTS)
    morph = tb.Pose(ctx).Morph(np.ascontiguousarray(g_morph["positions"][:, :64]))
    for call in (lambda: skin.SetPose(g_skin["mats"][0][:23]),                                                    # 23 matrices for 24 joints
                 lambda: morph.SetPose(np.zeros(2, np.float32)),                                                  # 2 weights for 3 targets
                 lambda: tb.check(tb.lib.tbvh_pose_set_morph(skin._h, None, 0, 0), "set_morph on a skin pose"),
                 lambda: tb.check(tb.lib.tbvh_pose_set_skin(morph._h, g_skin["mats"].ctypes.data, 24, 0), "set_skin on a morph pose"),
                 lambda: tb.check(tb.lib.tbvh_pose_set_skin(skin._h, None, 24, 0), "null matrices")):
        with pytest.raises(tb.TbvhError) as e:
            call()
        assert e.value.code == -1
    bad = g_skin["joints"][:64].copy(); bad[17, 3] = P.N_JOINTS
    with pytest.raises(tb.TbvhError) as e:
        tb.Pose(ctx).Skin(rest, bad, g_skin["weights"][:64], P.N_JOINTS)
    assert e.value.code == -5 and "vertex 17" in str(e.value)
    skin.free(); morph.free()


# ---- pose + refit against the host-staged flow -----------------------------------------------------------------------------------------------
def camera_rays(verts):
    """one 128 x 64 camera batch from in front of the mesh"""
    lo, hi = verts[:, :3].min(0), verts[:, :3].max(0)
    c, ext = (lo + hi) / 2, float(np.linalg.norm(hi - lo))
    eye = c + np.array([0.25, 0.15, 0.85], np.float32) * ext
    view = (c - eye) / np.linalg.norm(c - eye)
    return R.primary(R.camera(eye, view, 128, 64, 1, 1)), eye, c


def oracle_hits(oracle, flat, rays, shadow_from=None):
    """BVH::Intersect restated over the posed triangles; with shadow_from also the shadow rays of those hits towards that light and their IsOccluded"""
    h = tb.HostBVH(flat, tb.LAYOUT_BVH_GPU)
    want = oracle.bvh2_intersect(h.bvh2_nodes(), h.bvh2_prim_idx(), flat, rays)
    if shadow_from is None:
        return want
    sh = R.shadow(want, shadow_from, 1e-4)
    return want, sh, oracle.bvh2_occluded(h.bvh2_nodes(), h.bvh2_prim_idx(), flat, sh)


def check(got, want, bits=True):
    """as tests/test_refit_device.py judges a refit"""
    c = compare_hits(got, want)
    assert c["hitmiss"] == 0 and c["prim_real"] == 0 and c["t_bad"] == 0 and c["uv_bad"] == 0, c
    assert c["tie"] <= 4 and c["onsurf"] <= 4, c
    if bits:
        assert c["bit_identical"] == c["same_prim"], c
    assert c["hits"] > 400, c   # (every 16th triangle of the bunny: the batch finds 530 ... 980 of them, counted on the CPU oracle)
    return c


def build(ctx, layout, rest, idx):
    cls = tb.LAYOUT_CLASSES[layout]
    return cls(ctx).Build(rest) if idx is None else cls(ctx).Build(rest, indices=idx)


def host_refit(sc, verts, idx):
    return sc.Refit(verts) if idx is None else sc.Refit(verts, mesh=True)


def skin_case(indexed):
    g = P.golden("skin_indexed" if indexed else "skin_bunny16")
    rest = P.rest4(g)
    idx = g["indices"] if indexed else None
    return g, rest, idx


@pytest.mark.parametrize("indexed", [False, True], ids=["flat", "indexed"])
@pytest.mark.parametrize("layout", [tb.LAYOUT_CWBVH, tb.LAYOUT_BVH_GPU, tb.LAYOUT_BVH4_GPU])
def test_pose_refit_equals_the_host_staged_refit(ctx, oracle, pose_oracle, layout, indexed):
    g, rest, idx = skin_case(indexed)
    a, b = build(ctx, layout, rest, idx), build(ctx, layout, rest, idx)
    pose = tb.Pose(ctx).Skin(rest, g["joints"], g["weights"], P.N_JOINTS)
    rays, _, _ = camera_rays(rest)
    for frame in (1, 0, 1):
        mats = g["mats"][frame]
        posed = pose_oracle.skin(rest, g["joints"], g["weights"], mats)     # what a caller without this feature computes on the host
        pose.SetPose(mats).Refit(a)
        host_refit(b, posed, idx)
        ra, rb = a.Intersect(rays.copy()), b.Intersect(rays.copy())
        assert ra.tobytes() == rb.tobytes()
        flat = posed if idx is None else P.flatten(posed, idx)
        want, sh, occ_want = oracle_hits(oracle, flat, rays, shadow_from=tuple(rest[:, :3].max(0) * 2))
        check(ra, want)
        oa, ob = a.IsOccluded(sh), b.IsOccluded(sh)
        assert np.array_equal(oa, ob)
        assert int((oa != occ_want).sum()) <= 2 and int(occ_want.sum()) > 20
    pose.free(); a.free(); b.free()


def test_morph_pose_refit_equals_the_host_staged_refit(ctx, oracle, pose_oracle, g_morph):
    pos, w = g_morph["positions"], g_morph["weights"]
    rest = np.zeros((pos.shape[1], 4), np.float32); rest[:, :3] = pos[0]
    a, b = build(ctx, tb.LAYOUT_CWBVH, rest, None), build(ctx, tb.LAYOUT_CWBVH, rest, None)
    pose = tb.Pose(ctx).Morph(pos)
    rays, _, _ = camera_rays(rest)
    for k in (1, 0):
        posed = pose_oracle.morph(pos, w[k])
        pose.SetPose(w[k]).Refit(a)
        b.Refit(posed)
        ra, rb = a.Intersect(rays.copy()), b.Intersect(rays.copy())
        assert ra.tobytes() == rb.tobytes()
        check(ra, oracle_hits(oracle, posed, rays))
    pose.free(); a.free(); b.free()


@pytest.mark.parametrize("indexed", [False, True], ids=["flat", "indexed"])
@pytest.mark.parametrize("layout", [tb.LAYOUT_CWBVH, tb.LAYOUT_BVH_GPU, tb.LAYOUT_BVH4_GPU])
def test_pose_refit_under_a_tlas_that_is_not_uploaded_again(ctx, oracle, pose_oracle, layout, indexed):
    """Two instances of the animated BLAS — one where it is, one behind the camera —, the TLAS uploaded ONCE over boxes that hold every frame: per frame
    only SetPose + Pose.Refit run, and the TLAS traces the new geometry."""
    g, rest, idx = skin_case(indexed)
    frames = [pose_oracle.skin(rest, g["joints"], g["weights"], g["mats"][f]) for f in (0, 1)]
    every = np.concatenate([rest] + frames)[:, :3]
    box = np.concatenate([every.min(0), every.max(0)]).astype(np.float32)
    rays, eye, c = camera_rays(rest)
    xf = np.stack([np.eye(4, dtype=np.float32)] * 2)
    xf[1, :3, 3] = (eye - c) * 3          # behind the camera: no camera ray reaches it
    tl = []
    for _ in range(2):
        blas = build(ctx, layout, rest, idx)
        blas._bounds = box
        tl.append((tb.TLAS(ctx).Build(tb.make_instances(xf, np.zeros(2, np.uint32)), [blas]), blas))
    pose = tb.Pose(ctx).Skin(rest, g["joints"], g["weights"], P.N_JOINTS)
    for f in (1, 0):
        pose.SetPose(g["mats"][f]).Refit(tl[0][1])
        host_refit(tl[1][1], frames[f], idx)
        ra, rb = tl[0][0].Intersect(rays.copy()), tl[1][0].Intersect(rays.copy())
        assert ra.tobytes() == rb.tobytes()
        assert not ra["inst"][ra["t"] < 1e30].any()
        flat = frames[f] if idx is None else P.flatten(frames[f], idx)
        want, sh, _ = oracle_hits(oracle, flat, rays, shadow_from=tuple(rest[:, :3].max(0) * 2))
        check(ra, want, bits=False)      # (through an instance the ray is transformed first: same triangles, t / u / v within the contract's 1e-5)
        assert np.array_equal(tl[0][0].IsOccluded(sh), tl[1][0].IsOccluded(sh))
    pose.free()
    for t, blas in tl:
        t.free(); blas.free()


def test_pose_refit_refuses_what_it_cannot_refit(ctx, g_skin):
    rest = P.rest4(g_skin)
    sc = build(ctx, tb.LAYOUT_CWBVH, rest, None)
    pose = tb.Pose(ctx).Skin(rest[:64], g_skin["joints"][:64], g_skin["weights"][:64], P.N_JOINTS)   # 64 vertices: no whole number of triangles
    pose.SetPose(g_skin["mats"][0])
    with pytest.raises(tb.TbvhError) as e:
        pose.Refit(sc)
    assert e.value.code == -1
    pose.free(); sc.free()


def test_shutdown_frees_the_poses_still_alive(g_skin):
    """A pose belongs to its context as a scene does: closing the context frees a pose the caller kept, device memory included."""
    import ctypes as C
    import gc
    gc.collect()    # (scenes of earlier tests that are only waiting for the collector go now, not between the two readings)
    live = (C.c_uint64 * 2)()
    tb.check(tb.lib.tbvh_debug_device_allocations(live), "tbvh_debug_device_allocations")
    before = (int(live[0]), int(live[1]))
    own = tb.Context(0)
    pose = tb.Pose(own).Skin(P.rest4(g_skin)[:939], g_skin["joints"][:939], g_skin["weights"][:939], P.N_JOINTS)
    pose.SetPose(g_skin["mats"][0])
    tb.check(tb.lib.tbvh_debug_device_allocations(live), "tbvh_debug_device_allocations")
    assert int(live[1]) >= before[1] + 939 * 64
    own.close()
    pose.free()     # (no call into the library: the handle died with the context)
    tb.check(tb.lib.tbvh_debug_device_allocations(live), "tbvh_debug_device_allocations")
    assert (int(live[0]), int(live[1])) == before


# ---- last: a device-resident joint array with an index that is no joint -------------------------------------------------------------------------
def test_bad_device_joint_index_is_reported_and_never_used(ctx, g_skin):
    """The kernel compares every index with n_joints before it forms an address: the vertex with the bad index is left as it was (zero: a new pose's buffer is
    cleared), every other vertex is posed, and the next synchronising call reports TBVH_E_FORMAT once."""
    g = g_skin
    rest = P.rest4(g)
    n, bad_vertex = rest.shape[0], 4321
    joints = g["joints"].copy()
    joints[bad_vertex, 2] = P.N_JOINTS
    d = [ctx.malloc(n * 16) for _ in range(3)]
    for ptr, a in zip(d, (rest, joints, g["weights"])):
        ctx.to_device(ptr, a)
    pose = tb.Pose(ctx).SkinOnDevice(d[0], d[1], d[2], n, P.N_JOINTS)
    pose.SetPose(g["mats"][0])
    with pytest.raises(tb.TbvhError) as e:
        pose.Download()
    assert e.value.code == -5 and "joint" in str(e.value)
    got = pose.Download()               # the status word was reported once and is clear again
    keep = np.arange(n) != bad_vertex
    assert same_bytes(got[keep], g["out"][keep])
    assert not got[bad_vertex].view(np.uint32).any()
    pose.free()
    for ptr in d:
        ctx.free(ptr)
