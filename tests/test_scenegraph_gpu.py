"""The animated scene graph on the device (tbvh_scenegraph_*: kernels_scenegraph.hip; DESIGN.md par. 17) against the golden (the REAL reference's arrays,
tests/golden/graph/synthetic.npz) and against the host twin run in lockstep:
  - after every walk of the scripted sequence the channels' (t, k), the trig flags, the weights, every translation and scale, and every rotation that did not come
    down slerp's trigonometric branch equal the golden BYTEWISE; in the frames without such a rotation so do the local and combined matrices, the instance
    transforms and the joint matrices (a stale joint pair only where the walk before was exact too: it reads that walk's matrix)
  - a rotation from the trigonometric branch (acosf, sinf: the device's math library is not the host's) stays within the fixture's trig_bound of the golden, and the
    hierarchy stays pinned exactly all the same: the device's local / combined / instance / joint matrices equal, bytewise, the walk of the independent plain-C
    restatement (tests/oracle_scenegraph.c) over the T, R, S values DOWNLOADED FROM THE DEVICE (and the host twin's)
  - sizes at which a one-item-per-lane kernel can go wrong: 1 / 63 / 64 / 65 / 257 channels, 1 / 64 / 65 nodes (and the 33-deep chain and the 65-fan of the
    synthetic graph), 1 / 2 / 24 / 65 joints, 1 / 64 / 65 / 77 instances
  - the chain graph -> TLAS rebuild -> trace and graph -> pose -> refit, all from device memory, against the same scene fed the golden arrays from the host
  - a key state overwritten on the device is reported as TBVH_E_FORMAT and never used as an address; tbvh_shutdown frees a graph that is still alive."""
import ctypes as C

import numpy as np
import pytest

import pose_lib as P
import scenegraph_lib as L
import tinybvh_amd as tb
from scenegraph_fixtures import g_drone, g_graph, graph_oracle, synthetic  # noqa: F401
from tinybvh_amd import rays as R

pytestmark = pytest.mark.gpu
MATS = ("local", "combined", "inst", "joints")


def bits_differ(a, b):
    return int((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).sum())


def lockstep(ctx, orc, d, ops, bound, golden=None, exact_frames=()):
    """run ops on a device graph, the host twin and the plain-C restatement (tests/oracle_scenegraph.c) together.  The restatement's T, R, S are replaced by the
    device's before every walk, and the device's matrices must equal ITS walk: the hierarchy is pinned by code that shares nothing with the kernels' header.
    The host twin supplies what the restatement has no notion of: the trig flags and the stale-pair table."""
    dev, host, rest = tb.SceneGraph(ctx, d), tb.HostSceneGraph(d), L.OracleGraph(orc, d)
    rot_node = {}
    for c, (n, t) in enumerate(zip(d["channel_node"], d["channel_target"])):
        if t == 1:
            rot_node.setdefault(int(n), []).append(c)
    stale = dev.Download(L.STALE).astype(bool)
    assert L.same_bits(stale, host.Download(L.STALE).astype(bool))
    frame, prev_exact, n_trig = 0, True, 0
    for op in ops:
        if op[0] == "advance":
            dev.Advance(op[1])
            for a in range(d["n_animations"]):
                host.AdvanceAnimation(a, op[1]); rest.AdvanceAnimation(a, op[1])
        elif op[0] == "advance_animation": dev.AdvanceAnimation(op[1], op[2]); host.AdvanceAnimation(op[1], op[2]); rest.AdvanceAnimation(op[1], op[2])
        elif op[0] == "set_time": dev.SetTime(op[1], op[2]); host.SetTime(op[1], op[2]); rest.SetTime(op[1], op[2])
        elif op[0] == "reset": dev.Reset(op[1]); host.Reset(op[1]); rest.Reset(op[1])
        elif op[0] == "set_local": dev.SetLocal(op[1], op[2]); host.SetLocal(op[1], op[2]); rest.SetLocal(op[1], op[2])
        elif op[0] == "update_nodes": dev.UpdateNodes()
        if op[0] not in ("advance", "update_nodes"):
            continue
        got = {k: dev.Download(w) for k, w in L.WHATS.items()}
        trig = dev.Download(L.TRIG)
        want = golden[frame] if golden is not None else None
        for k, w in (("t", L.CHANNEL_T), ("k", L.CHANNEL_K), ("trig", L.TRIG), ("weights", L.WEIGHTS)):
            a = trig if k == "trig" else got[k]
            assert L.same_bits(a, host.Download(w)), (frame, k)
            if k != "trig":
                assert L.same_bits(a, rest.Download(w)), (frame, k, "restatement")
            if want is not None:
                assert L.same_bits(a, want[k]), (frame, k)
        inexact = np.zeros(got["trs"].shape[0], bool)     # nodes whose rotation the trigonometric branch may have produced
        for n, cs in rot_node.items():
            inexact[n] = bool(trig[cs].any())
        n_trig += int(inexact.sum())
        ref_trs = want["trs"] if want is not None else rest.Download(L.TRS)
        exact_cols = np.ones(got["trs"].shape, bool); exact_cols[inexact, 3:7] = False
        assert bits_differ(np.where(exact_cols, got["trs"], 0), np.where(exact_cols, ref_trs, 0)) == 0, frame
        if inexact.any():
            err = float(np.abs(got["trs"][inexact, 3:7] - ref_trs[inexact, 3:7]).max())
            print(f"frame {frame}: {int(inexact.sum())} rotations from the trigonometric branch, largest deviation {err:.3e} (bound {bound:.3e})")
            assert err <= bound, (frame, err, bound)
        rest.SetTRS(got["trs"]).UpdateNodes()
        host.SetTRS(got["trs"]).UpdateNodes()
        for k in MATS:
            assert L.same_bits(got[k], rest.Download(L.WHATS[k])), (frame, k, bits_differ(got[k], rest.Download(L.WHATS[k])))
            assert L.same_bits(got[k], host.Download(L.WHATS[k])), (frame, k, "host twin")
        if want is not None and frame in exact_frames:
            assert not inexact.any()
            for k in ("local", "combined", "inst"):
                assert L.same_bits(got[k], want[k]), (frame, k)
            keep = np.ones(stale.shape, bool) if prev_exact else ~stale
            assert L.same_bits(got["joints"][keep], want["joints"][keep]), frame
        prev_exact = not inexact.any()
        frame += 1
    dev.free(); host.free(); rest.free()
    return frame, n_trig


@pytest.mark.parametrize("name", ["synthetic", "drone"])
def test_device_equals_the_golden_over_the_whole_sequence(ctx, graph_oracle, name):
    g = L.golden(name)
    frames, n_trig = lockstep(ctx, graph_oracle, L.golden_desc(g), L.golden_ops(g), float(g["trig_bound"][2]), L.golden_frames(g), set(g["exact_frames"].tolist()))
    assert frames == g["t"].shape[0] and n_trig > 0


@pytest.mark.parametrize("n_channels", [1, 63, 64, 65, 257])
def test_channel_counts(ctx, graph_oracle, g_graph, synthetic, n_channels):
    d = synthetic[0].desc(shuffle_seed=5, n_channels=n_channels)
    ops = [op for op in L.ops_synthetic() if not (op[0] in ("reset", "advance_animation", "set_time") and op[1] >= d["n_animations"])]
    lockstep(ctx, graph_oracle, d, ops, float(g_graph["trig_bound"][2]))


@pytest.mark.parametrize("n_nodes", [1, 64, 65])
def test_node_counts(ctx, graph_oracle, g_graph, n_nodes):
    d = L.small(n_nodes, seed=n_nodes).desc(shuffle_seed=3)
    ops = [("advance", 0.0), ("advance", 0.3), ("advance", -0.1), ("advance", 3.5), ("set_time", 0, 0.2), ("advance", 0.05)]
    lockstep(ctx, graph_oracle, d, ops, float(g_graph["trig_bound"][2]))


def test_fresh_joints_flag(ctx, graph_oracle, g_graph):
    d = dict(L.golden_desc(g_graph), flags=tb.SCENEGRAPH_FRESH_JOINTS)
    lockstep(ctx, graph_oracle, d, [("advance", 0.1), ("advance", 0.2)], float(g_graph["trig_bound"][2]))


def test_advance_is_timed_and_refuses_what_the_host_twin_refuses(ctx, g_graph):
    g = tb.SceneGraph(ctx, L.golden_desc(g_graph))
    g.Advance(0.1)
    ctx.synchronize()
    assert ctx.time_last_ms() > 0
    for call in (lambda: g.Advance(float("inf")), lambda: g.SetTime(0, 1e9), lambda: g.AdvanceAnimation(2, 0.1), lambda: g.JointMatrices(4), lambda: g.MorphWeights(10 ** 6)):
        with pytest.raises(tb.TbvhError) as e:
            call()
        assert e.value.code == -1
    with pytest.raises(tb.TbvhError) as e:
        tb.SceneGraph(ctx, dict(L.golden_desc(g_graph), node_of_instance=np.array([10 ** 6], np.uint32)))
    assert e.value.code == -5 and "instance 0" in str(e.value)
    g.free()


# ---- the chain: graph -> TLAS rebuild -> trace, graph -> pose -> refit ---------------------------------------------------------------------------
def test_chain_from_device_memory_equals_the_host_fed_scene(ctx, g_graph):
    d = L.golden_desc(g_graph)
    frame = int(g_graph["exact_frames"][2])          # an all-lerp frame: the golden's matrices are the device's, bit for bit
    gold = L.golden_frames(g_graph)[frame]
    off = d["skin_joint_offset"]
    use = int(np.nonzero(np.diff(off.astype(np.int64)) == P.N_JOINTS)[0][0])                 # the 24-joint skin use poses the bunny's 24-joint rig
    wnode = int(np.nonzero(d["n_weights"] == 3)[0][0])                                       # the 3-weight node drives the 3-target morph bunny
    woff = np.concatenate([[0], np.cumsum(d["n_weights"].astype(np.int64))])
    gs = P.golden("skin_bunny16"); rest = P.rest4(gs)
    pos, _ = P.morph_bunny()
    base = np.zeros((pos.shape[1], 4), np.float32); base[:, :3] = pos[0]
    mats = gold["joints"][off[use]:off[use + 1]]
    weights = gold["weights"][woff[wnode]:woff[wnode + 1]]
    posed = [tb.host_pose_skin(rest, gs["joints"], gs["weights"], mats), tb.host_pose_morph(pos, weights)]
    boxes = [np.concatenate([p[:, :3].min(0), p[:, :3].max(0)]).astype(np.float32) for p in posed]
    assert all(np.isfinite(b).all() for b in boxes)
    xf = gold["inst"].reshape(-1, 4, 4)
    n_inst = xf.shape[0]
    blas_of = (np.arange(n_inst) % 2).astype(np.uint32)
    # the camera looks at the instances' origins from outside their cloud
    c = xf[:, :3, 3].mean(0); ext = float(np.linalg.norm(xf[:, :3, 3].max(0) - xf[:, :3, 3].min(0))) + float(np.linalg.norm(boxes[0][3:] - boxes[0][:3]))
    eye = c + np.array([0.3, 0.2, 0.9], np.float32) * ext
    view = (c - eye) / np.linalg.norm(c - eye)
    rays = R.primary(R.camera(eye, view, 128, 64, 1, 1))

    def scene():
        skin_blas, morph_blas = tb.BVH8_CWBVH(ctx).Build(rest), tb.BVH8_CWBVH(ctx).Build(base)
        tlas = tb.TLAS(ctx).Build(tb.make_instances(np.stack([np.eye(4, dtype=np.float32)] * n_inst), blas_of), [skin_blas, morph_blas])
        return skin_blas, morph_blas, tlas, tb.Pose(ctx).Skin(rest, gs["joints"], gs["weights"], P.N_JOINTS), tb.Pose(ctx).Morph(pos)

    a, b = scene(), scene()
    graph = tb.SceneGraph(ctx, d)
    ops = L.ops_synthetic()[:frame + 1]
    assert all(op[0] == "advance" for op in ops)
    for op in ops:
        graph.Advance(op[1])
    # device-fed: nothing but pointers crosses the host
    a[3].SetPose(graph.JointMatrices(use)[0], on_device=True).Refit(a[0])
    a[4].SetPose(graph.MorphWeights(wnode)[0], on_device=True).Refit(a[1])
    # host-fed: the golden's arrays go up
    b[3].SetPose(mats).Refit(b[0])
    b[4].SetPose(weights).Refit(b[1])
    for s in (a, b):
        s[0]._bounds, s[1]._bounds = boxes
    a[2].RebuildOnDevice(graph.InstanceTransforms()[0], on_device=True)
    b[2].RebuildOnDevice(np.ascontiguousarray(gold["inst"]))
    ra, rb = a[2].Intersect(rays.copy()), b[2].Intersect(rays.copy())
    assert ra.tobytes() == rb.tobytes()
    hit = ra["t"] < 1e30
    assert int(hit.sum()) > 200 and len(set(ra["inst"][hit].tolist())) > 3
    sh = R.shadow(ra, tuple(c + np.array([0.0, 2.0, 0.5], np.float32) * ext), 1e-4)
    oa, ob = a[2].IsOccluded(sh), b[2].IsOccluded(sh)
    assert np.array_equal(oa, ob)
    assert L.same_bits(a[3].Download(), posed[0]) and L.same_bits(a[4].Download(), posed[1])
    graph.free()
    for s in (a, b):
        s[3].free(); s[4].free(); s[2].free(); s[0].free(); s[1].free()


def test_shutdown_frees_a_graph_still_alive(g_graph):
    import gc
    gc.collect()
    live = (C.c_uint64 * 2)()
    tb.check(tb.lib.tbvh_debug_device_allocations(live), "tbvh_debug_device_allocations")
    before = (int(live[0]), int(live[1]))
    own = tb.Context(0)
    g = tb.SceneGraph(own, L.golden_desc(g_graph)).Advance(0.1)
    tb.check(tb.lib.tbvh_debug_device_allocations(live), "tbvh_debug_device_allocations")
    assert int(live[1]) >= before[1] + g.n_nodes * 64 * 4
    own.close()
    g.free()     # (no call into the library: the handle died with the context)
    tb.check(tb.lib.tbvh_debug_device_allocations(live), "tbvh_debug_device_allocations")
    assert (int(live[0]), int(live[1])) == before


# ---- last: a key state that is out of range on the device --------------------------------------------------------------------------------------
def test_bad_device_key_state_is_reported_and_never_used(ctx, g_graph):
    """The kernel compares a channel's k with its sampler's key count before it forms an address: the channel is left as it was (its t, its k, its node's field),
    every other channel runs, and the next synchronising call reports TBVH_E_FORMAT once."""
    d = L.golden_desc(g_graph)
    g, host = tb.SceneGraph(ctx, d), tb.HostSceneGraph(d)
    g.Advance(0.125); host.Advance(0.125)
    chan = int(np.nonzero(d["channel_target"] == 0)[0][7])
    p = C.c_void_p()
    tb.check(tb.lib.tbvh_debug_scenegraph_array(g._h, L.CHANNEL_K, C.byref(p)), "tbvh_debug_scenegraph_array")
    k = g.Download(L.CHANNEL_K)
    bad = k.copy(); bad[chan] = 1 << 30
    ctx.to_device(p.value, bad)
    before = g.Download(L.TRS)
    g.Advance(0.25); host.Advance(0.25)
    with pytest.raises(tb.TbvhError) as e:
        g.Download(L.CHANNEL_K)
    assert e.value.code == -5 and "scene graph" in str(e.value)
    got_k, got_t, got_trs = g.Download(L.CHANNEL_K), g.Download(L.CHANNEL_T), g.Download(L.TRS)      # (reported once; the word is clear again)
    others = np.arange(k.size) != chan
    assert got_k[chan] == 1 << 30 and L.same_bits(got_k[others], host.Download(L.CHANNEL_K)[others])
    assert L.same_bits(got_t[others], host.Download(L.CHANNEL_T)[others]) and got_t[chan] == np.float32(0.125)
    node = int(d["channel_node"][chan])
    assert L.same_bits(got_trs[node, 0:3], before[node, 0:3])                                  # the bad channel's field kept its value
    keep = np.ones(got_trs.shape, bool); keep[node, 0:3] = False
    trig_nodes = np.unique(d["channel_node"][(g.Download(L.TRIG) != 0)])
    keep[trig_nodes, 3:7] = False
    assert bits_differ(np.where(keep, got_trs, 0), np.where(keep, host.Download(L.TRS), 0)) == 0
    ctx.to_device(p.value, np.where(others, got_k, 0).astype(np.int32))                                                     # k = 0 for that channel: the graph is usable again
    g.Advance(0.0)
    g.Download(L.CHANNEL_K)
    g.free(); host.free()
