"""The animated scene graph on the CPU (tbvh_host_scenegraph_*: tinybvh_amd/csrc/scenegraph.h compiled for the host; DESIGN.md par. 17), no GPU:
  - tests/oracle_scenegraph.c, an independent plain-C restatement (sequential and recursive as the reference, none of the library's tables) == the REAL reference;
    the goldens == that restatement; the host twin == that restatement (these two need no checkout)
  - the host twin == the REAL reference (tests/scenegraph_ref_shim.cpp: tiny_scene.h's Animation::Update and Node::Update unmodified), bytewise, every array after
    every walk of the scripted sequence — slerp's trigonometric branch included, because both sides call the same libm here; skipped without the checkout
  - the committed golden (made through that shim) == the host twin, so the same holds where the reference is absent
  - what the synthetic graph covers, asserted: SPLINE and STEP samplers of each value type, a one-key and a duration-0 sampler, samplers whose first key time is
    > 0, two animations (and two channels of one animation) writing one field, three roots, a chain 33 deep, a fan of 65, 65+ instances, skins of 1, 2, 24 and 65
    joints, a mesh node before its skeleton and one after (stale and fresh pairs), nodes with 2, 3 and 4 morph weights, a non-uniform scale, a projective row, -0
  - every creation-time refusal with its code and message; the time limit; stale joints against TBVH_SCENEGRAPH_FRESH_JOINTS; the ABI is still 5."""
import numpy as np
import pytest

import scenegraph_lib as L
import tinybvh_amd as tb
from scenegraph_fixtures import g_drone, g_graph, graph_oracle, graph_ref, synthetic  # noqa: F401

KEYS = list(L.WHATS)


def assert_frames_equal(got, want, keys=KEYS):
    assert len(got) == len(want)
    for f, (a, b) in enumerate(zip(got, want)):
        for k in keys:
            assert L.same_bits(a[k], b[k]), (f, k, int((np.ascontiguousarray(a[k]).view(np.uint32) != np.ascontiguousarray(b[k]).view(np.uint32)).sum()))


@pytest.mark.parametrize("shuffle", [None, 5, 77], ids=["walk-order", "shuffled5", "shuffled77"])
def test_host_twin_equals_the_real_reference(graph_ref, synthetic, shuffle):
    d = synthetic[0].desc(shuffle_seed=shuffle)
    ops = L.ops_synthetic()
    assert_frames_equal(L.run_ops(tb.HostSceneGraph(d), ops), L.run_ops(L.RefGraph(graph_ref, d), ops))


@pytest.mark.parametrize("shuffle", [None, 5, 77], ids=["walk-order", "shuffled5", "shuffled77"])
def test_restatement_equals_the_real_reference(graph_ref, graph_oracle, synthetic, shuffle):
    """tests/oracle_scenegraph.c — sequential, recursive, written from the reference's text — against the real thing"""
    d = synthetic[0].desc(shuffle_seed=shuffle)
    ops = L.ops_synthetic()
    assert_frames_equal(L.run_ops(L.OracleGraph(graph_oracle, d), ops), L.run_ops(L.RefGraph(graph_ref, d), ops))


@pytest.mark.parametrize("name", ["synthetic", "drone"])
def test_golden_equals_the_restatement(graph_oracle, name):
    g = L.golden(name)
    assert_frames_equal(L.run_ops(L.OracleGraph(graph_oracle, L.golden_desc(g)), L.golden_ops(g)), L.golden_frames(g))


@pytest.mark.parametrize("case", ["walk-order", "shuffled5", "shuffled77", "fresh-joints", "c1", "c63", "c64", "c65", "c257", "n1", "n64", "n65"])
def test_host_twin_equals_the_restatement(graph_oracle, synthetic, case):
    """needs no reference checkout: the library's flat, per-item form (shadowed channels, the table of stale joints) against the sequential restatement"""
    ops = L.ops_synthetic()
    if case[0] == "n":
        d = L.small(int(case[1:]), seed=int(case[1:])).desc(shuffle_seed=3)
        ops = [("advance", 0.0), ("advance", 0.3), ("advance", -0.1), ("advance", 3.5), ("set_time", 0, 0.2), ("advance", 0.05)]
    elif case[0] == "c":
        d = synthetic[0].desc(shuffle_seed=5, n_channels=int(case[1:]))
        ops = [op for op in ops if not (op[0] in ("reset", "advance_animation", "set_time") and op[1] >= d["n_animations"])]
    else:
        d = synthetic[0].desc(shuffle_seed={"walk-order": None, "shuffled5": 5, "shuffled77": 77, "fresh-joints": 5}[case],
                              flags=tb.SCENEGRAPH_FRESH_JOINTS if case == "fresh-joints" else 0)
    assert_frames_equal(L.run_ops(tb.HostSceneGraph(d), ops), L.run_ops(L.OracleGraph(graph_oracle, d), ops))


@pytest.mark.parametrize("n_channels", [1, 63, 64, 65, 257])
def test_channel_prefixes_equal_the_real_reference(graph_ref, synthetic, n_channels):
    d = synthetic[0].desc(shuffle_seed=5, n_channels=n_channels)
    ops = [op for op in L.ops_synthetic() if not (op[0] in ("reset", "advance_animation", "set_time") and op[1] >= d["n_animations"])]
    assert_frames_equal(L.run_ops(tb.HostSceneGraph(d), ops), L.run_ops(L.RefGraph(graph_ref, d), ops))


@pytest.mark.parametrize("n_nodes", [1, 64, 65])
def test_small_trees_equal_the_real_reference(graph_ref, n_nodes):
    d = L.small(n_nodes, seed=n_nodes).desc(shuffle_seed=3)
    ops = [("advance", 0.0), ("advance", 0.3), ("advance", -0.1), ("advance", 3.5), ("set_time", 0, 0.2), ("advance", 0.05)]
    assert_frames_equal(L.run_ops(tb.HostSceneGraph(d), ops), L.run_ops(L.RefGraph(graph_ref, d), ops))


def test_nan_and_negative_steps_behave_as_the_reference(graph_ref):
    d = L.small(9, seed=4).desc()
    ops = [("advance", 0.4), ("advance", -0.7), ("advance", 0.1), ("advance", float("nan")), ("advance", 0.1), ("set_time", 0, 0.3), ("advance", 0.1)]
    got, want = L.run_ops(tb.HostSceneGraph(d), ops), L.run_ops(L.RefGraph(graph_ref, d), ops)
    assert_frames_equal(got, want, ["t", "k"])
    for a, b in zip(got, want):   # (a NaN's payload is not pinned down; where it is a NaN on one side it is on the other, everything else bit for bit)
        for k in ("trs", "local", "combined", "inst", "joints"):
            na, nb = np.isnan(a[k]), np.isnan(b[k])
            assert np.array_equal(na, nb) and L.same_bits(np.where(na, 0, a[k]), np.where(nb, 0, b[k])), k
    assert np.isnan(got[3]["t"]).all() and not np.isnan(got[5]["t"]).any()


@pytest.mark.parametrize("name", ["synthetic", "drone"])
def test_golden_equals_the_host_twin(name):
    g = L.golden(name)
    got = L.run_ops(tb.HostSceneGraph(L.golden_desc(g)), L.golden_ops(g), {"trig": L.TRIG})
    assert_frames_equal(got, L.golden_frames(g), KEYS + ["trig"])


def test_drone_golden_is_the_file_and_the_real_reference(g_drone, graph_ref):
    """the fixture's tables are what the glTF file holds (read with json + numpy), and the real reference run on them gives the fixture's arrays"""
    d = L.gltf_desc(L.drone_path(), graph_ref).desc()
    for k in L.DESC_KEYS:
        if d[k] is not None:
            assert L.same_bits(np.asarray(d[k]).reshape(-1), g_drone["desc_" + k].reshape(-1)), k
    assert_frames_equal(L.run_ops(L.RefGraph(graph_ref, L.golden_desc(g_drone)), L.golden_ops(g_drone)), L.golden_frames(g_drone))


def test_what_the_drone_fixture_covers(g_drone):
    d = L.golden_desc(g_drone)
    assert d["parent"].size == 93 and d["channel_node"].size == 100 and d["node_of_instance"].size == 39 and int((d["parent"] < 0).sum()) == 1
    assert set(d["channel_target"].tolist()) == {0, 1, 2, 3} and set(d["sampler_interpolation"].tolist()) == {L.LINEAR}
    depth = np.zeros(93, np.int64)
    for n in range(93):      # (node i is the i-th node of the walk: a parent comes first)
        depth[n] = 1 + (depth[d["parent"][n]] if d["parent"][n] >= 0 else 0)
    assert depth.max() == 20
    assert float(d["key_times"].max()) == L.DRONE_DURATION
    ops = L.golden_ops(g_drone)
    assert any(op[0] == "set_time" for op in ops)
    t, wrapped = 0.0, False
    for op in ops:
        if op[0] == "advance":
            t += op[1]
            if t >= L.DRONE_DURATION:
                wrapped = True; t -= L.DRONE_DURATION
    assert wrapped
    rot = d["channel_target"] == 1
    assert len(g_drone["exact_frames"]) >= 4 and all(not g_drone["trig"][f].any() for f in g_drone["exact_frames"])
    assert len(g_drone["trig_frames"]) >= 2 and all(g_drone["trig"][f][rot].any() for f in g_drone["trig_frames"])
    assert L.same_bits(g_drone["trig_bound"], L.golden("synthetic")["trig_bound"])


def test_golden_is_the_generator_of_today(g_graph, synthetic):
    d = synthetic[0].desc(shuffle_seed=5)
    for k in L.DESC_KEYS:
        assert L.same_bits(np.asarray(d[k]).reshape(-1), g_graph["desc_" + k].reshape(-1)), k


def test_golden_tolerance_is_rederived(g_graph, g_drone, graph_ref, graph_oracle):
    D, n = L.trig_bound(graph_ref, graph_oracle, [L.golden_desc(g_graph), L.golden_desc(g_drone)])
    u, Dg, bound = g_graph["trig_bound"]
    assert u == L.TRIG_U and np.float32(D) == np.float32(Dg) and bound == 2 * Dg and n == int(g_graph["trig_intervals"])


def test_what_the_synthetic_graph_covers(g_graph, synthetic):
    b, notes = synthetic
    d = L.golden_desc(g_graph)
    interp, kind = d["sampler_interpolation"], d["sampler_type"]
    used = {(int(interp[s]), int(kind[s])) for s in d["channel_sampler"]}
    assert used == {(i, k) for i in (L.LINEAR, L.SPLINE, L.STEP) for k in (L.VEC3, L.QUAT, L.FLOAT)}
    keys = np.diff(d["sampler_key_offset"].astype(np.int64))
    first = d["key_times"][d["sampler_key_offset"][:-1]]; last = d["key_times"][d["sampler_key_offset"][1:] - 1]
    assert (keys == 1).any() and ((keys > 1) & (last == 0)).any() and ((first > 0) & (interp == L.SPLINE) & (keys > 1)).any() and ((first > 0) & (interp == L.LINEAR) & (keys > 1)).any()
    field = {}
    for c, (a, n, t) in enumerate(zip(d["channel_animation"], d["channel_node"], d["channel_target"])):
        field.setdefault((int(n), int(t)), []).append(int(a))
    assert any(len(set(v)) > 1 for v in field.values()) and any(len(v) > len(set(v)) for v in field.values())
    assert int((d["parent"] < 0).sum()) == 3
    depth = {}
    for n in b.preorder():
        depth[n] = 1 + (depth[b.nodes[n]["parent"]] if b.nodes[n]["parent"] >= 0 else 0)
    assert max(depth.values()) >= 33 and max(np.bincount(d["parent"][d["parent"] >= 0])) >= 65
    assert d["node_of_instance"].size >= 65
    assert sorted(np.diff(d["skin_joint_offset"].astype(np.int64)).tolist()) == [1, 2, 24, 65]
    stale = g_graph["stale"]
    off = d["skin_joint_offset"]
    per_use = [stale[off[u]:off[u + 1]] for u in range(4)]
    assert any(s.all() for s in per_use) and any(not s.any() for s in per_use) and any(s.any() and not s.all() for s in per_use)
    assert sorted(set(d["n_weights"].tolist())) == [0, 2, 3, 4]
    weights_keys = {(int(keys[s]), float(last[s])) for s, t in zip(d["channel_sampler"], d["channel_target"]) if t == 3}
    assert any(k == 1 for k, _ in weights_keys) and any(k > 1 and e == 0 for k, e in weights_keys)      # a one-key and a duration-0 weights channel
    m = d["matrix"].reshape(-1, 16)
    assert (np.signbit(m) & (m == 0)).any() and (m[:, 12:15] != 0).any() and any(len({x[0], x[5], x[10]}) == 3 for x in m)
    assert len(g_graph["exact_frames"]) >= 4 and len(g_graph["trig_frames"]) >= 2
    rot = d["channel_target"] == 1
    for f in g_graph["exact_frames"]:
        assert not g_graph["trig"][f].any()
    for f in g_graph["trig_frames"]:
        assert (g_graph["trig"][f][rot]).any()
    assert int(g_graph["trig_intervals"]) > 0 and g_graph["trig_bound"][2] == 2 * g_graph["trig_bound"][1] > 0


def test_stale_joints_against_fresh_joints(g_graph):
    d = L.golden_desc(g_graph)
    ops = [("advance", 0.1), ("advance", 0.2), ("advance", 0.3)]
    stale_run = L.run_ops(tb.HostSceneGraph(d), ops)
    fresh = tb.HostSceneGraph(dict(d, flags=tb.SCENEGRAPH_FRESH_JOINTS))
    fresh_run = L.run_ops(fresh, ops)
    st = g_graph["stale"].astype(bool)
    assert not fresh.Download(L.STALE).any()
    for a, b in zip(stale_run, fresh_run):
        assert L.same_bits(a["combined"], b["combined"]) and L.same_bits(a["inst"], b["inst"])
        assert L.same_bits(a["joints"][~st], b["joints"][~st])
        assert (a["joints"][st] != b["joints"][st]).any(axis=1).all()      # (every joint node moves every frame: last frame's matrix is another one)
    # a stale pair is the fresh formula with LAST walk's joint matrix: frame 0 reads the identity
    off, mesh, joint = d["skin_joint_offset"], d["skin_mesh_node"], d["skin_joint_node"]
    first = stale_run[0]
    for u in range(len(mesh)):
        for p in range(off[u], off[u + 1]):
            if st[p]:
                inv = np.linalg.inv(first["combined"][mesh[u]].reshape(4, 4).astype(np.float64))
                want = inv @ np.eye(4) @ d["skin_inverse_bind"].reshape(-1, 4, 4)[p].astype(np.float64)
                assert np.allclose(first["joints"][p].reshape(4, 4), want, rtol=1e-3, atol=1e-4)


def _tiny():
    b = L.Builder()
    r = b.node(-1); c = b.node(r, n_weights=2)
    b.channel(0, b.sampler(L.LINEAR, L.VEC3, [0, 1], np.zeros((2, 3))), r, 0)
    b.channel(0, b.sampler(L.LINEAR, L.FLOAT, [0, 1], np.zeros(4)), c, 3)
    b.instance(c)
    b.skin(c, [r], [L.IDENT])
    return b.desc()


REFUSALS = [
    ("no nodes", lambda d: d.update(parent=np.zeros(0, np.int32)), -1, "no nodes"),
    ("null node array", lambda d: d.update(scale=None), -1, "null node array"),
    ("null sampler array", lambda d: d.update(key_times=None), -1, "null sampler array"),
    ("null channel array", lambda d: d.update(channel_target=None), -1, "null channel array"),
    ("null skin array", lambda d: d.update(skin_inverse_bind=None), -1, "null skin array"),
    ("unknown flags", lambda d: d.update(flags=8), -1, "unknown flags"),
    ("parent out of range", lambda d: d["parent"].__setitem__(1, 2), -5, "node 1: parent 2 is not a node"),
    ("cycle", lambda d: d["parent"].__setitem__(slice(None), [1, 0]), -5, "cycle"),
    ("visit order twice", lambda d: d.update(visit_order=np.array([0, 0], np.uint32)), -5, "visit_order[1] = 0"),
    ("visit order child first", lambda d: d.update(visit_order=np.array([1, 0], np.uint32)), -5, "node 1 comes before its parent 0"),
    ("key time nan", lambda d: d["key_times"].__setitem__(1, np.nan), -5, "sampler 0: key time 1"),
    ("key time decreasing", lambda d: d["key_times"].__setitem__(slice(2, 4), [1, 0.5]), -5, "sampler 1: key time 1"),
    ("no keys", lambda d: d.update(sampler_key_offset=np.array([0, 0, 4], np.uint32)), -5, "sampler 0 has no keys"),
    ("values too short", lambda d: d.update(sampler_value_offset=np.array([0, 5, 10], np.uint32)), -5, "sampler 0: 5 key values, 6 needed for 2 keys"),
    ("weights values too short", lambda d: d.update(sampler_value_offset=np.array([0, 6, 9], np.uint32)), -5, "sampler 1 has 3 key values, 4 needed for 2 keys and 2 weights"),
    ("bad interpolation", lambda d: d["sampler_interpolation"].__setitem__(0, 3), -5, "sampler 0: interpolation 3"),
    ("channel sampler", lambda d: d["channel_sampler"].__setitem__(0, 2), -5, "channel 0: sampler 2 is not a sampler"),
    ("channel node", lambda d: d["channel_node"].__setitem__(1, 2), -5, "channel 1: node 2 is not a node"),
    ("channel target", lambda d: d["channel_target"].__setitem__(0, 4), -5, "channel 0: target 4"),
    ("channel type", lambda d: d["channel_target"].__setitem__(0, 1), -5, "a rotation channel on sampler 0 of type 0"),
    ("weights on a node without", lambda d: d["channel_node"].__setitem__(1, 0), -5, "a weights channel on node 0, which has no weights"),
    ("channels unsorted", lambda d: (d["channel_animation"].__setitem__(slice(None), [1, 0]), d.update(n_animations=2)), -5, "not sorted by animation"),
    ("channel animation", lambda d: d["channel_animation"].__setitem__(1, 1), -5, "channel 1: animation 1 is not one"),
    ("instance node", lambda d: d["node_of_instance"].__setitem__(0, 9), -5, "instance 0: node 9 is not a node"),
    ("skin mesh node", lambda d: d["skin_mesh_node"].__setitem__(0, 9), -5, "skin use 0: mesh node 9"),
    ("skin without joints", lambda d: d.update(skin_joint_offset=np.array([0, 0], np.uint32)), -5, "skin use 0 has no joints"),
    ("joint node", lambda d: d["skin_joint_node"].__setitem__(0, 9), -5, "skin use 0: joint 0: node 9 is not a node"),
]


@pytest.mark.parametrize("name,patch,code,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_creation_refuses(name, patch, code, text):
    d = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in _tiny().items()}
    tb.HostSceneGraph(d).free()   # (the unpatched descriptor is fine)
    patch(d)
    with pytest.raises(tb.TbvhError) as e:
        tb.HostSceneGraph(d)
    assert e.value.code == code and text in str(e.value), str(e.value)


def test_creation_refuses_counts_beyond_32_bits_and_misaligned_arrays():
    import ctypes as C
    st, keep = tb.scenegraph_desc(_tiny())
    h = C.c_void_p()
    st.n_channels = 1 << 32
    assert tb.lib.tbvh_host_scenegraph_create(C.byref(st), C.byref(h)) == -1 and "beyond 32 bits" in tb.lib.tbvh_last_error().decode()
    st.n_channels = 2
    st.key_times += 2
    assert tb.lib.tbvh_host_scenegraph_create(C.byref(st), C.byref(h)) == -1 and "misaligned" in tb.lib.tbvh_last_error().decode()
    assert tb.lib.tbvh_host_scenegraph_create(None, C.byref(h)) == -1 and "null descriptor" in tb.lib.tbvh_last_error().decode()


def test_times_the_wrap_loop_cannot_digest_are_refused():
    g = tb.HostSceneGraph(_tiny())   # (shortest duration 1: the limit is 65536)
    g.Advance(65536.0)
    for call in (lambda: g.Advance(float("inf")), lambda: g.Advance(65537.0), lambda: g.SetTime(0, -1e6), lambda: g.AdvanceAnimation(0, float("-inf"))):
        with pytest.raises(tb.TbvhError) as e:
            call()
        assert e.value.code == -1 and "wrap loop" in str(e.value)
    with pytest.raises(tb.TbvhError) as e:
        g.AdvanceAnimation(1, 0.1)
    assert e.value.code == -1
    g.Advance(float("nan"))
    assert np.isnan(g.Download(L.CHANNEL_T)).all()


def test_outputs_and_set_local(g_graph):
    import ctypes as C
    d = L.golden_desc(g_graph)
    g = tb.HostSceneGraph(d).Advance(0.25)
    p, n = g.InstanceTransforms()
    assert n == d["node_of_instance"].size
    inst = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), (n, 16))
    assert L.same_bits(inst.copy(), g.Download(L.COMBINED)[d["node_of_instance"]])
    off = d["skin_joint_offset"]
    for u in range(4):
        p, n = g.JointMatrices(u)
        assert n == off[u + 1] - off[u]
        assert L.same_bits(np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), (n, 16)).copy(), g.Download(L.JOINTS)[off[u]:off[u + 1]])
    woff = np.concatenate([[0], np.cumsum(d["n_weights"].astype(np.int64))])
    for node in np.nonzero(d["n_weights"])[0]:
        p, n = g.MorphWeights(int(node))
        assert n == d["n_weights"][node]
        assert L.same_bits(np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), (n,)).copy(), g.Download(L.WEIGHTS)[woff[node]:woff[node + 1]])
    assert g.MorphWeights(int(np.nonzero(d["n_weights"] == 0)[0][0]))[1] == 0
    with pytest.raises(tb.TbvhError):
        g.JointMatrices(4)
    # a node no channel writes keeps the local transform it is given; its subtree follows in the next walk
    quiet = int(np.setdiff1d(np.arange(d["parent"].size), d["channel_node"])[0])
    m = np.arange(16, dtype=np.float32)
    g.SetLocal(quiet, m).UpdateNodes()
    assert L.same_bits(g.Download(L.LOCAL)[quiet], m)


@pytest.mark.parametrize("name", ["synthetic", "drone"])
def test_ancestor_chain_product_equals_the_walk(name):
    """the kernels' form of the walk (every node down its own ancestor list) run on the CPU over the lists creation builds: the bits of the parent-first walk"""
    import ctypes as C
    g = L.golden(name)
    h = tb.HostSceneGraph(L.golden_desc(g))
    n = C.c_uint64(99)
    for op in L.golden_ops(g):
        if op[0] == "advance":
            h.Advance(op[1])
            tb.check(tb.lib.tbvh_debug_host_scenegraph_check_chains(h._h, C.byref(n)), "tbvh_debug_host_scenegraph_check_chains")
            assert n.value == 0


def test_abi_is_still_5():
    assert tb.lib.tbvh_abi_version() == 5
