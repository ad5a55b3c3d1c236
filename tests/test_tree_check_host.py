"""tests/tree_check.py proves itself on the CPU: the host encoders' blobs pass it (which also confirms the slack bounds on the encoders the device
code restates), the reference-built golden blobs walk, and every way a writer can go wrong that the checker claims to see — one mutation of a
clean blob each — is reported under the finding named for it."""
import os

import numpy as np
import pytest

import tinybvh_amd as tb
from tinybvh_amd import scenes
import tree_check as tc

LAYOUTS = [tb.LAYOUT_CWBVH, tb.LAYOUT_BVH4_GPU, tb.LAYOUT_BVH_GPU]
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def scene(name):
    if name == "soup3000":
        return scenes.soup(3000, seed=5)
    if name == "blob8000":
        return scenes.blob(8000, seed=3)
    if name == "far2000":
        v = scenes.soup(2000, seed=6); v[:, :3] += np.array([1e5, -3e4, 7e3], np.float32); return v
    if name == "flat":
        v = scenes.soup(500, seed=8); v[:, 2] = 0; return v
    return scenes.soup(int(name), seed=4)


SCENES = ["soup3000", "blob8000", "far2000", "flat", "1", "9"]
WORST = {}        # (layout -> largest slack seen, exponent "+ 1" count) over the host-built trees: the maxima tree_check.py's comment records


def test_layout_numbers_are_the_library_s():
    assert (tc.LAYOUT_BVH_GPU, tc.LAYOUT_BVH4_GPU, tc.LAYOUT_CWBVH) == (tb.LAYOUT_BVH_GPU, tb.LAYOUT_BVH4_GPU, tb.LAYOUT_CWBVH)


def host_blobs(verts, layout):
    """(nodes, tris) of the whole-triangle host build, in the form check_tree takes (BVH_GPU: nodes + primIdx)."""
    h = tb.HostBVH(verts, layout, split_budget=0.0)
    if layout == tb.LAYOUT_BVH_GPU:
        return h.blob(0, np.uint32, 16).reshape(-1, 4).copy(), h.blob(1, np.uint32, 1).copy()
    if layout == tb.LAYOUT_BVH4_GPU:
        return h.blob(0, np.uint32, 4).copy(), None
    return h.blob(0, np.uint32, 4).copy(), h.blob(1, np.uint32, 4).copy()


def gathered(verts, idx):
    """the records a BVH_GPU scene holds on the device: {v0|prim, e1, e2} in primIdx order"""
    return tc.expected_records(tb.LAYOUT_BVH_GPU, tc.triangles(verts))[idx.reshape(-1)].reshape(-1, 4)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", SCENES)
def test_host_built_trees_pass(layout, name):
    """Every clean host blob is accepted — which also confirms the derived slack bounds on the HOST encoders, the ones the device code restates, before
    they are held against device output.  Prints the running maxima that the comment beside the constants in tree_check.py records."""
    verts = scene(name)
    nodes, tris = host_blobs(verts, layout)
    F = tc.assert_tree(layout, nodes, tris, verts, label=f"host {name}")
    w = WORST.setdefault(layout, [0.0, 0])
    w[0] = max(w[0], F["max_slack"]); w[1] += F["exponent_plus_one"]
    print(name, tc.describe(F), "| host maxima so far (slack, exponent + 1 used):", w)
    if layout == tb.LAYOUT_BVH_GPU:
        F = tc.assert_tree(layout, nodes, gathered(verts, tris), verts, label=f"host {name}, gathered records")
        assert F["records_compared"] == verts.shape[0] // 3


@pytest.mark.parametrize("name", ["soup_2k", "atrium_6k", "suzanne_decimated"])
@pytest.mark.parametrize("k", [0, 1])
def test_golden_reference_blobs_walk(name, k):
    """Blobs of the real tiny_bvh.h (BVH::Build and BuildHQ): the walk ends and reaches every triangle.  Containment is only counted: BuildHQ leaves hold
    clipped pieces, and the reference's BVH4_GPU scale falls slightly short of the far face."""
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    verts = g["verts"]
    n = verts.shape[0] // 3
    for layout, nodes, tris in ((tb.LAYOUT_CWBVH, g[f"cwbvh_nodes_{k}"], g[f"cwbvh_tris_{k}"]), (tb.LAYOUT_BVH_GPU, g[f"bvhgpu_nodes_{k}"], g[f"bvhgpu_idx_{k}"].reshape(-1, 1)),
                                (tb.LAYOUT_BVH4_GPU, g[f"bvh4_{k}"], None)):
        F = tc.check_tree(layout, nodes, tris, verts)
        print(name, k, tc.describe(F))
        assert not F["bad_index"] and not F["multi_reached"], (layout, F["bad_index"][:2], F["multi_reached"][:4])
        assert np.array_equal(np.unique(F["prims"]), np.arange(n, dtype=np.uint32)), layout
        if k == 0:
            assert F["prims"].size == n


# ---- mutations --------------------------------------------------------------------------------------------------------------------------------

MUT_SCENE = "soup3000"


@pytest.fixture(scope="module")
def clean():
    verts = scene(MUT_SCENE)
    out = {}
    for layout in LAYOUTS:
        nodes, tris = host_blobs(verts, layout)
        if layout == tb.LAYOUT_BVH_GPU:
            tris = gathered(verts, tris)
        F = tc.assert_tree(layout, nodes, tris, verts)
        out[layout] = (nodes, tris, F)
    return verts, out


def q_byte(layout, nodes, node, slot, axis, side):
    """the byte of `nodes` (viewed as uint8, flat) that holds the quantised plane (node, slot, axis, side)"""
    if layout == tb.LAYOUT_CWBVH:
        return node * 80 + 32 + ((3 if side == "hi" else 0) + axis) * 8 + slot
    block, word = [(0, 3), (1, 3)][side == "hi"] if axis == 0 else (2, 2 * (axis - 1) + (side == "hi"))
    return (node + block) * 16 + word * 4 + slot


def origin_word(layout, node, axis):
    """index into nodes.reshape(-1) of the word holding lo / bmin of `node`"""
    return (node * 20 if layout == tb.LAYOUT_CWBVH else node * 4) + axis


def records(layout, nodes, tris):
    """(array holding the records viewed (-1, 4), function record id -> first block)"""
    return (nodes, lambda r: r) if layout == tb.LAYOUT_BVH4_GPU else (tris, lambda r: 3 * r)


def a_leaf_with_two(F, layout, nodes, tris):
    """(node, slot, first record id, stride in record ids) of a leaf child whose first record has a neighbour behind it, found by decoding the clean
    blob: BVH4_GPU keeps the records of a leaf together, so the leaf holds two; the CWBVH records are one array (the host build makes one-triangle leaves)"""
    b = tc._Blob(layout, nodes, tris)
    need = 2 if layout == tb.LAYOUT_BVH4_GPU else 1
    for node in np.unique(F["planes"]["node"]):
        d = b.decode(np.array([node]))
        leaf = d["valid"][0] & ~d["interior"][0] & (d["count"][0] >= need) & (d["first"][0] + 1 < b.n_rec_blocks // 3)
        if leaf.any():
            s = int(np.nonzero(leaf)[0][0])
            return int(node), s, int(d["first"][0, s]), 3 if layout == tb.LAYOUT_BVH4_GPU else 1
    raise AssertionError("no leaf with two triangles")


def rerun(layout, nodes, tris, verts):
    F = tc.check_tree(layout, nodes, tris, verts)
    with pytest.raises(AssertionError):
        tc.assert_tree(layout, nodes, tris, verts)
    return F


@pytest.mark.parametrize("layout", [tb.LAYOUT_CWBVH, tb.LAYOUT_BVH4_GPU])
def test_mutation_hi_plane_one_quantum_low_is_a_containment_finding(clean, layout):
    verts, blobs = clean
    nodes, tris, F = blobs[layout]
    P = F["planes"]
    ok = (P["qhi"] >= 1) & (P["step"] > 0) & (P["slack_hi"] < 0.5)
    r, a = [int(x[0]) for x in np.nonzero(ok)]
    m = nodes.copy()
    m.view(np.uint8).reshape(-1)[q_byte(layout, nodes, int(P["node"][r]), int(P["slot"][r]), a, "hi")] -= 1
    G = rerun(layout, m, tris, verts)
    assert (int(P["node"][r]), int(P["slot"][r]), a, "hi") in [f[:4] for f in G["containment"]]


@pytest.mark.parametrize("layout", [tb.LAYOUT_CWBVH, tb.LAYOUT_BVH4_GPU])
def test_mutation_lo_plane_three_quanta_low_is_a_tightness_finding(clean, layout):
    verts, blobs = clean
    nodes, tris, F = blobs[layout]
    P = F["planes"]
    ok = (P["qlo"] >= 3) & (P["step"] > 4 * P["guard"])
    r, a = [int(x[0]) for x in np.nonzero(ok)]
    m = nodes.copy()
    m.view(np.uint8).reshape(-1)[q_byte(layout, nodes, int(P["node"][r]), int(P["slot"][r]), a, "lo")] -= 3
    G = rerun(layout, m, tris, verts)
    assert not G["containment"]
    assert (int(P["node"][r]), int(P["slot"][r]), a, "lo") in [f[:4] for f in G["slack_over"]]


def test_mutation_cwbvh_exponent_two_too_high_is_an_exponent_finding(clean):
    verts, blobs = clean
    nodes, tris, F = blobs[tb.LAYOUT_CWBVH]
    P = F["planes"]
    r, a = [int(x[0]) for x in np.nonzero((P["qhi"] >= 8) & (P["qhi"] <= 250))]   # a plane that stays in range and distinct when its quantum grows fourfold
    node = int(P["node"][r])
    m = nodes.copy()
    b = m.view(np.uint8).reshape(-1, 80)
    assert int(b[node, 12 + a].view(np.int8)) < 120
    b[node, 12 + a] = np.uint8((int(b[node, 12 + a].view(np.int8)) + 2) & 255)
    lo = b[node, 32 + 8 * a: 40 + 8 * a]; hi = b[node, 32 + 8 * (3 + a): 40 + 8 * (3 + a)]
    lo[:] = lo >> 2                                                      # requantised conservatively: floor for lo, ceil for hi
    hi[:] = (hi.astype(np.uint16) + 3) >> 2
    G = rerun(tb.LAYOUT_CWBVH, m, tris, verts)
    assert not G["containment"] and not G["slack_over"]
    assert [f[:3] for f in G["exponent_over"]] == [(node, -1, a)]


@pytest.mark.parametrize("layout", [tb.LAYOUT_CWBVH, tb.LAYOUT_BVH4_GPU])
def test_mutation_origin_one_ulp_down_is_an_exactness_finding(clean, layout):
    verts, blobs = clean
    nodes, tris, F = blobs[layout]
    P = F["planes"]
    r, a = [int(x[0]) for x in np.nonzero((P["step"] > 0) & (P["tlo"] != 0))]       # an origin that is an ordinary number on an axis with extent
    node = int(P["node"][r])
    m = nodes.copy()
    w = m.reshape(-1)[origin_word(layout, node, a): origin_word(layout, node, a) + 1]
    w.view(np.float32)[0] = np.nextafter(w.view(np.float32)[0], np.float32(-np.inf))
    G = rerun(layout, m, tris, verts)
    assert (node, -1, a, "origin") in [f[:4] for f in G["inexact"]]


@pytest.mark.parametrize("direction,finding", [(-1, "containment"), (+1, "inexact")])
def test_mutation_bvh_gpu_child_max_one_ulp(clean, direction, finding):
    """down: the box no longer holds its triangles; up: the stale box a refit that never shrinks would leave"""
    verts, blobs = clean
    nodes, tris, F = blobs[tb.LAYOUT_BVH_GPU]
    P = F["planes"]
    r, a = [int(x[0]) for x in np.nonzero((P["phi"] == P["thi"]) & (P["thi"] > P["tlo"]) & (P["thi"] != 0))]   # a clean, non-degenerate face
    node, slot = int(P["node"][r]), int(P["slot"][r])
    m = nodes.copy()
    w = m.reshape(-1, 16)[node, (4 if slot == 0 else 12) + a: (4 if slot == 0 else 12) + a + 1].view(np.float32)
    w[0] = np.nextafter(w[0], np.float32(direction * np.inf))
    G = rerun(tb.LAYOUT_BVH_GPU, m, tris, verts)
    assert (node, slot, a, "hi") in [f[:4] for f in G[finding]]
    if direction > 0:
        assert not G["containment"]


def test_mutation_bvh4_step_too_short_is_a_reach_finding(clean):
    verts, blobs = clean
    nodes, tris, F = blobs[tb.LAYOUT_BVH4_GPU]
    P = F["planes"]
    r = int(np.argmax(P["step"][:, 0])); node = int(P["node"][r])        # the widest node: the root
    far = F["node_truth"][1][node, 0]
    m = nodes.copy()
    bmin = m[node, 0:1].view(np.float32); e255 = m[node + 1, 0:1].view(np.float32)
    e255[0] = np.nextafter((far - bmin[0]) / np.float32(255), np.float32(0))    # just short of the far face, then settled ulp by ulp
    for _ in range(64):
        if bmin[0] + e255[0] * np.float32(255) < far:
            break
        e255[0] = np.nextafter(e255[0], np.float32(0))
    else:
        raise AssertionError("the step did not come to stop short of the far face within 64 ulps")
    G = rerun(tb.LAYOUT_BVH4_GPU, m, tris, verts)
    assert (node, -1, 0) in [f[:3] for f in G["short_reach"]]
    assert any(f[0] == node and f[2] == 0 and f[3] == "hi" for f in G["containment"])


def test_mutation_bvh4_stale_large_step_is_a_step_finding(clean):
    """the step a refit would leave behind if e255 never came back down after the mesh contracted: every plane is still close IN ITS UNITS"""
    verts, blobs = clean
    nodes, tris, F = blobs[tb.LAYOUT_BVH4_GPU]
    P = F["planes"]
    r = int(np.nonzero((P["step"][:, 1] > 0) & (P["qhi"][:, 1] >= 2))[0][0])    # a node with extent in y
    node = int(P["node"][r])
    m = nodes.copy()
    e255 = m[node + 1, 1:2].view(np.float32)
    e255[0] *= np.float32(2)
    qb = m.view(np.uint8).reshape(-1, 16)
    qb[node + 2, 0:4] >>= 1                                             # ymin: floor
    qb[node + 2, 4:8] = (qb[node + 2, 4:8].astype(np.uint16) + 1) >> 1   # ymax: ceil
    G = rerun(tb.LAYOUT_BVH4_GPU, m, tris, verts)
    assert not G["containment"] and not G["slack_over"]
    assert [f[:3] for f in G["step_over"]] == [(node, -1, 1)]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_mutation_duplicated_prim_word_is_a_topology_and_a_record_finding(clean, layout):
    verts, blobs = clean
    nodes, tris, F = blobs[layout]
    if layout == tb.LAYOUT_BVH_GPU:
        first, stride = int(np.nonzero(nodes.reshape(-1, 16)[:, 11] >= 2)[0][0]), 1
        first = int(nodes.reshape(-1, 16)[first, 15])
    else:
        _, _, first, stride = a_leaf_with_two(F, layout, nodes, tris)
    m, t = nodes.copy(), None if tris is None else tris.copy()
    arr, block = records(layout, m, t)
    pb = 2 if layout == tb.LAYOUT_CWBVH else 0
    arr[block(first) + pb, 3] = arr[block(first + stride) + pb, 3]
    G = rerun(layout, m, t, verts)
    n = verts.shape[0] // 3
    assert G["prims"].size == n and np.unique(G["prims"]).size == n - 1
    assert len(G["record_mismatch"]) == 1


@pytest.mark.parametrize("layout", [tb.LAYOUT_CWBVH, tb.LAYOUT_BVH4_GPU])
def test_mutation_dropped_child_is_a_missing_primitive(clean, layout):
    verts, blobs = clean
    nodes, tris, F = blobs[layout]
    node, slot, first, stride = a_leaf_with_two(F, layout, nodes, tris)
    m = nodes.copy()
    if layout == tb.LAYOUT_CWBVH:
        m.view(np.uint8).reshape(-1, 80)[node, 24 + slot] = 0          # meta of that slot
    else:
        m[node + 3, slot] = 0                                           # childInfo
    G = rerun(layout, m, tris, verts)
    assert G["prims"].size < verts.shape[0] // 3


@pytest.mark.parametrize("layout", LAYOUTS)
def test_mutation_edge_one_ulp_off_is_a_record_finding(clean, layout):
    verts, blobs = clean
    nodes, tris, F = blobs[layout]
    if layout == tb.LAYOUT_BVH_GPU:
        first = int(np.nonzero(tris.reshape(-1, 3, 4)[:, 1, 0].view(np.float32) != 0)[0][0])   # a record whose e1.x is an ordinary number
    else:
        _, _, first, _ = a_leaf_with_two(F, layout, nodes, tris)
    m, t = nodes.copy(), None if tris is None else tris.copy()
    arr, block = records(layout, m, t)
    w = arr[block(first) + 1, 0:1].view(np.float32)                     # e1 is the middle block in every layout
    w[0] = np.nextafter(w[0], np.float32(np.inf))
    G = rerun(layout, m, t, verts)
    assert len(G["record_mismatch"]) == 1 and G["record_mismatch"][0][2] == first
    assert not G["containment"] and not G["inexact"]
