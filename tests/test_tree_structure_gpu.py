"""Every device code path that WRITES a single-precision BLAS — refit (kernels_refit.hip), BVH2 -> wide conversion (kernels_convert.hip with
cwbvh_encode.h / bvh4_encode.h), LBVH and PLOC build (kernels_build.hip) — checked box by box: the blob is downloaded and tests/tree_check.py
compares every stored child box with the exact float32 box of the triangles beneath it (containment with zero tolerance, float layouts and node
origins bit-exact, quantised planes within the derived number of steps, exponents and steps minimal, every triangle record bit-equal, every triangle
reached exactly once).  Hit parity is asserted only for the two degenerate scenes whose trees no other test builds; the others have it in
test_refit_device.py / test_convert_device.py / test_mesh_gpu.py.

Shapes: the ones that break writers — zero extent on an axis (FLAT) and on all three (POINT, the collapse to one point), coordinates far from the
origin (FAR), equal Morton keys (POINT, TWO), 1..9 triangles, sizes around the wave and block widths, a contraction by 1e-3 followed by an expansion
by 1e6 (exponents and steps must follow DOWN as well as up), and a caterpillar tree that needs several batches of refit passes in every layout."""
import os

import numpy as np
import pytest

import tinybvh_amd as tb
from tinybvh_amd import scenes
import pose_lib as P
import tree_check as tc
from oracle_lib import compare_hits
from test_deep_tree import chain_bvh2
from test_refit_device import deform

pytestmark = pytest.mark.gpu

CW, B4, AL = tb.LAYOUT_CWBVH, tb.LAYOUT_BVH4_GPU, tb.LAYOUT_BVH_GPU
LAYOUTS = [CW, B4, AL]
WIDE = [CW, B4]
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
TINY = (1, 2, 3, 4, 5, 8, 9)
EDGE = (63, 64, 65, 255, 256, 257)
_cache = {}


def scene(name):
    """the scenes of this module, each made once and never written to (callers copy before they change anything)"""
    if name in _cache:
        return _cache[name]
    if name == "S":
        v = scenes.soup(3000, seed=5)
    elif name == "FAR":
        v = scenes.soup(2000, seed=6); v[:, :3] += np.array([1e5, -3e4, 7e3], np.float32)
    elif name == "FLAT":
        v = scenes.soup(500, seed=8); v[:, 2] = 0
    elif name == "POINT":                                  # 700 copies of one triangle: every box, centroid and Morton key equal
        v = np.tile(scenes.soup(1, seed=3), (700, 1))
    elif name == "TWO":                                    # two clusters 1e6 apart: nearly all of the 21-bit cells of a cluster are equal
        a, b = scenes.soup(300, seed=1), scenes.soup(300, seed=2)
        b[:, :3] += np.array([1e6, 0, 0], np.float32)
        v = np.concatenate([a, b])
    elif name.startswith("TINY") or name.startswith("EDGE"):
        v = scenes.soup(int(name[4:]), seed=4 if name[0] == "T" else 9)
    else:
        raise KeyError(name)
    v = np.ascontiguousarray(v, np.float32)
    v.flags.writeable = False
    _cache[name] = v
    return v


def blobs(sc):
    nodes, tris = sc.download_blobs()
    return nodes, (None if sc.layout == B4 else tris)


def checked(sc, verts, label, indices=None, prims=None):
    nodes, tris = blobs(sc)
    F = tc.assert_tree(sc.layout, nodes, tris, verts, indices=indices, prims=prims, label=label)
    print(label, tc.describe(F))
    return F


def build_whole(ctx, layout, verts, **kw):
    """host build without spatial splits (BVH8_CWBVH's default holds pieces of triangles), uploaded"""
    return tb.LAYOUT_CLASSES[layout](ctx).Build(verts, split_budget=0.0, **kw)


def al_from_bvh2(n2):
    """BVH_GPU::ConvertFrom restated (tiny_bvh.h:4612-4655; host_builder.cpp: encode_bvh_gpu): depth-first pre-order, the left child of node k is
    node k + 1, an interior node carries the boxes of both children, leaves are zero but for triCount / firstTri."""
    f = np.ascontiguousarray(n2).view(np.float32).reshape(-1, 8); u = f.view(np.uint32)
    out = np.zeros((f.shape[0], 16), np.float32); ou = out.view(np.uint32)
    stack, nxt = [(0, -1)], 0
    while stack:
        src, parent = stack.pop()
        dst = nxt; nxt += 1
        if parent >= 0:
            ou[parent, 7] = dst
        while True:
            if u[src, 7]:
                ou[dst, 11] = u[src, 7]; ou[dst, 15] = u[src, 3]
                break
            l = int(u[src, 3]); r = l + 1
            out[dst, 0:3] = f[l, 0:3]; out[dst, 4:7] = f[l, 4:7]; out[dst, 8:11] = f[r, 0:3]; out[dst, 12:15] = f[r, 4:7]
            ou[dst, 3] = nxt
            stack.append((r, dst))
            src = l; dst = nxt; nxt += 1
    return ou[:nxt].copy()


# ---- refit ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", LAYOUTS)
def test_refit_deformations_and_back_to_rest(ctx, layout):
    verts = scene("S")
    sc = build_whole(ctx, layout, verts)
    before = checked(sc, verts, "uploaded S")
    nodes0, _ = blobs(sc)
    for amount in (0.05, 0.2, 0.0):
        v2 = deform(verts, amount, seed=3) if amount else verts
        sc.Refit(v2)
        checked(sc, v2, f"S refitted to deform({amount})")
    nodes, _ = blobs(sc)
    if layout == AL:       # nothing is quantised: back at rest the refit must write the very floats the builder wrote
        diff = np.nonzero(np.any(nodes.reshape(-1, 16) != nodes0.reshape(-1, 16), axis=1))[0]
        assert diff.size == 0, f"{diff.size} BVH_GPU nodes differ from the uploaded blob after the refit back to rest, first node {diff[0]}"
    assert before["nodes_reached"] > 100
    sc.free()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_refit_follows_the_scale_down_and_up(ctx, layout):
    """contract by 1e-3, expand to 1e3, flatten to z = 0, collapse to one point, back to rest: exponents (CWBVH) and steps (BVH4_GPU) must come
    down as well as go up, and zero extents take the encoders' special cases"""
    verts = scene("S")
    sc = build_whole(ctx, layout, verts)
    frames = []
    for f in (1e-3, 1e3):
        v = verts.copy(); v[:, :3] *= np.float32(f); frames.append((f"S x {f}", v))
    v = verts.copy(); v[:, 2] = 0; frames.append(("S flattened", v))
    v = verts.copy(); v[:, :3] = np.array([1.5, -2.25, 3.0], np.float32); frames.append(("S at one point", v))
    frames.append(("S at rest", verts))
    for label, v in frames:
        sc.Refit(v)
        checked(sc, v, label)
    sc.free()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_refit_far_from_the_origin(ctx, layout):
    verts = scene("FAR")
    sc = build_whole(ctx, layout, verts)
    v2 = deform(verts, 0.01, seed=1)
    sc.Refit(v2)
    checked(sc, v2, "FAR refitted")
    sc.free()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_refit_tiny_trees(ctx, layout):
    for n in TINY:
        verts = scene(f"TINY{n}")
        sc = build_whole(ctx, layout, verts)
        v2 = deform(verts, 0.05, seed=n)
        sc.Refit(v2)
        checked(sc, v2, f"TINY({n}) refitted")
        sc.free()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_refit_of_a_chain_takes_several_batches_of_passes(ctx, layout):
    """the caterpillar of test_deep_tree.py: ~57 levels 8-wide, ~130 4-wide, 400 binary: more passes than launch_refit runs between two looks at
    the root (6 for CWBVH, 24 for BVH_GPU), and one launch per level for BVH4_GPU"""
    n2, pi, verts = chain_bvh2(400)
    v2 = deform(verts, 0.05, seed=2)
    if layout == AL:
        host = build_whole(ctx, AL, verts)             # the host builder's (shallow) tree over the same triangles
        host.Refit(v2)
        checked(host, v2, "CHAIN, host-built BVH_GPU, refitted")
        host.free()
        sc = tb.BVH_GPU(ctx).Upload(al_from_bvh2(n2), pi, verts)   # and the chain itself
    else:
        sc = tb.LAYOUT_CLASSES[layout](ctx).ConvertFromBVH2(n2, pi, verts)
    F = checked(sc, verts, "CHAIN uploaded")
    assert F["levels"] > {CW: 6, B4: 24, AL: 24}[layout]
    sc.Refit(v2)
    checked(sc, v2, "CHAIN refitted")
    sc.free()


@pytest.mark.parametrize("k", [0, 1])
def test_refit_of_reference_built_blobs(ctx, k):
    """blobs of the real tiny_bvh.h (BVH::Build, and BuildHQ whose leaves share prims): after a refit every leaf box is its whole triangles' box,
    and exactly the prim words the blob held before are reachable"""
    g = np.load(os.path.join(GOLDEN, "soup_2k.npz"))
    verts = g["verts"]
    v2 = deform(verts, 0.03, seed=2)
    made = {CW: lambda: tb.BVH8_CWBVH(ctx).Upload(g[f"cwbvh_nodes_{k}"], g[f"cwbvh_tris_{k}"]),
            AL: lambda: tb.BVH_GPU(ctx).Upload(g[f"bvhgpu_nodes_{k}"], g[f"bvhgpu_idx_{k}"], verts),
            B4: lambda: tb.BVH4_GPU(ctx).Upload(g[f"bvh4_{k}"])}
    for layout in LAYOUTS:
        sc = made[layout]()
        held = tc.check_tree(layout, *blobs(sc), verts)["prims"]
        assert np.array_equal(np.unique(held), np.arange(verts.shape[0] // 3, dtype=np.uint32))
        sc.Refit(v2)
        checked(sc, v2, f"soup_2k k={k} layout {layout} refitted", prims=held)
        sc.free()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_refit_of_an_indexed_mesh(ctx, layout):
    """indices=: the GENERAL instances of the refit kernels"""
    pos, idx = P.bunny(16)
    sc = build_whole(ctx, layout, pos, indices=idx)
    checked(sc, pos, "indexed bunny uploaded", indices=idx)
    p2 = deform(pos, 0.02, seed=5)
    sc.Refit(p2, mesh=True)
    checked(sc, p2, "indexed bunny refitted", indices=idx)
    sc.free()


def test_pose_refit(ctx):
    g = P.golden("skin_bunny16")
    rest = P.rest4(g)
    sc = build_whole(ctx, CW, rest)
    pose = tb.Pose(ctx).Skin(rest, g["joints"], g["weights"], P.N_JOINTS)
    pose.SetPose(g["mats"][1]).Refit(sc)
    posed = pose.Download()                                # the vertices the refit read
    assert not np.array_equal(posed[:, :3], rest[:, :3])
    checked(sc, posed, "skin_bunny16 posed and refitted")
    pose.free(); sc.free()


# ---- conversion -------------------------------------------------------------------------------------------------------------------------------

def bvh2_of(verts):
    h = tb.HostBVH(verts, tb.LAYOUT_BVH2_WALD, max_leaf_tris=3, split_budget=0.0)
    return h.bvh2_nodes(), h.bvh2_prim_idx()


@pytest.mark.parametrize("name", ["S", "FAR", "FLAT", "POINT", "CHAIN"])
@pytest.mark.parametrize("layout", WIDE)
def test_convert(ctx, layout, name):
    if name == "CHAIN":
        n2, pi, verts = chain_bvh2(400)
    else:
        verts = scene(name)
        n2, pi = bvh2_of(verts)
    sc = tb.LAYOUT_CLASSES[layout](ctx).ConvertFromBVH2(n2, pi, verts)
    checked(sc, verts, f"{name} converted")
    if layout == B4:
        # k_b4_refit_level restates bvh4_encode.h, which the conversion includes: on the same boxes (a BVH2 whose boxes are its triangles') the two copies
        # of the arithmetic must write the same bytes
        conv, _ = blobs(sc)
        sc.Refit(verts)
        refit, _ = blobs(sc)
        diff = np.nonzero(np.any(conv != refit, axis=1))[0]
        assert diff.size == 0, f"{diff.size} blocks of the refitted stream differ from the converted one, first block {diff[0]}"
    sc.free()


@pytest.mark.parametrize("layout", WIDE)
def test_convert_tiny_trees(ctx, layout):
    for n in TINY:
        verts = scene(f"TINY{n}")
        n2, pi = bvh2_of(verts)
        sc = tb.LAYOUT_CLASSES[layout](ctx).ConvertFromBVH2(n2, pi, verts)
        checked(sc, verts, f"TINY({n}) converted")
        sc.free()


# ---- device build -----------------------------------------------------------------------------------------------------------------------------

def rays_at(verts, n, seed):
    """n rays from around the scene towards points inside randomly chosen triangles"""
    rng = np.random.default_rng(seed)
    tri = tc.triangles(verts)[:, :, :3]
    t = rng.integers(0, tri.shape[0], n)
    w = rng.random((n, 3), dtype=np.float32) + np.float32(0.05); w /= w.sum(1, keepdims=True)
    target = np.einsum("nk,nkc->nc", w, tri[t]).astype(np.float32)
    O = target + (rng.normal(size=(n, 3)) * 3.0).astype(np.float32)
    return tb.make_rays(O, target - O)


def point_rays_hit_prim_0(sc, oracle, verts):
    """700 triangles at the same place: every hit is a 700-way tie, which the library's rule gives to the smallest prim; t, u, v are one triangle's"""
    rays = rays_at(verts, 4096, seed=7)
    h = tb.HostBVH(verts, tb.LAYOUT_BVH2_WALD, max_leaf_tris=3, split_budget=0.0)
    want = oracle.bvh2_intersect(h.bvh2_nodes(), h.bvh2_prim_idx(), verts, rays)
    got = sc.Intersect(rays.copy())
    hit = want["t"] < 1e30
    assert hit.sum() > 3000
    assert np.array_equal(got["t"] < 1e30, hit)
    assert np.all(got["prim"][hit] == 0), np.unique(got["prim"][hit])[:8]
    for k in ("t", "u", "v"):
        assert np.array_equal(got[k][hit].view(np.uint32), want[k][hit].view(np.uint32)), k


def oracle_over_every_triangle(oracle, verts, rays):
    """The oracle's hit records with its box test taken out: the host BVH2 with every node box opened to +-1e9, so each ray meets each triangle, in the
    oracle's own triangle arithmetic and under its tie rule.  "Hit records do not depend on the tree" holds for BVH::Intersect only while its unpadded
    slab test culls no real hit; at |x| = 1e6, where an ulp is 1/16, it does: of the 8192 rays below the oracle over the host-built tree (any of the
    three host layouts' BVH2) misses two triangles that it hits once the boxes are open (7352 against 7354 hits, the other 7352 records bit-identical)."""
    h = tb.HostBVH(verts, tb.LAYOUT_BVH2_WALD, max_leaf_tris=3, split_budget=0.0)
    n2 = h.bvh2_nodes().copy()
    f = n2.view(np.float32)
    f[:, 0:3] = -1e9; f[:, 4:7] = 1e9
    return oracle.bvh2_intersect(n2, h.bvh2_prim_idx(), verts, rays)


def two_cluster_parity(sc, oracle, verts):
    rays = rays_at(verts, 8192, seed=8)
    want = oracle_over_every_triangle(oracle, verts, rays)
    c = compare_hits(sc.Intersect(rays.copy()), want)      # as test_convert_device.check
    assert c["hitmiss"] == 0 and c["prim_real"] == 0 and c["t_bad"] == 0 and c["uv_bad"] == 0, c
    assert c["tie"] <= max(4, c["hits"] // 1500) and c["onsurf"] <= 4, c
    assert c["bit_identical"] == c["same_prim"], c
    far = rays["O"][:, 0] > 5e5
    assert c["hits"] > 6000 and (want["t"][far] < 1e30).sum() > 2000 and (want["t"][~far] < 1e30).sum() > 2000


def built(ctx, oracle, layout, name, **kw):
    verts = scene(name)
    sc = tb.LAYOUT_CLASSES[layout](ctx).BuildOnDevice(verts, **kw)
    checked(sc, verts, f"{name} built on the device {kw}")
    if name == "POINT":
        point_rays_hit_prim_0(sc, oracle, verts)
    if name == "TWO":
        two_cluster_parity(sc, oracle, verts)
    sc.free()


LBVH = [(CW, 1), (CW, 2), (CW, 3), (B4, 1), (B4, 4)]
PLOC = [(layout, radius) for layout in WIDE for radius in (1, 8, 32)]
BIG = ["S", "FAR", "FLAT", "POINT", "TWO"]
SMALL = [f"TINY{n}" for n in TINY] + [f"EDGE{n}" for n in EDGE]


@pytest.mark.parametrize("name", BIG)
@pytest.mark.parametrize("layout,leaf", LBVH)
def test_lbvh_build(ctx, oracle, layout, leaf, name):
    built(ctx, oracle, layout, name, max_leaf_tris=leaf)


@pytest.mark.parametrize("layout,leaf", LBVH)
def test_lbvh_build_small_and_edge_sizes(ctx, oracle, layout, leaf):
    for name in SMALL:
        built(ctx, oracle, layout, name, max_leaf_tris=leaf)


@pytest.mark.parametrize("name", BIG)
@pytest.mark.parametrize("layout,radius", PLOC)
def test_ploc_build(ctx, oracle, layout, radius, name):
    built(ctx, oracle, layout, name, builder="ploc", radius=radius)


@pytest.mark.parametrize("layout,radius", PLOC)
def test_ploc_build_small_and_edge_sizes(ctx, oracle, layout, radius):
    for name in SMALL:
        built(ctx, oracle, layout, name, builder="ploc", radius=radius)
