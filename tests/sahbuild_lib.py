"""Shared by the SAH-builder tests and tools/make_sahbuild_golden.py: the real reference's BVH::Build behind tests/sahbuild_ref_shim.cpp (compiled
per session into a pytest temp dir), the scenes, the golden directory and the comparisons (DESIGN.md par. 18)."""
import ctypes as C
import hashlib
import os

import numpy as np

import native_build as nb
from native_build import _i, _u32, _u64, _vp
from tinybvh_amd import scenes

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "sahbuild")
GOLDEN_SCENES = ("SOUP500", "FLAT", "QUADS", "STREET45K")
_cache = {}


def quad_grid(n=32):
    """n x n identical unit quads (two triangles each) in the plane z = 0: exact cost ties between bins and between the x and y axes"""
    v = np.zeros((n * n * 6, 4), np.float32)
    q = np.array([[0, 0], [1, 0], [1, 1], [0, 0], [1, 1], [0, 1]], np.float32)
    k = 0
    for y in range(n):
        for x in range(n):
            v[k:k + 6, 0] = q[:, 0] + x
            v[k:k + 6, 1] = q[:, 1] + y
            k += 6
    return v


def lattice(n=10):
    """n^3 small identical triangles on an integer lattice: ties on all three axes"""
    g = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    t = np.array([[0, 0, 0], [0.25, 0, 0], [0, 0.25, 0.25]], np.float32)
    v = np.zeros((g.shape[0] * 3, 4), np.float32)
    v[:, :3] = (g[:, None, :] + t[None, :, :]).reshape(-1, 3)
    return v


def scene(name):
    """the scenes of the SAH-builder tests, each made once and never written to"""
    if name in _cache:
        return _cache[name]
    if name.startswith("SOUP"):
        n = int(name[4:])
        v = scenes.soup(n, seed=5 if n == 500 else 4)
    elif name == "S":
        v = scenes.soup(3000, seed=5)
    elif name == "FAR":
        v = scenes.soup(2000, seed=6); v[:, :3] += np.array([1e5, -3e4, 7e3], np.float32)
    elif name == "FLAT":
        v = scenes.soup(500, seed=8); v[:, 2] = 0
    elif name == "POINT":
        v = np.tile(scenes.soup(1, seed=3), (700, 1))
    elif name == "TWO":
        a, b = scenes.soup(300, seed=1), scenes.soup(300, seed=2)
        b[:, :3] += np.array([1e6, 0, 0], np.float32)
        v = np.concatenate([a, b])
    elif name == "QUADS":
        v = quad_grid(32)
    elif name == "LATTICE":
        v = lattice(10)
    elif name == "ATRIUM30K":
        v = scenes.atrium(30000)
    elif name == "STREET45K":
        v = scenes.street(45000)
    elif name == "BLOB20K":
        v = scenes.blob(20000)
    elif name == "ATRIUM262K":
        v = scenes.atrium(262267)
    else:
        raise KeyError(name)
    v = np.ascontiguousarray(v, np.float32)
    v.flags.writeable = False
    _cache[name] = v
    return v


class RefSah:
    """The real reference's BVH::Build with threadedBuild = false (sahbuild_ref_shim.cpp)."""

    def __init__(self, so):
        self.lib = L = C.CDLL(so)
        L.sref_build.argtypes = [_vp, _u32, _vp, _u32, _u32]
        L.sref_build.restype = _vp
        L.sref_free.argtypes = [_vp]
        L.sref_blob.argtypes = [_vp, _i, C.POINTER(_vp)]
        L.sref_blob.restype = _u64

    def build(self, verts, indices=None, split_leafs=0):
        """(nodes (n, 8) uint32, primIdx)"""
        v = np.ascontiguousarray(verts, np.float32)
        assert v.ndim == 2 and v.shape[1] == 4
        if indices is None:
            h = self.lib.sref_build(v.ctypes.data, v.shape[0], None, v.shape[0] // 3, split_leafs)
        else:
            idx = np.ascontiguousarray(indices, np.uint32).reshape(-1)
            h = self.lib.sref_build(v.ctypes.data, v.shape[0], idx.ctypes.data, idx.size // 3, split_leafs)
        out = []
        for which, width in ((0, 8), (1, 1)):
            p = _vp()
            n = self.lib.sref_blob(h, which, C.byref(p))
            out.append(np.ctypeslib.as_array((C.c_uint32 * (n * width)).from_address(p.value)).reshape(n, width).copy())
        self.lib.sref_free(h)
        return out[0], out[1].reshape(-1)


def compile_ref_shim(d):
    """the reference with oracle/Makefile's flags; None when the reference is absent"""
    so = nb.compile_ref_shim(d, "sahbuild_ref_shim.cpp")
    return so and RefSah(so)


sah_ref = nb.ref_fixture("sahbuild_ref", compile_ref_shim)


def leaf_sets(nodes, prim_idx):
    """primIdx with every leaf's range sorted ascending (the builders' output contract; the reference's order inside a leaf is its partition's)"""
    out = np.array(prim_idx, np.uint32, copy=True)
    leaves = np.nonzero(nodes[:, 7])[0]
    for i in leaves:
        f, c = int(nodes[i, 3]), int(nodes[i, 7])
        out[f:f + c] = np.sort(out[f:f + c])
    return out


def assert_same_tree(nodes, prim_idx, ref_nodes, ref_idx, what=""):
    """node for node and byte for byte (pad node 1 included); every leaf's set the reference's, ascending; primIdx a permutation"""
    assert nodes.shape == ref_nodes.shape, f"{what}: {nodes.shape[0]} nodes, the reference has {ref_nodes.shape[0]}"
    if not np.array_equal(nodes, ref_nodes):
        bad = np.nonzero((nodes != ref_nodes).any(axis=1))[0]
        raise AssertionError(f"{what}: {bad.size} of {nodes.shape[0]} nodes differ, first {bad[0]}: {nodes[bad[0]]} != {ref_nodes[bad[0]]}")
    assert not nodes[1].any(), f"{what}: node 1 is not zero"
    assert np.array_equal(np.sort(prim_idx), np.arange(prim_idx.size, dtype=np.uint32)), f"{what}: primIdx is not a permutation"
    assert np.array_equal(prim_idx, leaf_sets(ref_nodes, ref_idx)), f"{what}: a leaf's primitives are not the reference's in ascending order"


def node_digest(nodes):
    return hashlib.sha256(np.ascontiguousarray(nodes, np.uint32).tobytes()).hexdigest()


def golden_path(name):
    return os.path.join(GOLDEN, name.lower() + ".npz")


def load_golden(name):
    """(nodes or None, sha256 of the node bytes, node count, primIdx with sorted leaves)"""
    d = np.load(golden_path(name))
    return (d["nodes"] if "nodes" in d.files else None), str(d["sha256"]), int(d["n_nodes"]), d["prim_idx"]


def assert_matches_golden(name, nodes, prim_idx, what=""):
    g_nodes, sha, n_nodes, g_idx = load_golden(name)
    assert nodes.shape[0] == n_nodes, f"{what} {name}: {nodes.shape[0]} nodes, the fixture has {n_nodes}"
    if g_nodes is not None:
        assert np.array_equal(nodes, g_nodes), f"{what} {name}: nodes differ from the fixture"
    assert node_digest(nodes) == sha, f"{what} {name}: the node bytes do not hash to the fixture's SHA-256"
    assert np.array_equal(prim_idx, g_idx), f"{what} {name}: primIdx differs from the fixture"


# ---- wide blobs ---------------------------------------------------------------------------------------------------------------------------
# The device conversion (kernels_convert.hip) numbers a level's nodes in the order its atomics come back: two conversions of ONE BVH2 may give the
# same nodes in another order (tests/test_mesh_gpu.py: same_built).  So a blob made from the device-built BVH2 is compared byte for byte with the
# conversion of the host twin's BVH2, and where the bytes differ, as node boxes and triangle records in sorted order.  (The BVH2 that goes into the conversion is itself compared byte for byte, every time.)

def bvh4_nodes(blocks):
    """the node boxes of a BVH4_GPU stream (3 blocks per node: frame + quantised planes), found by walking it"""
    out, todo = [], [0]
    while todo:
        off = todo.pop()
        out.append(blocks[off:off + 3].reshape(-1))
        for w in blocks[off + 3]:
            if w and not (w >> 31):
                todo.append(int(w))
    return np.array(out)


def node_boxes(layout_is_cwbvh, nodes):
    if layout_is_cwbvh:   # n0 (origin, exponents, imask) and the quantised planes n2..n4; n1 holds child / triangle numbers
        n = nodes.reshape(-1, 20)
        rows = np.concatenate([n[:, :4], n[:, 8:]], 1)
    else:
        rows = bvh4_nodes(nodes)
    return rows[np.lexsort(rows.T[::-1])]


def sorted_rows(a, width):
    rows = a.reshape(-1, width)
    return rows[np.lexsort(rows.T[::-1])]


def assert_same_blobs(is_cwbvh, a, a2, b, what):
    """a, a2: two conversions of the host twin's BVH2 (nodes, tris); b: the blob under test.  Equal bytes, or — the order of the atomics differs from
    run to run, so that two runs agreed says nothing about a third — the same node boxes and triangle records in another order."""
    assert a[0].shape == b[0].shape and a[1].shape == b[1].shape, what
    if np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]):
        return True
    assert np.array_equal(node_boxes(is_cwbvh, a[0]), node_boxes(is_cwbvh, a2[0])), "two conversions of one BVH2 give different node boxes"
    assert np.array_equal(node_boxes(is_cwbvh, a[0]), node_boxes(is_cwbvh, b[0])), f"{what}: node boxes differ"
    if is_cwbvh:
        assert np.array_equal(sorted_rows(a[1], 12), sorted_rows(b[1], 12)), f"{what}: triangle records differ"
    return False
