"""Shared by the SBVH-builder tests and tools/make_sbvhbuild_golden.py: the scenes, the real reference's BVH::BuildHQ (the flat form through
oracle/_ref, the indexed form behind tests/sbvhbuild_ref_shim.cpp, compiled per session into a pytest temp dir), the golden directory and the
comparisons (DESIGN.md par. 19)."""
import ctypes as C
import os

import numpy as np

import native_build as nb
from native_build import _i, _u32, _u64, _vp
from tinybvh_amd import scenes
import sahbuild_lib as sl

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "sbvhbuild")
GOLDEN_FULL = ("SOUP500", "FLAT", "LONG300", "LONGFLAT")   # full nodes
GOLDEN_HASHED = ("LONG2000", "ATRIUMROT30K")               # SHA-256 of the nodes, their count, primIdx
GOLDEN_SCENES = GOLDEN_FULL + GOLDEN_HASHED
SOUPS = [f"SOUP{n}" for n in (1, 2, 3, 5, 9, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)]   # around the wave, the block and the tile
# the reference's results (nodes, used references), measured once: they confirm the generators; the tests compare trees
REFERENCE_SIZES = {"SOUP500": (972, 501), "S": (5192, 3013), "FAR": (3612, 2025), "FLAT": (802, 550), "TWO": (1170, 600), "QUADS": (2048, 2048),
                   "LATTICE": (2000, 1000), "POINT": (2, 700), "LONG300": (644, 366), "LONG2000": (3944, 2459), "LONGFLAT": (2308, 2074),
                   "BLOB20K": (21086, 19748), "ATRIUMROT30K": (38796, 30930), "STREET45K": (70888, 45000), "STREETROT262K": (301864, 281157)}
_cache = {}


def longtris(n, seed=11):
    """long thin triangles: many straddlers, fragments split more than once"""
    r = np.random.default_rng(seed); v = np.zeros((n * 3, 4), np.float32)
    c = r.uniform(-10, 10, (n, 3)); d = r.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1)[:, None]
    L = r.uniform(0.2, 12, (n, 1)); e = r.normal(size=(n, 3)) * 0.2
    v[0::3, :3] = c - d * L / 2; v[1::3, :3] = c + d * L / 2; v[2::3, :3] = c + e
    return v


def scene(name):
    """sahbuild_lib's scenes and the ones that make an SBVH builder work, each made once and never written to"""
    if name in _cache:
        return _cache[name]
    if name == "LONG300":
        v = longtris(300)
    elif name == "LONG2000":
        v = longtris(2000)
    elif name == "LONGFLAT":
        v = longtris(1500, seed=13); v[:, 1] = 0
    elif name == "HUGE300":   # coordinates whose areas overflow: the one scene on which a partition leaves one side empty (never compared with the reference)
        v = longtris(300); v[5::13, 2] = 3e37
    elif name == "ATRIUMROT30K":
        v = scenes.rotate(scenes.rotate(scenes.atrium(30000), 1, 0.6), 0, 0.35)
    elif name == "STREETROT262K":
        v = scenes.street_rot(262144)
    else:
        return sl.scene(name)
    v = np.ascontiguousarray(v, np.float32)
    v.flags.writeable = False
    _cache[name] = v
    return v


def used_refs(nodes):
    return int(nodes[nodes[:, 7] > 0, 7].sum())


def ref_flat(reference, verts, threaded=False):
    """(nodes (n, 8) uint32, the used prefix of primIdx) of the real BVH::BuildHQ through oracle/_ref"""
    s = reference.build(verts, hq=True, threaded=threaded)
    nodes = s.blob(1, 0, np.uint32, 8)
    idx = s.blob(1, 1, np.uint32, 1).reshape(-1)
    return nodes, idx[:used_refs(nodes)].copy()   # (Compact allocates primIdx without clearing it: only the leaves' references are defined)


class RefSbvhIndexed:
    """The real reference's BVH::BuildHQ( slice, indices, n ) with threadedBuild = false (sbvhbuild_ref_shim.cpp)."""

    def __init__(self, so):
        self.lib = L = C.CDLL(so)
        L.qref_build.argtypes = [_vp, _u32, _vp, _u32]
        L.qref_build.restype = _vp
        L.qref_free.argtypes = [_vp]
        L.qref_blob.argtypes = [_vp, _i, C.POINTER(_vp)]
        L.qref_blob.restype = _u64

    def build(self, verts, indices):
        v = np.ascontiguousarray(verts, np.float32)
        assert v.ndim == 2 and v.shape[1] == 4
        idx = np.ascontiguousarray(indices, np.uint32).reshape(-1)
        h = self.lib.qref_build(v.ctypes.data, v.shape[0], idx.ctypes.data, idx.size // 3)
        out = []
        for which, width in ((0, 8), (1, 1)):
            p = _vp()
            n = self.lib.qref_blob(h, which, C.byref(p))
            out.append(np.ctypeslib.as_array((C.c_uint32 * (n * width)).from_address(p.value)).reshape(n, width).copy())
        self.lib.qref_free(h)
        return out[0], out[1].reshape(-1)[:used_refs(out[0])].copy()


def compile_ref_shim(d):
    """the reference with oracle/Makefile's flags; None when the reference is absent"""
    so = nb.compile_ref_shim(d, "sbvhbuild_ref_shim.cpp")
    return so and RefSbvhIndexed(so)


sbvh_ref_indexed = nb.ref_fixture("sbvhbuild_ref", compile_ref_shim)


def assert_same_tree(got, want, what=""):
    """node for node and byte for byte (pad node 1 included), reference for reference"""
    nodes, idx = got[0], got[1]
    ref_nodes, ref_idx = want[0], want[1]
    assert nodes.shape == ref_nodes.shape, f"{what}: {nodes.shape[0]} nodes, expected {ref_nodes.shape[0]}"
    if not np.array_equal(nodes, ref_nodes):
        bad = np.nonzero((nodes != ref_nodes).any(axis=1))[0]
        raise AssertionError(f"{what}: {bad.size} of {nodes.shape[0]} nodes differ, first {bad[0]}: {nodes[bad[0]]} != {ref_nodes[bad[0]]}")
    if nodes[0, 7] == 0:
        assert not nodes[1].any(), f"{what}: node 1 is not zero"
    assert idx.shape == ref_idx.shape, f"{what}: {idx.size} references, expected {ref_idx.size}"
    if not np.array_equal(idx, ref_idx):
        bad = np.nonzero(idx != ref_idx)[0]
        raise AssertionError(f"{what}: {bad.size} of {idx.size} references differ, first at {bad[0]}: {idx[bad[0]]} != {ref_idx[bad[0]]}")


def golden_path(name):
    return os.path.join(GOLDEN, name.lower() + ".npz")


def load_golden(name):
    """(nodes or None, sha256 of the node bytes, node count, primIdx)"""
    d = np.load(golden_path(name))
    return (d["nodes"] if "nodes" in d.files else None), str(d["sha256"]), int(d["n_nodes"]), d["prim_idx"]


def assert_matches_golden(name, nodes, prim_idx, what=""):
    g_nodes, sha, n_nodes, g_idx = load_golden(name)
    assert nodes.shape[0] == n_nodes, f"{what} {name}: {nodes.shape[0]} nodes, the fixture has {n_nodes}"
    if g_nodes is not None:
        assert np.array_equal(nodes, g_nodes), f"{what} {name}: nodes differ from the fixture"
    assert sl.node_digest(nodes) == sha, f"{what} {name}: the node bytes do not hash to the fixture's SHA-256"
    assert np.array_equal(prim_idx, g_idx), f"{what} {name}: primIdx differs from the fixture"
