"""Shared by the box-SAH-builder tests and tools/make_boxbuild_golden.py: the real reference's builds over boxes behind tests/boxbuild_ref_shim.cpp
(compiled per session into a pytest temp dir), the box sets, the golden directory (DESIGN.md par. 20).  The comparisons are sahbuild_lib's."""
import ctypes as C
import os

import numpy as np

import native_build as nb
import tinybvh_amd as tb
from native_build import _i, _u32, _u64, _vp
from sahbuild_lib import assert_same_tree, leaf_sets, node_digest  # noqa: F401  (re-exported)

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "boxbuild")
MIXED_SIZES = (1, 2, 3, 63, 64, 65, 1023, 1024, 1025)
SETS = ("LATTICE1000", "IDENT700", "GEO256", "MIXED1000", "FAR", "FLAT") + tuple(f"MIXED{n}" for n in MIXED_SIZES)
TLAS_SIZES = (1, 2, 3, 64, 65, 1000)
MAX_NODE_BYTES = 24 << 10   # a fixture keeps the node bytes of a small tree; of a larger one their count and SHA-256
_cache = {}


def mixed(n):
    """default_rng(7): centres uniform in [0, 100] x [0, 20] x [0, 100], half extent 0.2 + u, every 50th box 5 + 20 u"""
    rng = np.random.default_rng(7)
    c = rng.uniform(0, 1, (n, 3)) * np.array([100, 20, 100])
    h = 0.2 + rng.uniform(0, 1, (n, 3))
    big = 5 + 20 * rng.uniform(0, 1, (n, 3))
    h[::50] = big[::50]
    return c, h


def boxes(name):
    """(n, 8) float32, BVH::BuildAABB's layout {min.xyz, w, max.xyz, w}; made once and never written to"""
    if ("B", name) in _cache:
        return _cache[("B", name)]
    if name == "LATTICE1000":   # exact ties on all axes
        g = np.stack(np.meshgrid(np.arange(10), np.arange(10), np.arange(10), indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
        lo, hi = g, g + 0.5
    elif name == "IDENT700":
        lo = np.tile(np.array([[1.0, 2.0, 3.0]]), (700, 1)); hi = lo + np.array([0.5, 0.25, 1.0])
    elif name == "GEO256":      # centre (1.25^i, 0, 0), half extent 0.1 * 1.25^i: reaches the rootExtent * 1e-20f gate
        s = (np.float32(1.25) ** np.arange(256, dtype=np.float32)).astype(np.float64)
        c = np.zeros((256, 3)); c[:, 0] = s
        h = np.repeat((0.1 * s)[:, None], 3, 1)
        lo, hi = c - h, c + h
    elif name.startswith("MIXED"):
        c, h = mixed(int(name[5:]))
        lo, hi = c - h, c + h
    elif name == "FAR":
        c, h = mixed(1000)
        c = c + np.array([1e5, -3e4, 7e3])
        lo, hi = c - h, c + h
    elif name == "FLAT":
        c, h = mixed(1000)
        c[:, 2] = 0; h[:, 2] = 0
        lo, hi = c - h, c + h
    else:
        raise KeyError(name)
    a = np.zeros((lo.shape[0], 8), np.float32)
    a[:, 0:3] = lo.astype(np.float32); a[:, 4:7] = hi.astype(np.float32)
    a.flags.writeable = False
    _cache[("B", name)] = a
    return a


def spheres(name):
    """the same set, each box read as a sphere: centre = the box centre, r = half the x extent"""
    if ("S", name) in _cache:
        return _cache[("S", name)]
    b = boxes(name)
    s = np.zeros((b.shape[0], 4), np.float32)
    s[:, :3] = (b[:, 0:3] + b[:, 4:7]) * np.float32(0.5)
    s[:, 3] = (b[:, 4] - b[:, 0]) * np.float32(0.5)
    s.flags.writeable = False
    _cache[("S", name)] = s
    return s


BLAS_BOUNDS = np.array([[-1, -1, -1, 1, 1, 1], [0, 0, 0, 2, 0.5, 1]], np.float32)   # the root boxes of two small BLASes


def instances(n):
    """n UPDATED BLASInstance records (tb.INSTANCE_DTYPE) of two small BLASes: rotations, scales from 0.05 to 20, translations in [0, 100]^3.  The update
    (invTransform, world box) is the library's host restatement of BLASInstance::Update, which tests/test_tlas.py holds to the reference bit for bit."""
    if ("I", n) in _cache:
        return _cache[("I", n)]
    rng = np.random.default_rng(11)
    m = np.zeros((n, 4, 4), np.float64)
    q, _ = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    scale = 0.05 * (20 / 0.05) ** rng.uniform(0, 1, n)
    m[:, :3, :3] = q * scale[:, None, None]
    m[:, :3, 3] = rng.uniform(0, 100, (n, 3))
    m[:, 3, 3] = 1
    inst = tb.make_instances(m.astype(np.float32), (np.arange(n) % 2).astype(np.uint32))
    h = C.c_void_p()
    tb.check(tb.lib.tbvh_host_build_tlas(inst.ctypes.data_as(_vp), n, BLAS_BOUNDS.ctypes.data_as(_vp), 2, C.byref(h)), "tbvh_host_build_tlas")
    tb.lib.tbvh_host_free(h)
    inst.flags.writeable = False
    _cache[("I", n)] = inst
    return inst


class RefBox:
    """The real reference's box builds with threadedBuild = false (boxbuild_ref_shim.cpp)."""
    AABBS, SPHERES, TLAS_WALD, TLAS_GPU = 0, 1, 2, 3

    def __init__(self, so):
        self.lib = L = C.CDLL(so)
        L.bref_build.argtypes = [_i, _vp, _u32]
        L.bref_build.restype = _vp
        L.bref_free.argtypes = [_vp]
        L.bref_blob.argtypes = [_vp, _i, C.POINTER(_vp)]
        L.bref_blob.restype = _u64

    def build(self, which, data):
        """(nodes (n, 8) uint32 — (n, 16) for TLAS_GPU —, primIdx)"""
        a = np.ascontiguousarray(data)
        n = a.nbytes // {0: 32, 1: 16, 2: 192, 3: 192}[which]
        h = self.lib.bref_build(which, a.ctypes.data, n)
        out = []
        for what, width in ((0, 16 if which == 3 else 8), (1, 1)):
            p = _vp()
            cnt = self.lib.bref_blob(h, what, C.byref(p))
            out.append(np.ctypeslib.as_array((C.c_uint32 * (cnt * width)).from_address(p.value)).reshape(cnt, width).copy())
        self.lib.bref_free(h)
        return out[0], out[1].reshape(-1)


def compile_ref_shim(d):
    """the reference with oracle/Makefile's flags; None when the reference is absent"""
    so = nb.compile_ref_shim(d, "boxbuild_ref_shim.cpp")
    return so and RefBox(so)


box_ref = nb.ref_fixture("boxbuild_ref", compile_ref_shim)


def al_leaf_sets(nodes64, idx):
    """the instance indices with every Aila-Laine leaf's range sorted ascending (triCount: word 11, firstTri: word 15)"""
    out = np.array(idx, np.uint32, copy=True)
    for i in np.nonzero(nodes64[:, 11])[0]:
        f, c = int(nodes64[i, 15]), int(nodes64[i, 11])
        out[f:f + c] = np.sort(out[f:f + c])
    return out


# ---- fixtures: what the real reference built, for the GPU tests (the GPU machine has no reference checkout) ---------------------------------------

def golden_names():
    return [f"boxes_{s}" for s in SETS] + [f"spheres_{s}" for s in SETS] + [f"tlas_{n}" for n in TLAS_SIZES]


def golden_path(name):
    return os.path.join(GOLDEN, name.lower() + ".npz")


def make_golden(ref, name):
    """the fixture of one name as a dict of arrays, from the real reference"""
    kind, what = name.split("_", 1)
    if kind == "tlas":
        inst = instances(int(what))
        nodes, idx = ref.build(RefBox.TLAS_GPU, inst)
        idx = al_leaf_sets(nodes, idx)
    else:
        nodes, idx = ref.build(RefBox.AABBS, boxes(what)) if kind == "boxes" else ref.build(RefBox.SPHERES, spheres(what))
        idx = leaf_sets(nodes, idx)
    out = {"sha256": np.array(node_digest(nodes)), "n_nodes": np.array(nodes.shape[0], np.uint32), "prim_idx": idx}
    if nodes.nbytes <= MAX_NODE_BYTES:
        out["nodes"] = nodes
    return out


def load_golden(name):
    d = np.load(golden_path(name))
    return {k: d[k] for k in d.files}


def assert_matches_golden(name, nodes, prim_idx, what=""):
    g = load_golden(name)
    assert nodes.shape[0] == int(g["n_nodes"]), f"{what} {name}: {nodes.shape[0]} nodes, the fixture has {int(g['n_nodes'])}"
    if "nodes" in g:
        assert np.array_equal(nodes, g["nodes"]), f"{what} {name}: nodes differ from the fixture"
    assert node_digest(nodes) == str(g["sha256"]), f"{what} {name}: the node bytes do not hash to the fixture's SHA-256"
    assert np.array_equal(prim_idx, g["prim_idx"]), f"{what} {name}: primIdx differs from the fixture"
