"""Shared by the scene graph tests (test_scenegraph_host.py, test_scenegraph_gpu.py) and tools/make_scenegraph_golden.py (so: NumPy, the package's ctypes
layer and the compilers only; no GPU): a builder for scene graph descriptors, the seeded synthetic graph, the scripted frame sequence,
the real reference behind tests/scenegraph_ref_shim.cpp (compiled per session into a temp dir when the reference checkout is present), the slerp tolerance of
tests/oracle_scenegraph.c, and the goldens under tests/golden/graph (DESIGN.md par. 17)."""
import ctypes as C
import os

import numpy as np

import native_build as nb

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "graph")
LINEAR, SPLINE, STEP = 0, 1, 2
VEC3, QUAT, FLOAT = 0, 1, 2
TRS, LOCAL, COMBINED, CHANNEL_T, CHANNEL_K, INSTANCES, JOINTS, WEIGHTS, STALE, TRIG = range(10)
WHATS = {"trs": TRS, "local": LOCAL, "combined": COMBINED, "t": CHANNEL_T, "k": CHANNEL_K, "inst": INSTANCES, "joints": JOINTS, "weights": WEIGHTS}
IDENT = np.eye(4, dtype=np.float32).reshape(16)


# ---- descriptors ---------------------------------------------------------------------------------------------------------------------------
class Builder:
    """Nodes are added parent first, children in visit order; desc() numbers them in that (depth-first) order, or shuffled with an explicit visit_order."""

    def __init__(self):
        self.nodes, self.samplers, self.channels, self.instances, self.skins = [], [], [], [], []

    def node(self, parent=-1, t=(0, 0, 0), r=(1, 0, 0, 0), s=(1, 1, 1), matrix=IDENT, local=None, n_weights=0, weights=None):
        self.nodes.append(dict(parent=parent, t=np.float32(t), r=np.float32(r), s=np.float32(s), matrix=np.float32(matrix).reshape(16),
                               local=np.float32(matrix if local is None else local).reshape(16), n_weights=n_weights,
                               weights=np.zeros(n_weights, np.float32) if weights is None else np.float32(weights)))
        return len(self.nodes) - 1

    def sampler(self, interp, kind, times, values):
        self.samplers.append((interp, kind, np.float32(times).reshape(-1), np.float32(values).reshape(-1)))
        return len(self.samplers) - 1

    def channel(self, anim, sampler, node, target):
        self.channels.append((anim, sampler, node, target))

    def instance(self, node):
        self.instances.append(node)

    def skin(self, mesh_node, joints, inverse_bind):
        self.skins.append((mesh_node, list(joints), np.float32(inverse_bind).reshape(-1, 16)))

    def preorder(self):
        kids = {}
        for i, n in enumerate(self.nodes):
            kids.setdefault(n["parent"], []).append(i)
        out, stack = [], list(reversed(kids.get(-1, [])))
        while stack:
            i = stack.pop()
            out.append(i)
            stack.extend(reversed(kids.get(i, [])))
        return out

    def desc(self, shuffle_seed=None, n_channels=None, flags=0):
        """the dict tinybvh_amd.scenegraph_desc takes.  Without a seed node i of the descriptor is the i-th node visited and visit_order is absent; with one
        the numbering is a random permutation and visit_order lists the walk."""
        order = self.preorder()
        n = len(order)
        if shuffle_seed is None:
            new_of = np.empty(n, np.int64); new_of[order] = np.arange(n)
            visit = None
        else:
            new_of = np.random.default_rng(shuffle_seed).permutation(n)
            visit = new_of[order].astype(np.uint32)
        old_of = np.argsort(new_of)
        nd = [self.nodes[i] for i in old_of]
        channels = sorted(self.channels, key=lambda c: c[0])[:n_channels]   # (stable: by animation, creation order within one)
        koff = np.cumsum([0] + [s[2].size for s in self.samplers]).astype(np.uint32)
        voff = np.cumsum([0] + [s[3].size for s in self.samplers]).astype(np.uint32)
        joff = np.cumsum([0] + [len(s[1]) for s in self.skins]).astype(np.uint32)
        cat = lambda parts, dt: np.concatenate([np.asarray(p, dt).reshape(-1) for p in parts]) if parts else np.zeros(0, dt)
        d = dict(flags=flags, parent=np.array([-1 if x["parent"] < 0 else new_of[x["parent"]] for x in nd], np.int32), visit_order=visit,
                 translation=cat([x["t"] for x in nd], np.float32), rotation=cat([x["r"] for x in nd], np.float32), scale=cat([x["s"] for x in nd], np.float32),
                 matrix=cat([x["matrix"] for x in nd], np.float32), local_transform=cat([x["local"] for x in nd], np.float32),
                 n_weights=np.array([x["n_weights"] for x in nd], np.uint32), weights=cat([x["weights"] for x in nd], np.float32),
                 sampler_interpolation=np.array([s[0] for s in self.samplers], np.uint32), sampler_type=np.array([s[1] for s in self.samplers], np.uint32),
                 sampler_key_offset=koff, sampler_value_offset=voff, key_times=cat([s[2] for s in self.samplers], np.float32),
                 key_values=cat([s[3] for s in self.samplers], np.float32),
                 n_animations=(max(c[0] for c in channels) + 1) if channels else 0,
                 channel_animation=np.array([c[0] for c in channels], np.uint32), channel_sampler=np.array([c[1] for c in channels], np.uint32),
                 channel_node=np.array([new_of[c[2]] for c in channels], np.uint32), channel_target=np.array([c[3] for c in channels], np.uint32),
                 node_of_instance=np.array([new_of[i] for i in self.instances], np.uint32),
                 skin_mesh_node=np.array([new_of[s[0]] for s in self.skins], np.uint32), skin_joint_offset=joff,
                 skin_joint_node=cat([[new_of[j] for j in s[1]] for s in self.skins], np.uint32), skin_inverse_bind=cat([s[2] for s in self.skins], np.float32))
        if not self.samplers:
            for k in ("sampler_interpolation", "sampler_type", "sampler_key_offset", "sampler_value_offset", "key_times", "key_values"):
                d[k] = None
        if not self.skins:
            for k in ("skin_mesh_node", "skin_joint_offset", "skin_joint_node", "skin_inverse_bind"):
                d[k] = None
        d["new_of"] = new_of
        return d


def _unit(q):
    q = np.asarray(q, np.float64)
    return (q / np.linalg.norm(q, axis=-1, keepdims=True)).astype(np.float32)


def _affine(rng, spread=1.0):
    m = np.eye(4)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    m[:3, :3] = q * rng.uniform(0.7, 1.4)
    m[:3, 3] = rng.uniform(-spread, spread, 3)
    return m.astype(np.float32).reshape(16)


def _rot_keys(rng, n, wide_from=None):
    """n unit quaternions (w x y z): neighbours 2 - 6 degrees apart (slerp's lerp branch, cosTheta > 0.99), from key `wide_from` on 25 - 80 degrees apart (the
    trigonometric branch); every other step flips the sign, which slerp undoes"""
    q = [_unit(rng.normal(size=4))]
    for i in range(1, n):
        wide = wide_from is not None and i >= wide_from
        ang = np.radians(rng.uniform(25, 80) if wide else rng.uniform(2, 6)) / 2
        ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
        d = np.concatenate([[np.cos(ang)], np.sin(ang) * ax])
        a = q[-1].astype(np.float64)
        w = np.array([a[0] * d[0] - a[1:] @ d[1:], *(a[0] * d[1:] + d[0] * a[1:] + np.cross(a[1:], d[1:]))])
        q.append(_unit(w) * np.float32(-1 if i % 2 else 1))
    return np.stack(q)


def _times(rng, n, t0=0.0, dur=None):
    dur = dur if dur is not None else rng.uniform(1.5, 3.0)
    t = np.sort(rng.uniform(t0, dur, n)); t[0] = t0; t[-1] = dur
    return t.astype(np.float32)


WIDE_FROM_TIME = 1.0   # every rotation sampler of the synthetic graph is on the lerp branch before this time: frames that end before it are exact end to end


def synthetic(seed=20251019):
    """The seeded synthetic graph (see the module docstring of tests/test_scenegraph_host.py for what it covers).  Returns (Builder, notes)."""
    rng = np.random.default_rng(seed)
    b = Builder()
    notes = {}

    def lin3(node, target, anim=0, t0=0.0, keys=None):
        n = keys or int(rng.integers(3, 9))
        v = rng.uniform(0.5, 1.5, (n, 3)) if target == 2 else rng.uniform(-1, 1, (n, 3))
        b.channel(anim, b.sampler(LINEAR, VEC3, _times(rng, n, t0), v), node, target)

    def linq(node, anim=0, wide=False):
        n = int(rng.integers(4, 10))
        t = _times(rng, n)
        wide_from = int(np.searchsorted(t, WIDE_FROM_TIME) + 1) if wide else None
        b.channel(anim, b.sampler(LINEAR, QUAT, t, _rot_keys(rng, n, wide_from)), node, 1)

    # root A: a chain 33 deep with T, R, S channels on every link, and a fan of 65 mesh nodes under link 5
    special = {3: np.diag([1.5, 0.5, 2.0, 1.0]).astype(np.float32).reshape(16)}                                   # a non-uniform scale
    m = np.eye(4, dtype=np.float32); m[3] = [0.05, -0.02, 0.03, 1.1]; special[7] = m.reshape(16)                 # a projective last row
    m = np.eye(4, dtype=np.float32); m[0, 1] = -0.0; m[1, 2] = -0.0; m[2, 3] = -0.0; special[11] = m.reshape(16)  # minus zeros
    chain, p = [], -1
    for i in range(33):
        p = b.node(p, t=rng.uniform(-0.2, 0.2, 3), r=_unit(rng.normal(size=4)), matrix=special.get(i, IDENT), local=_affine(rng, 0.2))
        chain.append(p)
        if i == 5:
            fan = [b.node(p, local=_affine(rng), matrix=IDENT) for _ in range(65)]
    for i, n in enumerate(chain):
        lin3(n, 0); linq(n, wide=(i % 4 == 0)); lin3(n, 2)
    for n in fan:
        lin3(n, 0)
        b.instance(n)
    notes["chain"], notes["fan"] = chain, fan
    # root B: a skinned mesh node BEFORE its 24-joint skeleton (every pair stale), and a 1-joint skin whose joint is its own child (fresh)
    rb = b.node(-1, local=_affine(rng))
    m1 = b.node(rb, local=_affine(rng))
    one = b.node(rb, local=_affine(rng))
    one_joint = b.node(one, local=_affine(rng))
    lin3(one_joint, 0)
    skel1, p = [], rb
    for i in range(24):
        p = b.node(p if i % 3 else rb, t=rng.uniform(-0.3, 0.3, 3), r=_unit(rng.normal(size=4)), local=_affine(rng, 0.3))
        skel1.append(p)
        linq(p, wide=(i % 5 == 0)); lin3(p, 0)
    b.skin(m1, skel1, [_affine(rng) for _ in skel1])
    b.skin(one, [one_joint], [_affine(rng)])
    b.instance(m1); b.instance(one)
    # root C: a 65-joint skeleton, then the mesh node that uses it (every pair fresh), which also names root B's first joint (stale: never — it was visited)
    rc = b.node(-1, local=_affine(rng))
    skel2 = []
    for i in range(65):
        p = b.node(rc if i < 5 else skel2[(i - 5) // 4], r=_unit(rng.normal(size=4)), local=_affine(rng, 0.3))
        skel2.append(p)
        linq(p)
    m2 = b.node(rc, local=_affine(rng))
    b.skin(m2, skel2, [_affine(rng) for _ in skel2])
    b.instance(m2)
    # a mesh node with a skin of two joints, one visited before it and one after: a fresh and a stale pair in one skin use
    m3 = b.node(rc, local=_affine(rng))
    late = b.node(rc, local=_affine(rng))
    lin3(late, 0)
    b.skin(m3, [skel2[0], late], [_affine(rng), _affine(rng)])
    # morph nodes: W1 with 3 weights (LINEAR in animation 0, SPLINE in animation 1: the later wins), W2 with 2 (STEP)
    w1 = b.node(rc, local=_affine(rng), n_weights=3, weights=[0.1, 0.2, 0.3])
    w2 = b.node(rc, local=_affine(rng), n_weights=2)
    b.instance(w1)
    nk = 5
    b.channel(0, b.sampler(LINEAR, FLOAT, _times(rng, nk), rng.uniform(0, 1, nk * 3)), w1, 3)
    b.channel(1, b.sampler(SPLINE, FLOAT, _times(rng, nk), rng.uniform(-1, 1, nk * 3 * 3)), w1, 3)
    b.channel(1, b.sampler(STEP, FLOAT, _times(rng, nk), rng.uniform(0, 1, nk * 2)), w2, 3)
    w3 = b.node(rc, local=_affine(rng), n_weights=4, weights=[0.5, 0.25, 0.125, 1.0])
    b.channel(0, b.sampler(LINEAR, FLOAT, _times(rng, nk), rng.uniform(0, 1, nk * 4)), w3, 3)   # (a LINEAR weights channel nothing shadows)
    w4 = b.node(rc, local=_affine(rng), n_weights=2, weights=[0.75, 0.5])
    w5 = b.node(rc, local=_affine(rng), n_weights=3, weights=[0.1, 0.2, 0.3])
    b.channel(1, b.sampler(LINEAR, FLOAT, [0.6], [0.375]), w4, 3)                                  # one key: every weight becomes floatKey[0]
    b.channel(1, b.sampler(STEP, FLOAT, [0.0, 0.0], rng.uniform(0, 1, 6)), w5, 3)                  # duration 0: likewise
    notes["w1"], notes["w2"], notes["w3"] = w1, w2, w3
    # animation 1, the special samplers, on nodes of their own under root C
    sp = [b.node(rc, t=rng.uniform(-1, 1, 3), r=_unit(rng.normal(size=4)), s=rng.uniform(0.5, 1.5, 3), local=_affine(rng)) for _ in range(8)]
    n = 5
    b.channel(1, b.sampler(SPLINE, VEC3, _times(rng, n), rng.uniform(-1, 1, (n * 3, 3))), sp[0], 0)
    b.channel(1, b.sampler(SPLINE, QUAT, _times(rng, n), rng.uniform(-1, 1, (n * 3, 4))), sp[0], 1)
    b.channel(1, b.sampler(STEP, VEC3, _times(rng, n), rng.uniform(0.5, 1.5, (n, 3))), sp[1], 2)
    b.channel(1, b.sampler(STEP, QUAT, _times(rng, n), _rot_keys(rng, n)), sp[1], 1)
    b.channel(1, b.sampler(LINEAR, VEC3, [0.7], rng.uniform(-1, 1, 3)), sp[2], 0)                                   # one key
    b.channel(1, b.sampler(LINEAR, QUAT, [0.0, 0.0], _rot_keys(rng, 2)), sp[2], 1)                                  # duration 0
    b.channel(1, b.sampler(LINEAR, VEC3, _times(rng, n, t0=0.4), rng.uniform(-1, 1, (n, 3))), sp[3], 0)             # t[0] > 0: returns key 0 before it
    b.channel(1, b.sampler(SPLINE, VEC3, _times(rng, n, t0=0.4), rng.uniform(0.5, 1.5, (n * 3, 3))), sp[3], 2)      # ... key 1 for a spline
    b.channel(1, b.sampler(SPLINE, QUAT, _times(rng, n, t0=0.3), rng.uniform(-1, 1, (n * 3, 4))), sp[4], 1)
    b.channel(1, b.sampler(LINEAR, QUAT, _times(rng, n, t0=0.3), _rot_keys(rng, n)), sp[5], 1)
    # two animations writing the same field of one node: the chain's link 2 translation (animation 0 above) again in animation 1, and twice within animation 1
    lin3(chain[2], 0, anim=1)
    lin3(sp[6], 0, anim=1); lin3(sp[6], 0, anim=1)
    for x in sp:
        b.instance(x)
    notes["special"] = sp
    return b, notes


def small(n_nodes, seed):
    """a random tree of n_nodes, a T and an R channel on every node, every node an instance, one skin over all of them used by node 0"""
    rng = np.random.default_rng(seed)
    b = Builder()
    ids = []
    for i in range(n_nodes):
        ids.append(b.node(-1 if i == 0 else ids[int(rng.integers(0, i))], t=rng.uniform(-1, 1, 3), r=_unit(rng.normal(size=4)), local=_affine(rng)))
    for n in ids:
        k = int(rng.integers(2, 6))
        b.channel(0, b.sampler(LINEAR, VEC3, _times(rng, k), rng.uniform(-1, 1, (k, 3))), n, 0)
        b.channel(0, b.sampler(LINEAR, QUAT, _times(rng, k), _rot_keys(rng, k)), n, 1)
        b.instance(n)
    b.skin(ids[0], ids, [_affine(rng) for _ in ids])
    return b


def ops_synthetic(notes=None):
    """the scripted sequence: frames before WIDE_FROM_TIME (all rotations on the lerp branch), frames after it, a negative step, a wrap past every duration, a
    SetTime, a Reset, single-animation steps with a separate walk, a local transform set by hand"""
    m = (np.eye(4, dtype=np.float32) * np.float32(1.25)); m[0, 3] = 0.5; m[3, 3] = 1
    return [("advance", 0.0), ("advance", 0.125), ("advance", 0.25), ("advance", 0.3), ("advance", 0.5), ("advance", -0.2), ("advance", 0.75), ("advance", 2.9),
            ("set_time", 0, 0.55), ("advance", 0.05), ("reset", 1), ("advance_animation", 1, 0.2), ("update_nodes",), ("set_local", 0, m.reshape(16)),
            ("advance_animation", 0, 0.1), ("advance_animation", 1, 0.1), ("update_nodes",), ("advance", 0.015625)]


def run_ops(g, ops, download=None):
    """apply ops to a graph (device, host twin or reference: the same method names); after every op that walks the nodes, one snapshot of every array"""
    frames = []
    for op in ops:
        if op[0] == "advance": g.Advance(op[1])
        elif op[0] == "advance_animation": g.AdvanceAnimation(op[1], op[2])
        elif op[0] == "update_nodes": g.UpdateNodes()
        elif op[0] == "set_time": g.SetTime(op[1], op[2])
        elif op[0] == "reset": g.Reset(op[1])
        elif op[0] == "set_local": g.SetLocal(op[1], op[2])
        if op[0] in ("advance", "update_nodes"):
            frames.append({k: g.Download(w) for k, w in WHATS.items()})
            if download:
                for k, w in download.items():
                    frames[-1][k] = g.Download(w)
    return frames


def same_bits(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- the real reference --------------------------------------------------------------------------------------------------------------------
class RefGraph:
    """the shim's one graph, with the method names of tinybvh_amd.SceneGraph"""

    def __init__(self, lib, desc):
        import tinybvh_amd as tb
        self.lib = lib
        st, keep = tb.scenegraph_desc(desc)
        self._keep = keep
        n = lambda k: keep[k].size if k in keep else 0
        self.shape = {TRS: (n("parent"), 10), LOCAL: (n("parent"), 16), COMBINED: (n("parent"), 16), CHANNEL_T: (n("channel_node"),), CHANNEL_K: (n("channel_node"),),
                      INSTANCES: (n("node_of_instance"), 16), JOINTS: (int(keep["skin_joint_offset"][-1]) if n("skin_mesh_node") else 0, 16),
                      WEIGHTS: (int(keep["n_weights"].sum()) if "n_weights" in keep else 0,)}
        assert lib.sgref_create(C.byref(st)) == 0

    def Advance(self, dt): self.lib.sgref_advance(C.c_float(dt))
    def AdvanceAnimation(self, a, dt): self.lib.sgref_advance_animation(C.c_uint32(a), C.c_float(dt))
    def UpdateNodes(self): self.lib.sgref_update_nodes()
    def SetTime(self, a, t): self.lib.sgref_set_time(C.c_uint32(a), C.c_float(t))
    def Reset(self, a): self.lib.sgref_reset(C.c_uint32(a))

    def SetLocal(self, node, m):
        m = np.ascontiguousarray(m, np.float32)
        self.lib.sgref_set_local(C.c_uint32(node), C.c_void_p(m.ctypes.data))

    def Download(self, what):
        out = np.zeros(self.shape[what], np.int32 if what == CHANNEL_K else np.float32)
        buf = out if out.size else np.zeros(1, out.dtype)
        assert self.lib.sgref_download(C.c_int(what), C.c_void_p(buf.ctypes.data)) == 0
        return out


def compile_ref_shim(d):
    """the real tiny_scene.h with oracle/Makefile's flags (and its private members open to the shim); None when the reference is absent"""
    so = nb.compile_ref_shim(d, "scenegraph_ref_shim.cpp", extra=("-fno-access-control", "-I" + os.path.join(ROOT, "include")), scene_header=True,
                             need=("tiny_bvh.h", "tiny_scene.h"))
    if so is None:
        return None
    lib = C.CDLL(so)
    for name in ("sgref_local_from_trs", "sgref_advance", "sgref_advance_animation", "sgref_update_nodes", "sgref_set_time", "sgref_reset", "sgref_set_local", "sgref_mul", "sgref_invert", "sgref_slerp"):
        getattr(lib, name).restype = None
    return lib


# ---- a glTF file's animation tables (json + numpy; no glTF library) -------------------------------------------------------------------------
def gltf_desc(gltf_path, ref):
    """the descriptor of a .gltf + .bin scene as the reference's loader sets its nodes up (Node::ConvertFromGLTFNode: T, R, S, matrix, and localTransform =
    T * R * S * matrix for a node that gives any of them — computed by the reference itself through `ref`), every animation's samplers and channels, the mesh
    nodes as instances in depth-first visit order.  Skins are not read (the drone scene has none)."""
    import json
    with open(gltf_path) as f:
        g = json.load(f)
    base = os.path.dirname(gltf_path)
    bufs = [np.fromfile(os.path.join(base, b["uri"]), np.uint8) for b in g["buffers"]]

    def accessor(i):
        a = g["accessors"][i]; v = g["bufferViews"][a["bufferView"]]
        n = {"SCALAR": 1, "VEC3": 3, "VEC4": 4}[a["type"]]
        assert a["componentType"] == 5126 and v.get("byteStride", 4 * n) == 4 * n, "float accessors, tightly packed"
        o = v.get("byteOffset", 0) + a.get("byteOffset", 0)
        return bufs[v["buffer"]][o:o + a["count"] * n * 4].view(np.float32).reshape(a["count"], n).copy()

    b = Builder()
    nodes = g["nodes"]
    ids = {}

    def add(i, parent):
        n = nodes[i]
        t = n.get("translation", (0, 0, 0)); r = n.get("rotation", (0, 0, 0, 1)); s = n.get("scale", (1, 1, 1))
        m = np.float32(n["matrix"]).reshape(4, 4).T.reshape(16) if "matrix" in n else IDENT
        trs = np.float32([*t, r[3], r[0], r[1], r[2], *s])
        local = IDENT.copy()
        if any(k in n for k in ("translation", "rotation", "scale", "matrix")):
            m = np.ascontiguousarray(m, np.float32)
            ref.sgref_local_from_trs(C.c_void_p(trs.ctypes.data), C.c_void_p(m.ctypes.data), C.c_void_p(local.ctypes.data))
        nw = 0
        if "mesh" in n:
            nw = len(g["meshes"][n["mesh"]]["primitives"][0].get("targets", []))
        ids[i] = b.node(parent, t=trs[0:3], r=trs[3:7], s=trs[7:10], matrix=m, local=local, n_weights=nw)
        if "mesh" in n:
            b.instance(ids[i])
        for c in n.get("children", []):
            add(c, ids[i])

    for root in g["scenes"][g.get("scene", 0)]["nodes"]:
        add(root, -1)
    interp = {"LINEAR": LINEAR, "CUBICSPLINE": SPLINE, "STEP": STEP}
    target = {"translation": 0, "rotation": 1, "scale": 2, "weights": 3}
    for a, anim in enumerate(g.get("animations", [])):
        made = {}
        for ch in anim["channels"]:
            tg = target[ch["target"]["path"]]
            key = (ch["sampler"], tg)
            if key not in made:
                sm = anim["samplers"][ch["sampler"]]
                v = accessor(sm["output"])
                if tg == 1:   # (the loader zeroes subnormal quaternion components, and stores w first)
                    v = np.where(np.abs(v) < np.finfo(np.float32).tiny, np.float32(0), v)[:, [3, 0, 1, 2]]
                made[key] = b.sampler(interp[sm.get("interpolation", "LINEAR")], QUAT if tg == 1 else FLOAT if tg == 3 else VEC3, accessor(sm["input"]), v)
            b.channel(a, made[key], ids[ch["target"]["node"]], tg)
    return b


def ops_drone(exact_times, trig_times, duration):
    """frames at the given animation times, in order; then a step past the duration (a wrap) that lands on the first exact time again; then a SetTime"""
    times = sorted(list(exact_times) + list(trig_times))
    ops, t = [], 0.0
    for x in times:
        ops.append(("advance", float(np.float32(x) - np.float32(t)))); t = x
    ops.append(("advance", float(np.float32(duration) - np.float32(t) + np.float32(times[0]))))
    ops += [("set_time", 0, float(exact_times[-1])), ("advance", 0.0)]
    return ops


# ---- goldens -------------------------------------------------------------------------------------------------------------------------------
DESC_KEYS = ("parent", "visit_order", "translation", "rotation", "scale", "matrix", "local_transform", "n_weights", "weights", "sampler_interpolation", "sampler_type",
             "sampler_key_offset", "sampler_value_offset", "key_times", "key_values", "channel_animation", "channel_sampler", "channel_node", "channel_target",
             "node_of_instance", "skin_mesh_node", "skin_joint_offset", "skin_joint_node", "skin_inverse_bind")


def golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def golden_desc(g):
    d = {k: g["desc_" + k] for k in DESC_KEYS if "desc_" + k in g.files}
    d["n_animations"] = int(g["n_animations"]); d["flags"] = 0
    return d


def golden_frames(g):
    return [{k: g[k][f] for k in list(WHATS) + ["trig"]} for f in range(g["t"].shape[0])]


# ---- the tolerance of slerp's trigonometric branch (DESIGN.md par. 17) -------------------------------------------------------------------------
TRIG_U = 2   # ulps: neither the HIP math API table nor OCML's documentation is installed with the toolchain, so the issue's fallback holds (an assumption)
TRIG_U_SOURCE = "assumed: no HIP math API accuracy table or OCML documentation is installed; 2 ulp for acosf and sinf"


def compile_oracle(d):
    lib = C.CDLL(nb.compile_c_oracle(d, "oracle_scenegraph", extra=("-std=c11", "-I" + os.path.join(ROOT, "include"))))
    lib.sgorc_slerp.restype = C.c_int
    lib.sgorc_slerp_spread.restype = C.c_float
    lib.sgorc_create.restype = C.c_void_p
    for name in ("sgorc_free", "sgorc_advance", "sgorc_advance_animation", "sgorc_update_nodes", "sgorc_set_time", "sgorc_reset", "sgorc_set_local", "sgorc_set_trs"):
        getattr(lib, name).restype = None
    return lib


class OracleGraph:
    """the plain-C restatement (tests/oracle_scenegraph.c) with the method names of tinybvh_amd.SceneGraph.  The descriptor must be one the library accepts."""

    def __init__(self, lib, desc):
        import tinybvh_amd as tb
        self.lib = lib
        st, keep = tb.scenegraph_desc(desc)
        n = lambda k: keep[k].size if k in keep else 0
        self.shape = {TRS: (n("parent"), 10), LOCAL: (n("parent"), 16), COMBINED: (n("parent"), 16), CHANNEL_T: (n("channel_node"),), CHANNEL_K: (n("channel_node"),),
                      INSTANCES: (n("node_of_instance"), 16), JOINTS: (int(keep["skin_joint_offset"][-1]) if n("skin_mesh_node") else 0, 16),
                      WEIGHTS: (int(keep["n_weights"].sum()) if "n_weights" in keep else 0,)}
        self._h = C.c_void_p(lib.sgorc_create(C.byref(st)))

    def Advance(self, dt): self.lib.sgorc_advance(self._h, C.c_float(dt)); return self
    def AdvanceAnimation(self, a, dt): self.lib.sgorc_advance_animation(self._h, C.c_uint32(a), C.c_float(dt)); return self
    def UpdateNodes(self): self.lib.sgorc_update_nodes(self._h); return self
    def SetTime(self, a, t): self.lib.sgorc_set_time(self._h, C.c_uint32(a), C.c_float(t)); return self
    def Reset(self, a): self.lib.sgorc_reset(self._h, C.c_uint32(a)); return self

    def SetLocal(self, node, m):
        m = np.ascontiguousarray(m, np.float32)
        self.lib.sgorc_set_local(self._h, C.c_uint32(node), C.c_void_p(m.ctypes.data)); return self

    def SetTRS(self, trs):
        a = np.ascontiguousarray(trs, np.float32)
        self.lib.sgorc_set_trs(self._h, C.c_void_p(a.ctypes.data)); return self

    def Download(self, what):
        out = np.zeros(self.shape[what], np.int32 if what == CHANNEL_K else np.float32)
        buf = out if out.size else np.zeros(1, out.dtype)
        assert self.lib.sgorc_download(self._h, C.c_int(what), C.c_void_p(buf.ctypes.data)) == 0
        return out

    def free(self):
        if self._h:
            self.lib.sgorc_free(self._h)
        self._h = None


def trig_intervals(desc):
    """(a, b) key pairs of every interval of a LINEAR quaternion sampler that a rotation channel uses and that slerp sends down the trigonometric branch"""
    out = []
    used = set(int(s) for s, t in zip(desc["channel_sampler"], desc["channel_target"]) if t == 1)
    for s in sorted(used):
        if desc["sampler_interpolation"][s] != LINEAR:
            continue
        v = desc["key_values"][desc["sampler_value_offset"][s]:desc["sampler_value_offset"][s + 1]].reshape(-1, 4)
        n = desc["sampler_key_offset"][s + 1] - desc["sampler_key_offset"][s]
        for k in range(int(n) - 1):
            c = abs(float(np.dot(v[k].astype(np.float64), v[k + 1].astype(np.float64))))
            if c <= 0.9901:   # (a generous pre-filter; the oracle's own branch decides below)
                out.append((v[k].copy(), v[k + 1].copy()))
    return out


def trig_bound(ref, orc, descs, u=TRIG_U):
    """D: over every trigonometric-branch interval of the descriptors at 16 values of f, the largest component deviation of the restated branch with its
    four libm results moved by -u, 0, +u ulp (all 81 combinations) from the REAL reference's normalised quaternion.  Returns (D, intervals counted)."""
    worst, n = 0.0, 0
    zero = (C.c_int * 4)(0, 0, 0, 0)
    q = np.zeros(4, np.float32); want = np.zeros(4, np.float32)
    for desc in descs:
        for a, b in trig_intervals(desc):
            took = False
            for i in range(16):
                f = C.c_float((i + 0.5) / 16)
                if not orc.sgorc_slerp(C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data), f, zero, C.c_void_p(q.ctypes.data)):
                    continue
                took = True
                ref.sgref_slerp(C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data), f, C.c_void_p(want.ctypes.data))
                worst = max(worst, float(orc.sgorc_slerp_spread(C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data), f, C.c_int(u), C.c_void_p(want.ctypes.data))))
            n += took
    return worst, n


DRONE_DURATION = 25.0


def drone_path():
    return os.path.join(nb.reference_dir(), "testdata", "drone", "scene.gltf")


def search_frames(d, candidates):
    """(times at which no channel is on slerp's trigonometric branch, times at which a rotation channel is), by the host twin's own flags"""
    import tinybvh_amd as tb
    host = tb.HostSceneGraph(d)
    rot = d["channel_target"] == 1
    exact, inexact = [], []
    for t in candidates:
        for a in range(d["n_animations"]):
            host.SetTime(a, float(t))
        trig = host.Advance(0.0).Download(TRIG)
        (inexact if (trig.astype(bool) & rot).any() else exact).append(float(t))
    return exact, inexact


def _golden_arrays(ref, d, ops, bound):
    import tinybvh_amd as tb
    frames = run_ops(RefGraph(ref, d), ops)
    host = tb.HostSceneGraph(d)
    hframes = run_ops(host, ops, {"trig": TRIG})
    rot = d["channel_target"] == 1
    trig = np.stack([f["trig"] for f in hframes])
    exact = [i for i in range(len(frames)) if not trig[i].any()]
    inexact = [i for i in range(len(frames)) if (trig[i].astype(bool) & rot).any()]
    out = {"desc_" + k: d[k] for k in DESC_KEYS if d[k] is not None}
    out.update(n_animations=np.int64(d["n_animations"]), stale=host.Download(STALE), trig=trig, exact_frames=np.array(exact), trig_frames=np.array(inexact),
               trig_bound=np.array(bound[:3]), trig_intervals=np.int64(bound[3]), trig_u_source=np.array(TRIG_U_SOURCE))
    for k in WHATS:
        out[k] = np.stack([f[k] for f in frames])
    return out


def make_golden(ref, orc, out_dir=GOLDEN):
    """synthetic.npz and drone.npz: a descriptor, the REAL reference's arrays after every walk of the scripted sequence, the host twin's trig flags and stale pairs,
    and the slerp tolerance (derived over BOTH descriptors).  Asserts the properties the tests rely on.  drone.npz: the animation tables of the reference's
    testdata/drone/scene.gltf + scene.bin (data its programs read), frames found by search: at least 4 all on the lerp branch, at least 2 with the other."""
    os.makedirs(out_dir, exist_ok=True)
    b, notes = synthetic()
    d = b.desc(shuffle_seed=5)
    drone = gltf_desc(drone_path(), ref).desc()
    D, n = trig_bound(ref, orc, [d, drone])
    assert n > 0 and D > 0
    bound = (TRIG_U, D, 2 * D, n)
    out = _golden_arrays(ref, d, ops_synthetic(), bound)
    assert out["stale"].any() and not out["stale"].all(), "the synthetic graph needs a stale and a fresh joint pair"
    assert len(out["exact_frames"]) >= 4 and len(out["trig_frames"]) >= 2, (out["exact_frames"], out["trig_frames"])
    np.savez_compressed(os.path.join(out_dir, "synthetic.npz"), **out)
    exact, inexact = search_frames(drone, np.arange(0.5, DRONE_DURATION - 1, 0.7312))
    assert len(exact) >= 4 and len(inexact) >= 2, (len(exact), len(inexact))
    pick = lambda v, k: [v[i * (len(v) - 1) // (k - 1)] for i in range(k)]
    ops = ops_drone(pick(exact, 4), pick(inexact, 2), DRONE_DURATION)
    dout = _golden_arrays(ref, drone, ops, bound)
    dout["ops_dt"] = np.array([op[1] if op[0] == "advance" else op[2] for op in ops], np.float64)     # (the sequence itself: the searched times are data)
    dout["ops_kind"] = np.array([0 if op[0] == "advance" else 1 for op in ops])
    assert len(dout["exact_frames"]) >= 4 and len(dout["trig_frames"]) >= 2, (dout["exact_frames"], dout["trig_frames"])
    np.savez_compressed(os.path.join(out_dir, "drone.npz"), **dout)
    return out, dout


def golden_ops(g):
    """the scripted sequence a golden was made with"""
    if "ops_dt" not in g.files:
        return ops_synthetic()
    return [("advance", float(x)) if k == 0 else ("set_time", 0, float(x)) for x, k in zip(g["ops_dt"], g["ops_kind"])]
