"""Shared pieces of the tests of BVH_Double scenes that move (test_double_anim_host.py, test_double_anim_gpu.py): the device TLAS builder
restated in numpy (63-bit Morton keys, stable sort, Karras topology, the library's node numbering), a validity check of such a tree, the
bottom-up recomputation of a BLAS's boxes, and the scene / ray batch the query tests share."""
import numpy as np

import tinybvh_amd as tb
from double_lib import instance_scene, random_rays_dbl

# the TLAS query tests' scene and batch: instance_scene(500) and the rays of test_double_gpu.test_tlas_instances.  test_double_anim_host checks on
# the CPU that the host-built tree and a Karras tree over the same records give the oracle the same records for this choice (at most TREE_SHAPE_CAP
# differ: 1e-4 of the batch, the bound the project uses for fp32-against-fp64 agreement).
SCENE_SEED = 3
RAY_SEED = 21
N_INST = 500
N_RAYS = 32768
TREE_SHAPE_CAP = 3
CENTRE = np.array([1.0e6, -2.0e6, 3.0e6])


def tlas_scene():
    return instance_scene(N_INST, seed=SCENE_SEED)


def tlas_rays(n: int = N_RAYS, seed: int = RAY_SEED) -> np.ndarray:
    rays = random_rays_dbl(n, CENTRE - 80, CENTRE + 80, seed=seed)
    rays["mask"][::2] = 0x1   # half of the rays skip the instances with mask 0x2
    rays["instIdx"] = 7
    return rays


def bounds_of(blas_verts) -> np.ndarray:
    return np.stack([np.concatenate([v.min(0), v.max(0)]) for v in blas_verts])


def _spread21(v: np.ndarray) -> np.ndarray:
    v = v.astype(np.uint64) & np.uint64(0x1fffff)
    for shift, mask in ((32, 0x001f00000000ffff), (16, 0x001f0000ff0000ff), (8, 0x100f00f00f00f00f), (4, 0x10c30c30c30c30c3), (2, 0x1249249249249249)):
        v = (v | (v << np.uint64(shift))) & np.uint64(mask)
    return v


def morton63(lo: np.ndarray, hi: np.ndarray) -> np.ndarray:
    """21 bits per axis of the box centres relative to the centre bounds, in double (kernels_double_anim.hip: k_morton_dbl)."""
    c = 0.5 * lo + 0.5 * hi
    cl, ch = c.min(0), c.max(0)
    ext = ch - cl
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(ext > 0, (c - cl) / ext, 0.0)
    u = np.where(u > 0, np.where(u < 1, u, 1.0), 0.0)
    q = np.minimum((u * 2097151.0).astype(np.uint64), np.uint64(2097151))
    return (_spread21(q[:, 0]) << np.uint64(2)) | (_spread21(q[:, 1]) << np.uint64(1)) | _spread21(q[:, 2])


def _clz64(x: int) -> int:
    return 64 - int(x).bit_length()


def karras_tlas(inst: np.ndarray):
    """(nodes, idx) over the instance boxes exactly as the device builds them: root 0, the children of Karras interior node i at 1 + 2 i and
    2 + 2 i, one instance per leaf, every interior box the union of its children's."""
    n = inst.shape[0]
    lo, hi = inst["aabbMin"], inst["aabbMax"]
    nodes = np.zeros(2 * n - 1, tb.NODE_DBL_DTYPE)
    keys = morton63(lo, hi)
    order = np.argsort(keys, kind="stable")
    k = [int(x) for x in keys[order]]
    idx = order.astype(np.uint64)

    def leaf(slot, j):
        nodes[slot]["aabbMin"], nodes[slot]["aabbMax"], nodes[slot]["leftFirst"], nodes[slot]["triCount"] = lo[order[j]], hi[order[j]], j, 1

    if n == 1:
        leaf(0, 0)
        return nodes, idx

    def delta(i, j):
        if j < 0 or j >= n:
            return -1
        return 64 + (32 - (i ^ j).bit_length()) if k[i] == k[j] else _clz64(k[i] ^ k[j])

    slot_of = {0: 0}          # Karras interior node -> slot
    children = {}
    for i in range(n - 1):
        d = 1 if delta(i, i + 1) - delta(i, i - 1) >= 0 else -1
        dmin = delta(i, i - d)
        lmax = 2
        while delta(i, i + lmax * d) > dmin:
            lmax <<= 1
        l, t = 0, lmax >> 1
        while t >= 1:
            if delta(i, i + (l + t) * d) > dmin:
                l += t
            t >>= 1
        j = i + l * d
        dnode = delta(i, j)
        s, t = 0, (l + 1) >> 1
        while True:
            if delta(i, i + (s + t) * d) > dnode:
                s += t
            if t <= 1:
                break
            t = (t + 1) >> 1
        gamma = i + s * d + min(d, 0)
        a, b = min(i, j), max(i, j)
        children[i] = (("leaf", gamma) if a == gamma else ("node", gamma), ("leaf", gamma + 1) if b == gamma + 1 else ("node", gamma + 1))
    # slots top-down, boxes bottom-up
    order_nodes, stack = [], [0]
    while stack:
        i = stack.pop()
        order_nodes.append(i)
        for c, (kind, g) in enumerate(children[i]):
            if kind == "leaf":
                leaf(1 + 2 * i + c, g)
            else:
                slot_of[g] = 1 + 2 * i + c
                stack.append(g)
    for i in reversed(order_nodes):
        s, c = slot_of[i], 1 + 2 * i
        nodes[s]["aabbMin"] = np.minimum(nodes[c]["aabbMin"], nodes[c + 1]["aabbMin"])
        nodes[s]["aabbMax"] = np.maximum(nodes[c]["aabbMax"], nodes[c + 1]["aabbMax"])
        nodes[s]["leftFirst"], nodes[s]["triCount"] = c, 0
    return nodes, idx


def check_tlas_tree(nodes: np.ndarray, idx: np.ndarray, inst: np.ndarray):
    """2 n - 1 nodes all reached from the root, every instance in exactly one leaf of one instance, leaf boxes the instance boxes, every
    interior box exactly the union of its children's."""
    n = inst.shape[0]
    assert nodes.shape[0] == 2 * n - 1 and idx.shape[0] == n
    assert np.array_equal(np.sort(idx), np.arange(n, dtype=np.uint64))
    seen = np.zeros(nodes.shape[0], bool)
    covered = np.zeros(n, np.int64)
    stack = [0]
    while stack:
        i = stack.pop()
        assert not seen[i], i
        seen[i] = True
        nd = nodes[i]
        if nd["triCount"] > 0:
            assert nd["triCount"] == 1, (i, nd["triCount"])
            k = int(nd["leftFirst"])
            covered[k] += 1
            assert np.array_equal(nd["aabbMin"], inst["aabbMin"][idx[k]]) and np.array_equal(nd["aabbMax"], inst["aabbMax"][idx[k]]), i
        else:
            c = int(nd["leftFirst"])
            assert 0 < c and c + 1 < nodes.shape[0], (i, c)
            assert np.array_equal(nd["aabbMin"], np.minimum(nodes[c]["aabbMin"], nodes[c + 1]["aabbMin"])), i
            assert np.array_equal(nd["aabbMax"], np.maximum(nodes[c]["aabbMax"], nodes[c + 1]["aabbMax"])), i
            stack += [c, c + 1]
    assert seen.all() and (covered == 1).all()


def refit_boxes(nodes: np.ndarray, prim_idx: np.ndarray, verts: np.ndarray) -> np.ndarray:
    """The node array with every box reachable from the root recomputed bottom-up from verts ((3 n, 3) float64): a leaf's from the vertices
    of its triangles, an interior node's the union of its children's.  leftFirst / triCount as given."""
    out = nodes.copy()
    tri = np.asarray(verts, np.float64).reshape(-1, 3, 3)
    tlo, thi = tri.min(1), tri.max(1)
    order, stack = [], [0]
    while stack:
        i = stack.pop()
        order.append(i)
        if out[i]["triCount"] == 0:
            stack += [int(out[i]["leftFirst"]), int(out[i]["leftFirst"]) + 1]
    for i in reversed(order):
        f, c = int(out[i]["leftFirst"]), int(out[i]["triCount"])
        if c:
            p = prim_idx[f:f + c].astype(np.int64)
            out[i]["aabbMin"], out[i]["aabbMax"] = tlo[p].min(0), thi[p].max(0)
        else:
            out[i]["aabbMin"] = np.minimum(out[f]["aabbMin"], out[f + 1]["aabbMin"])
            out[i]["aabbMax"] = np.maximum(out[f]["aabbMax"], out[f + 1]["aabbMax"])
    return out
