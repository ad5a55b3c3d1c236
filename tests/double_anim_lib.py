"""Shared pieces of the tests of BVH_Double scenes that move (test_double_anim_host.py, test_double_anim_gpu.py): the device TLAS builder
restated in numpy (lbvh_ref.py: 63-bit Morton keys, stable sort, Karras topology; here the fp64 node records), a validity check of such a tree, the
bottom-up recomputation of a BLAS's boxes, and the scene / ray batch the query tests share."""
import numpy as np

import lbvh_ref
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


def morton63(lo: np.ndarray, hi: np.ndarray) -> np.ndarray:
    """21 bits per axis of the box centres relative to the centre bounds, in double (kernels_double_anim.hip: k_morton_dbl)."""
    return lbvh_ref.morton63(0.5 * lo + 0.5 * hi)


def karras_tlas(inst: np.ndarray):
    """(nodes, idx) over the instance boxes exactly as the device builds them: root 0, the children of Karras interior node i at 1 + 2 i and
    2 + 2 i, one instance per leaf, every interior box the union of its children's."""
    lo, hi = inst["aabbMin"], inst["aabbMax"]
    tree, box, order = lbvh_ref.build(morton63(lo, hi), 64, "pairs", lo, hi)
    nodes = np.zeros(2 * inst.shape[0] - 1, tb.NODE_DBL_DTYPE)
    for slot, is_leaf, a, _ in tree:
        nodes[slot]["aabbMin"], nodes[slot]["aabbMax"] = box[slot]
        nodes[slot]["leftFirst"], nodes[slot]["triCount"] = a, 1 if is_leaf else 0
    return nodes, order.astype(np.uint64)


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
