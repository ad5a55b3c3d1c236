"""Shared pieces of the tests of sphere BLASes that move (device build, rebuild, refit: DESIGN.md par. 12): the numpy restatement of the refit
rule, the structure check of a downloaded Wald tree, and the sphere sets of the build test."""
import numpy as np

from custom_lib import sphere_set


def wald_refit(nodes, prim_idx, spheres):
    """(boxes (n_nodes, 6) float32, reached (n_nodes,) bool): every node the root reaches gets, children first, the box the refit rule gives
    it: a leaf the min of pos - r / the max of pos + r over its primIdx range (float32, one operation per component), an interior node the
    min / max of its two children.  Unreached nodes keep zeros."""
    nodes = np.ascontiguousarray(nodes).view(np.uint32).reshape(-1, 8)
    sph = np.ascontiguousarray(spheres, np.float32).reshape(-1, 4)
    lo, hi = sph[:, :3] - sph[:, 3:4], sph[:, :3] + sph[:, 3:4]
    assert lo.dtype == np.float32
    box = np.zeros((nodes.shape[0], 6), np.float32)
    reached = np.zeros(nodes.shape[0], bool)
    order, stack = [], [0]
    while stack:
        k = stack.pop()
        assert not reached[k], f"node {k} reached twice"
        reached[k] = True
        order.append(k)
        if nodes[k, 7] == 0:
            stack += [int(nodes[k, 3]), int(nodes[k, 3]) + 1]
    for k in reversed(order):   # a parent precedes its children in `order`
        first, count = int(nodes[k, 3]), int(nodes[k, 7])
        if count:
            p = prim_idx[first:first + count]
            box[k, :3], box[k, 3:] = lo[p].min(0), hi[p].max(0)
        else:
            box[k, :3] = np.minimum(box[first, :3], box[first + 1, :3])
            box[k, 3:] = np.maximum(box[first, 3:], box[first + 1, 3:])
    return box, reached


def node_boxes(nodes):
    f = np.ascontiguousarray(nodes).view(np.uint32).reshape(-1, 8).view(np.float32)
    return np.concatenate([f[:, 0:3], f[:, 4:7]], axis=1)


def check_boxes(nodes, prim_idx, spheres):
    """every reachable node's box equals the restatement, compared by value (-0 equals +0)"""
    want, reached = wald_refit(nodes, prim_idx, spheres)
    got = node_boxes(nodes)
    bad = np.nonzero(reached & (got != want).any(1))[0]
    assert bad.size == 0, (bad[:5], got[bad[:5]], want[bad[:5]])
    return reached


def check_structure(nodes, prim_idx, n, max_leaf, node1_unused=True):
    """a downloaded Wald tree over n spheres: child pairs inside the array, every reachable node reached once, node 1 unused when n > 1 (the
    device builders' numbering; the host builder hands node 1 out), the leaves tile primIdx exactly once, primIdx a permutation of range(n), no
    leaf above max_leaf"""
    nodes = np.ascontiguousarray(nodes).view(np.uint32).reshape(-1, 8)
    seen = np.zeros(nodes.shape[0], np.int64)
    cover = np.zeros(prim_idx.size, np.int64)
    stack = [0]
    while stack:
        k = stack.pop()
        seen[k] += 1
        assert seen[k] == 1, f"node {k} reached twice"
        first, count = int(nodes[k, 3]), int(nodes[k, 7])
        if count:
            assert count <= max_leaf, (k, count, max_leaf)
            assert first + count <= prim_idx.size, (k, first, count)
            cover[first:first + count] += 1
        else:
            assert first + 1 < nodes.shape[0], (k, first)
            stack += [first, first + 1]
    if n > 1 and node1_unused:
        assert seen[1] == 0, "node 1 is reached"
    assert (cover == 1).all(), "the leaves do not tile primIdx exactly once"
    assert prim_idx.size == n and np.array_equal(np.sort(prim_idx), np.arange(n, dtype=np.uint32)), "primIdx is not a permutation of range(n)"


def random_spheres(n):
    rng = np.random.default_rng(1000 + n)
    s = np.empty((n, 4), np.float32)
    s[:, :3] = rng.uniform(-5, 5, (n, 3))
    s[:, 3] = rng.uniform(0.1, 0.8, n)
    return s


BUILD_SETS = ["one", "rand2", "rand3", "rand63", "rand64", "rand65", "rand257", "centre65", "dups", "soup", "bunny16", "soup_badr"]


def build_set(name):
    """the sets of the build test: the odd sizes around a wave, 65 spheres at one centre (the centroid extent is 0 on every axis), exact
    duplicates (equal Morton keys), and the soup with its first eight radii set to 0 and the next eight negated"""
    if name.startswith("rand"):
        return random_spheres(int(name[4:]))
    if name == "centre65":
        s = np.empty((65, 4), np.float32)
        s[:, :3] = [1.5, -2.0, 0.25]
        s[:, 3] = np.arange(1, 66, dtype=np.float32) / np.float32(64)   # (dyadic: pos -/+ r and the centroids are exact)
        return s
    if name == "soup_badr":
        s = sphere_set("soup").copy()
        s[0:8, 3] = 0.0
        s[8:16, 3] = -s[8:16, 3]
        return s
    return sphere_set(name)
