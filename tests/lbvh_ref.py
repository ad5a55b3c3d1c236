"""The device LBVH builders restated in numpy, once (tinybvh_amd/csrc/lbvh.h is the device's one copy): Morton keys from box centres, the
Karras 2012 range search, and the three ways the builders number the result.  The byte-exact tests of the fp64 TLAS (double_anim_lib.py),
the fp32 TLAS and the BVH2 builder (test_lbvh_gpu.py) all build their expected blobs from here."""
import numpy as np


def _spread(v, steps):
    v = v.astype(np.uint64)
    for shift, mask in steps:
        v = (v | (v << np.uint64(shift))) & np.uint64(mask)
    return v


def spread10(v: np.ndarray) -> np.ndarray:
    """10 bits -> every third bit of 30"""
    return _spread(v & np.uint64(0x3ff), ((16, 0xff0000ff), (8, 0x0f00f00f), (4, 0xc30c30c3), (2, 0x49249249)))


def spread21(v: np.ndarray) -> np.ndarray:
    """21 bits -> every third bit of 63"""
    return _spread(v & np.uint64(0x1fffff), ((32, 0x001f00000000ffff), (16, 0x001f0000ff0000ff), (8, 0x100f00f00f00f00f), (4, 0x10c30c30c30c30c3),
                                             (2, 0x1249249249249249)))


def quantise(c: np.ndarray, maxq: int) -> np.ndarray:
    """(n, 3) centres -> (n, 3) cells 0..maxq relative to the centres' own bounds, every operation in c's own precision (float32 or float64;
    maxq = 1023 and 2097151 are exact in both).  The two precisions clamp differently, as the kernels do: float32 keeps a NaN (the conversion
    then decides), float64 turns it into 0."""
    f = c.dtype.type
    cl, ch = c.min(0), c.max(0)
    ext = ch - cl
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(ext > 0, (c - cl) / ext, f(0))
    if c.dtype == np.float64:
        u = np.where(u > 0, np.where(u < 1, u, f(1)), f(0))
    else:
        u = np.where(u < 0, f(0), np.where(u > 1, f(1), u))
    assert u.dtype == c.dtype
    return np.minimum((u * f(maxq)).astype(np.uint64), np.uint64(maxq))


def morton30(c: np.ndarray) -> np.ndarray:
    q = quantise(c, 1023)
    return (spread10(q[:, 0]) << np.uint64(2)) | (spread10(q[:, 1]) << np.uint64(1)) | spread10(q[:, 2])


def morton63(c: np.ndarray) -> np.ndarray:
    q = quantise(c, 2097151)
    return (spread21(q[:, 0]) << np.uint64(2)) | (spread21(q[:, 1]) << np.uint64(1)) | spread21(q[:, 2])


def sort_keys(keys: np.ndarray):
    """(sorted keys as Python ints, order): the device's radix sort is stable"""
    order = np.argsort(keys, kind="stable")
    return [int(x) for x in keys[order]], order


def karras(k, key_bits: int):
    """Karras 2012 over the sorted keys k: per interior node i = 0 .. n - 2 (left, right, lo, hi) in Karras ids (interior node g -> g, leaf
    g -> n - 1 + g) with its sorted range [lo, hi].  Equal keys are told apart by their position: key_bits + clz32(i ^ j)."""
    n = len(k)

    def delta(i, j):
        if j < 0 or j >= n:
            return -1
        return key_bits + (32 - (i ^ j).bit_length()) if k[i] == k[j] else key_bits - (k[i] ^ k[j]).bit_length()

    out = []
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
        lo, hi = min(i, j), max(i, j)
        out.append((n - 1 + gamma if lo == gamma else gamma, n + gamma if hi == gamma + 1 else gamma + 1, lo, hi))
    return out


# the three numberings: where the two children of Karras interior node i go (id: the child's Karras id)
SCHEMES = {
    "pairs": lambda i, c, id: 1 + 2 * i + c,     # fp64 TLAS: 2 n - 1 nodes, no unused slot
    "bvh2": lambda i, c, id: 2 + 2 * i + c,      # BVH2: node 1 unused; ranges of at most max_leaf are one leaf
    "karras": lambda i, c, id: id,               # fp32 TLAS: the Karras ids themselves
}


def number(topo, n: int, scheme: str, max_leaf: int = 1):
    """The tree from the root down as [(slot, is_leaf, a, b)]: a leaf covers the sorted positions [a, a + b), an interior node has its
    children in slots a and b.  Every node comes before its children."""
    if n == 1:
        return [(0, True, 0, 1)]
    place = SCHEMES[scheme]
    out, stack = [], [(0, 0)]
    while stack:
        i, slot = stack.pop()
        left, right, lo, hi = topo[i]
        if scheme == "bvh2" and hi - lo + 1 <= max_leaf:
            out.append((slot, True, lo, hi - lo + 1))
            continue
        kids = [place(i, c, id) for c, id in enumerate((left, right))]
        out.append((slot, False, kids[0], kids[1]))
        for s, id in zip(kids, (left, right)):
            if id >= n - 1:
                out.append((s, True, id - (n - 1), 1))
            else:
                stack.append((id, s))
    return out


def boxes(tree, lo: np.ndarray, hi: np.ndarray, order: np.ndarray):
    """{slot: (min, max)}: a leaf's box is the union of its primitives' (lo, hi by primitive, order = the sorted positions' primitives), an
    interior node's the union of its children's (min and max are exact, so the order of the unions does not matter)."""
    b = {}
    for slot, is_leaf, a, c in reversed(tree):
        if is_leaf:
            p = order[a:a + c]
            b[slot] = (lo[p].min(0), hi[p].max(0))
        else:
            b[slot] = (np.minimum(b[a][0], b[c][0]), np.maximum(b[a][1], b[c][1]))
    return b


def build(keys: np.ndarray, key_bits: int, scheme: str, lo: np.ndarray, hi: np.ndarray, max_leaf: int = 1):
    """(tree, boxes, order) of the LBVH over primitives with these keys and boxes"""
    k, order = sort_keys(keys)
    tree = number(karras(k, key_bits), len(k), scheme, max_leaf)
    return tree, boxes(tree, lo, hi, order), order


def bvh2_nodes(c: np.ndarray, lo: np.ndarray, hi: np.ndarray, max_leaf: int):
    """kernels_build.hip's LBVH over float32 boxes with centres c: ({slot: the 8 words of its 32-byte BVHNode}, primIdx)"""
    tree, b, order = build(morton63(c), 64, "bvh2", lo, hi, max_leaf)
    out = {}
    for slot, is_leaf, a, cnt in tree:
        rec = np.zeros(8, np.uint32)
        rec[0:3] = b[slot][0].view(np.uint32); rec[4:7] = b[slot][1].view(np.uint32)
        rec[3], rec[7] = (a, cnt) if is_leaf else (a, 0)
        out[slot] = rec
    return out, order.astype(np.uint32)


def tlas_nodes(c: np.ndarray, lo: np.ndarray, hi: np.ndarray):
    """kernels_tlasbuild.hip's LBVH over float32 instance boxes: ((2 n - 1, 16) uint32 Aila-Laine records, the instance index list).  An
    interior record holds its children's boxes and Karras ids; a leaf record is zero but for triCount = 1 (word 11) and firstTri (word 15)."""
    n = c.shape[0]
    tree, b, order = build(morton30(c), 32, "karras", lo, hi)
    nodes = np.zeros((2 * n - 1, 16), np.uint32)
    for slot, is_leaf, a, cnt in tree:
        if is_leaf:
            nodes[slot, 11], nodes[slot, 15] = 1, a
        else:
            nodes[slot, 0:3] = b[a][0].view(np.uint32); nodes[slot, 4:7] = b[a][1].view(np.uint32)
            nodes[slot, 8:11] = b[cnt][0].view(np.uint32); nodes[slot, 12:15] = b[cnt][1].view(np.uint32)
            nodes[slot, 3], nodes[slot, 7] = a, cnt
    return nodes, order.astype(np.uint32)
