"""The ray / triangle test in its two forms (tinybvh_amd/csrc/device_common.h; no GPU needed) through tbvh_debug_tri_test_flat: tri_test with its three early-outs,
as the per-lane kernels run it, and tri_test_flat, the branch-free form of the wave-packet kernel, which computes a, f, u, v, t unconditionally and forms one
predicate from the same comparisons with the same negations.  Both run on the host over the same pairs: accept / reject must be equal, and t, u, v the same
bits wherever a pair is accepted — also with a NaN or an infinity on the way (f = 1 / a behind an edge-on triangle, a NaN vertex), which must take the path it
takes in the branching form.

Pairs: the edge cases by construction (an edge-on triangle with |a| < 1e-6, rays through a vertex and along an edge with u = 0, v = 0 and u + v = 1 exactly, t equal
to the ray's tmax, t < 0, a NaN vertex, infinite and zero directions), then 10^6 seeded random pairs of several kinds (aimed into the triangle, aimed at its rim,
unrelated, tmax at and one ulp either side of the true t)."""
import ctypes as C

import numpy as np

import tinybvh_amd as tb
from tinybvh_amd import _capi


def both(O, D, v0, e1, e2, tmax):
    """-> accept_branch, accept_flat (uint8), tuv_branch, tuv_flat (n x 3 float32)"""
    n = len(tmax)
    od = np.ascontiguousarray(np.concatenate([np.asarray(O, np.float32).reshape(n, 3), np.asarray(D, np.float32).reshape(n, 3)], axis=1), np.float32)
    tri = np.ascontiguousarray(np.concatenate([np.asarray(x, np.float32).reshape(n, 3) for x in (v0, e1, e2)], axis=1), np.float32)
    tm = np.ascontiguousarray(tmax, np.float32)
    ab, af = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    tb_, tf = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    tb.check(_capi.lib.tbvh_debug_tri_test_flat(C.c_void_p(od.ctypes.data), C.c_void_p(tri.ctypes.data), C.c_void_p(tm.ctypes.data), n, C.c_void_p(ab.ctypes.data),
                                                C.c_void_p(af.ctypes.data), C.c_void_p(tb_.ctypes.data), C.c_void_p(tf.ctypes.data)), "tbvh_debug_tri_test_flat")
    return ab, af, tb_, tf


def agree(O, D, v0, e1, e2, tmax):
    ab, af, tb_, tf = both(O, D, v0, e1, e2, tmax)
    bad = np.flatnonzero(ab != af)
    assert bad.size == 0, ("accept differs", bad.size, int(bad[0]), int(ab[bad[0]]), int(af[bad[0]]), tf[bad[0]])
    acc = ab == 1
    bits = (tb_[acc].view(np.uint32) != tf[acc].view(np.uint32)).any(1)
    assert not bits.any(), ("t, u, v differ in bits", int(bits.sum()), tb_[acc][bits][:2], tf[acc][bits][:2])
    return ab, tf


F = np.float32


def one(O, D, v0, v1, v2, tmax=1e30):
    with np.errstate(all="ignore"):                 # (the non-finite cases overflow and subtract infinities on purpose)
        v0, v1, v2 = (np.asarray(x, np.float64).astype(np.float32) for x in (v0, v1, v2))
        a, tuv = agree([O], [D], [v0], [v1 - v0], [v2 - v0], [tmax])
    return bool(a[0]), tuv[0]


TRI = ((0.0, 0.0, 2.0), (1.0, 0.0, 2.0), (0.0, 1.0, 2.0))       # in the plane z = 2: u along x, v along y, exact in fp32


def test_plain_hit_and_miss():
    ok, (t, u, v) = one((0.25, 0.25, 0.0), (0.0, 0.0, 1.0), *TRI)
    assert ok and (t, u, v) == (F(2.0), F(0.25), F(0.25))
    assert not one((2.0, 2.0, 0.0), (0.0, 0.0, 1.0), *TRI)[0]


def test_edge_on_triangle_is_rejected_by_the_determinant():
    # the ray lies in the triangle's plane: a == 0 exactly, f = inf, u and v are inf or NaN
    assert not one((-1.0, 0.25, 2.0), (1.0, 0.0, 0.0), *TRI)[0]
    # nearly in the plane: 0 < |a| < 1e-6
    ok, _ = one((-1.0, 0.25, 2.0), (1.0, 0.0, 5e-7), *TRI)
    assert not ok
    # just past the threshold the determinant lets it through to the other comparisons
    one((-1.0, 0.25, 2.0 - 3e-6), (1.0, 0.0, 2e-6), *TRI)


def test_rays_through_a_vertex_and_along_the_edges_are_hits():
    for x, y, uv in ((0.0, 0.0, (0.0, 0.0)), (1.0, 0.0, (1.0, 0.0)), (0.0, 1.0, (0.0, 1.0)),       # the three vertices
                     (0.5, 0.0, (0.5, 0.0)), (0.0, 0.5, (0.0, 0.5)), (0.5, 0.5, (0.5, 0.5)),       # v = 0, u = 0, u + v = 1 exactly
                     (0.25, 0.75, (0.25, 0.75))):
        ok, (t, u, v) = one((x, y, 0.0), (0.0, 0.0, 1.0), *TRI)
        assert ok and (u, v) == (F(uv[0]), F(uv[1])) and t == F(2.0), (x, y, t, u, v)
    for x, y in ((-2.0 ** -20, 0.5), (0.5, -2.0 ** -20), (0.5 + 2.0 ** -20, 0.5)):                  # one step outside each edge
        assert not one((x, y, 0.0), (0.0, 0.0, 1.0), *TRI)[0]


def test_t_at_tmax_is_a_hit_beyond_it_and_behind_the_origin_are_not():
    O, D = (0.25, 0.25, 0.0), (0.0, 0.0, 1.0)
    assert one(O, D, *TRI, tmax=2.0)[0]                                           # inclusive
    assert not one(O, D, *TRI, tmax=float(np.nextafter(F(2.0), F(0.0))))[0]
    assert one(O, D, *TRI, tmax=float(np.nextafter(F(2.0), F(3.0))))[0]
    assert not one((0.25, 0.25, 4.0), D, *TRI)[0]                                 # t = -2
    ok, (t, _, _) = one((0.25, 0.25, 2.0), D, *TRI)                               # t = 0: the origin on the triangle
    assert ok and t == 0.0
    one(O, D, *TRI, tmax=float("nan"))                                            # (whatever a NaN tmax does, both forms do it: agree() checks)


def test_non_finite_values_take_the_same_path():
    nan, inf = float("nan"), float("inf")
    O, D = (0.25, 0.25, 0.0), (0.0, 0.0, 1.0)
    for k in range(3):
        for c in range(3):
            for bad in (nan, inf, -inf):
                tri = [list(p) for p in TRI]
                tri[k][c] = bad
                one(O, D, *tri)      # (a NaN falls through comparisons written as !(x < 0 || ...): such a pair may be ACCEPTED, by both forms alike)
    for c in range(3):
        for bad in (nan, inf, -inf):
            o = list(O); o[c] = bad
            one(o, D, *TRI)
            d = list(D); d[c] = bad
            one(O, d, *TRI)
    assert not one(O, (0.0, 0.0, 0.0), *TRI)[0]                                   # a == 0
    assert not one(O, D, (0, 0, 2), (0, 0, 2), (0, 0, 2))[0]                      # a degenerate triangle
    one(O, D, *[tuple(3e38 * np.asarray(p)) for p in TRI])                         # products overflow


def random_pairs(rng, n, kind):
    v0 = (rng.normal(size=(n, 3)) * 10.0 ** rng.integers(-2, 3, (n, 1))).astype(np.float32)
    e1 = (rng.normal(size=(n, 3)) * 10.0 ** rng.integers(-3, 2, (n, 1))).astype(np.float32)
    e2 = (rng.normal(size=(n, 3)) * 10.0 ** rng.integers(-3, 2, (n, 1))).astype(np.float32)
    O = (rng.normal(size=(n, 3)) * 10.0).astype(np.float32)
    if kind == "unrelated":
        D = rng.normal(size=(n, 3))
    else:
        if kind == "inside":
            u = rng.random(n); v = rng.random(n) * (1 - u)
        else:                                                                      # on the rim: one barycentric 0, or their sum 1, up to rounding
            u = rng.random(n); v = rng.random(n) * (1 - u)
            which = rng.integers(3, size=n)
            u = np.where(which == 0, 0.0, u); v = np.where(which == 1, 0.0, np.where(which == 2, 1.0 - u, v))
        target = v0.astype(np.float64) + u[:, None] * e1 + v[:, None] * e2
        D = target - O
        D *= np.where(rng.random(n) < 0.1, -1.0, 1.0)[:, None]                      # one in ten looks away: t < 0
    D = (D / np.linalg.norm(D, axis=1, keepdims=True)).astype(np.float32)
    return O, D, v0, e1, e2


def test_a_million_seeded_random_pairs():
    rng = np.random.default_rng(20261)
    accepted = total = 0
    with np.errstate(all="ignore"):
        for kind, n in (("inside", 400_000), ("rim", 300_000), ("unrelated", 300_000)):
            O, D, v0, e1, e2 = random_pairs(rng, n, kind)
            a, tuv = agree(O, D, v0, e1, e2, np.full(n, 1e30, np.float32))
            accepted += int(a.sum()); total += n
            # the same pairs with tmax at the true t, one ulp below and one ulp above it, and at half of it
            sel = a == 1
            t = tuv[sel, 0]
            for tm, want in ((t, True), (np.nextafter(t, np.float32(-np.inf)), False), (np.nextafter(t, np.float32(np.inf)), True)):
                a2, _ = agree(O[sel], D[sel], v0[sel], e1[sel], e2[sel], tm.astype(np.float32))
                assert bool(a2.all()) if want else not a2.any(), (kind, want, int(a2.sum()), int(sel.sum()))
    assert total == 1_000_000 and accepted > 300_000, (total, accepted)
