"""Which two-level kernel serves a TLAS (tinybvh_amd/csrc/tlas_plan.h; no GPU needed), driven through tbvh_debug_tlas_plan, which runs the function the
library runs when it classifies a TLAS.  The expected answers come from a model of the rule's sentences kept here (model() below: written from the
sentences, not from the header):

 1. A pinned BLAS is entered through its own arrays.
 2. Otherwise a closest-hit query enters a BVH_GPU or BVH8_CWBVH BLAS through its 4-wide copy, if the BLAS has one and 4-wide copies are allowed.
 3. Otherwise a BVH_GPU BLAS (either kind of query) or a BVH4_GPU BLAS (any-hit only) is entered through its 8-wide copy, if it has one.
 4. Otherwise the BLAS is entered through its own arrays.
 5. A kind's class is the views' common layout, or 0.
 6. `mix` means class 0 with no BVH4_GPU view.
 7. If the closest-hit class comes out 0 without `mix`, it is formed again with 4-wide copies disallowed.
 8. Any-hit queries get their own class only if the TLAS has had an any-hit query, some BLAS's any-hit view differs from its closest-hit view, and the
    any-hit class is BVH8_CWBVH or `mix`; otherwise they take the closest-hit views and class.
 9. A TLAS with a sphere BLAS has one class for both kinds: every BLAS through its own arrays, no copies, no wide trees.
10. The 8-wide tree is wanted if a class in use is BVH8_CWBVH or `mix`.  It fits up to 0x00ffffff nodes.
11. The 4-wide tree is wanted if the closest-hit class is BVH4_GPU.  It fits up to 0x7fffffff blocks.  (Without TLAS nodes no tree fits.)
12. Family: spheres -> TlasSphere.
13. Class BVH4_GPU with the 4-wide tree wanted and fitting -> Tlas4.
14. Class BVH8_CWBVH or `mix` with the 8-wide tree wanted and fitting -> Tlas8.
15. Class VOXELSET -> TlasVoxel.
16. Class BVH_GPU -> Tlas2.
17. Otherwise TlasFlat, with the class layout.
Stack entries are 8 bytes for Tlas8, TlasFlat and TlasSphere, 4 bytes for the others.

The nine rows of tlas_edges_lib.CONFIGS are cases by name (test_rows_of_the_edge_tests): the table of tests/test_tlas_edges_gpu.py, executable."""
import ctypes as C
import itertools
import time

import numpy as np
import pytest

import tinybvh_amd as tb
from tinybvh_amd import _capi
import tlas_edges_lib as E

L2, L4, L8, LS, LV = tb.LAYOUT_BVH_GPU, tb.LAYOUT_BVH4_GPU, tb.LAYOUT_CWBVH, tb.LAYOUT_BVH2_WALD, tb.LAYOUT_VOXELSET
OWN, COPY8, COPY4 = range(3)
SPHERE, TLAS4, TLAS8, VOXEL, TLAS2, FLAT = range(6)
MAX8, MAX4 = 0x00FFFFFF, 0x7FFFFFFF
HEAD_F, HEAD_P = 5, 13


def blas(layout, pinned=False, has8=False, has4=False):
    return (layout, bool(pinned), bool(has8), bool(has4))


def model(b, any_hit_seen, has_nodes, cap8, cap4):
    """the plan words of one case, from the sentences"""
    spheres = any(l == LS for l, _, _, _ in b)

    def view(x, any_hit, allow4):
        layout, pinned, has8, has4 = x
        if spheres or pinned:                                                  # 9, 1
            return OWN
        if not any_hit and allow4 and has4 and layout in (L2, L8):            # 2
            return COPY4
        if has8 and (layout == L2 or (any_hit and layout == L4)):             # 3
            return COPY8
        return OWN                                                             # 4

    def form(any_hit, allow4):
        views = [view(x, any_hit, allow4) for x in b]
        layouts = {L4 if v == COPY4 else L8 if v == COPY8 else x[0] for v, x in zip(views, b)}
        cls = layouts.pop() if len(layouts) == 1 else 0                        # 5
        return views, cls, (not spheres and cls == 0 and L4 not in layouts)    # 6 (layouts still holds all of them when there are several)

    v0, c0, m0 = form(False, True)
    if not spheres and c0 == 0 and not m0:                                     # 7
        v0, c0, m0 = form(False, False)
    v1, c1, m1 = form(True, True)
    own = (not spheres) and any_hit_seen and v1 != v0 and (c1 == L8 or m1)     # 8
    if not own:
        v1, c1, m1 = v0, c0, m0
    want8 = (not spheres) and (c0 == L8 or m0 or c1 == L8 or m1)               # 10
    want4 = (not spheres) and c0 == L4                                         # 11
    fits8 = want8 and has_nodes and cap8 <= MAX8
    fits4 = want4 and has_nodes and cap4 <= MAX4

    def family(c, m):
        if spheres: return SPHERE                                              # 12
        if c == L4 and fits4: return TLAS4                                     # 13
        if (c == L8 or m) and fits8: return TLAS8                              # 14
        if c == LV: return VOXEL                                               # 15
        if c == L2: return TLAS2                                               # 16
        return FLAT                                                            # 17

    words = []
    for c, m in ((c0, m0), (c1, m1)):
        f = family(c, m)
        words += [c, int(m), f, 8 if f in (TLAS8, FLAT, SPHERE) else 4]
    words += [int(own), int(want8), int(fits8), int(want4), int(fits4)]
    return words + [a | k << 8 for a, k in zip(v0, v1)]


def fact_words(b, any_hit_seen, has_nodes, cap8, cap4):
    return [len(b), int(any_hit_seen), int(has_nodes), cap8, cap4] + [l | p << 8 | h8 << 9 | h4 << 10 for l, p, h8, h4 in b]


def ask(cases):
    """the library's plan words of every case, through ONE call (cases back to back)"""
    f = np.array([w for c in cases for w in fact_words(*c)], np.uint64)
    out = np.full(sum(HEAD_P + len(c[0]) for c in cases), 0xDEAD, np.uint32)
    tb.check(_capi.lib.tbvh_debug_tlas_plan(C.c_void_p(f.ctypes.data), f.size, C.c_void_p(out.ctypes.data), out.size), "tbvh_debug_tlas_plan")
    return out


def ask_one(b, any_hit_seen=False, has_nodes=True, cap8=100, cap4=100):
    return tb.tlas_plan_dict(ask([(b, any_hit_seen, has_nodes, cap8, cap4)]))


# every BLAS a TLAS can hold: a copy only where the layout has one (an 8-wide copy of BVH_GPU / BVH4_GPU, a 4-wide one of BVH_GPU / BVH8_CWBVH)
BLAS_STATES = ([blas(L2, p, h8, h4) for p in (0, 1) for h8 in (0, 1) for h4 in (0, 1)] + [blas(L4, p, h8) for p in (0, 1) for h8 in (0, 1)] +
               [blas(L8, p, False, h4) for p in (0, 1) for h4 in (0, 1)] + [blas(LS, p) for p in (0, 1)])


def test_every_small_tlas_against_the_model():
    t0 = time.perf_counter()
    cases = [(b, seen, True, cap8, cap4) for n in (1, 2, 3) for b in itertools.product(BLAS_STATES, repeat=n) for seen in (False, True)
             for cap8 in (MAX8, MAX8 + 1) for cap4 in (MAX4, MAX4 + 1)]
    cases += [(b, seen, False, 100, 100) for n in (1, 2) for b in itertools.product(BLAS_STATES, repeat=n) for seen in (False, True)]   # classified before the nodes are there
    cases += [((blas(LV),) * n, seen, True, cap8, cap4) for n in (1, 2) for seen in (False, True) for cap8 in (MAX8, MAX8 + 1) for cap4 in (MAX4, MAX4 + 1)]
    got = ask(cases)
    want = np.array([w for c in cases for w in model(*c)], np.uint32)
    bad = np.flatnonzero(got != want)
    if bad.size:
        at = 0
        for c in cases:                                                        # the first case that differs, named
            n = HEAD_P + len(c[0])
            if bad[0] < at + n:
                raise AssertionError((c, got[at:at + n].tolist(), want[at:at + n].tolist()))
            at += n
    print(f"{len(cases)} cases, {bad.size} words differ, {time.perf_counter() - t0:.2f} s")
    assert len(cases) > 49000


def row_facts(row, after_first_occluded):
    """the BLASes of a row of tlas_edges_lib.CONFIGS as the library holds them right after the TLAS upload (every unpinned BVH_GPU / BVH8_CWBVH BLAS has its
    4-wide copy) and after the TLAS's first IsOccluded (every unpinned BVH_GPU / BVH4_GPU BLAS has its 8-wide copy too); none where a sphere BLAS is present"""
    sph = E.LS in row.layouts
    return tuple(blas(l, v != 0, has8=after_first_occluded and not sph and v == 0 and l in (L2, L4), has4=not sph and v == 0 and l in (L2, L8))
                 for l, v in zip(row.layouts, row.variants))


@pytest.mark.parametrize("key", list(E.CONFIGS))
def test_rows_of_the_edge_tests(key):
    row = E.CONFIGS[key]
    before = ask_one(row_facts(row, False))
    E.assert_kernel(before["closest"], row.intersect)
    assert not before["any_own"] and before["any"]["family"] == before["closest"]["family"]   # no any-hit query yet: one class
    after = ask_one(row_facts(row, True), any_hit_seen=True)
    E.assert_kernel(after["closest"], row.intersect)
    E.assert_kernel(after["any"], row.occluded)
    assert after["any_own"] == (row.intersect != row.occluded)
    # the `grows` observable of the GPU tests is these copies: a 4-wide copy at the upload, an 8-wide one at the first IsOccluded
    for (_, _, has8, has4), (at_build, at_occ) in zip(row_facts(row, True), row.grows):
        assert has4 == at_build and has8 == at_occ


def test_too_small_for_a_copy_next_to_copied_ones():
    """sentence 7: a BVH_GPU BLAS without copies (too small for one) beside a BVH_GPU BLAS with its 4-wide copy: the views {BVH_GPU, BVH4_GPU} are neither a
    class nor `mix`, so the closest-hit class is formed again without 4-wide copies"""
    p = ask_one((blas(L2), blas(L2, has8=True, has4=True)))
    assert p["closest"]["views"] == ["own", "copy8"] and p["closest"]["layout"] == 0 and p["closest"]["mix"] and p["closest"]["family"] == "Tlas8"
    p = ask_one((blas(L2), blas(L2, has4=True)))                               # no 8-wide copy to fall back to: both through their own arrays
    assert p["closest"]["views"] == ["own", "own"] and p["closest"]["family"] == "Tlas2"
    p = ask_one((blas(L4), blas(L8, has4=True)))                               # with the copy the views agree: no second pass
    assert p["closest"]["views"] == ["own", "copy4"] and p["closest"]["family"] == "Tlas4"


def test_trees_beyond_their_index_range():
    b = (blas(L8, True),)
    assert ask_one(b, cap8=MAX8)["closest"]["family"] == "Tlas8"
    p = ask_one(b, cap8=MAX8 + 1)
    assert p["want8"] and not p["fits8"] and p["closest"]["family"] == "TlasFlat" and p["closest"]["layout"] == L8 and p["closest"]["entry_bytes"] == 8
    b = (blas(L4),)
    assert ask_one(b, cap4=MAX4, cap8=MAX4)["closest"]["family"] == "Tlas4"    # (the 8-wide limit does not bind a tree that is not wanted)
    p = ask_one(b, cap4=MAX4 + 1)
    assert p["want4"] and not p["fits4"] and p["closest"]["family"] == "TlasFlat" and p["closest"]["layout"] == L4


def test_word_counts_are_checked():
    lib = _capi.lib
    f = np.array(fact_words((blas(L2), blas(L4)), False, True, 1, 1), np.uint64)
    out = np.zeros(HEAD_P + 2, np.uint32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    assert lib.tbvh_debug_tlas_plan(p(f), f.size, p(out), out.size) == 0
    assert lib.tbvh_debug_tlas_plan(p(f), f.size - 1, p(out), out.size) == -1   # the last case is cut short
    assert lib.tbvh_debug_tlas_plan(p(f), f.size, p(out), out.size - 1) == -1
    assert lib.tbvh_debug_tlas_plan(p(f), f.size, p(out), out.size + 1) == -1
    assert lib.tbvh_debug_tlas_plan(None, f.size, p(out), out.size) == -1
    f[0] = 0
    assert lib.tbvh_debug_tlas_plan(p(f), f.size, p(out), out.size) == -1       # a TLAS has a BLAS
