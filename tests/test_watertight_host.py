"""The watertight triangle test on the host (no GPU): tri_test_wt of tinybvh_amd/csrc/device_common.h through tbvh_host_tri_test / tbvh_debug_tri_test_batch
against the real reference built with -DWATERTIGHT_TRITEST -ffp-contract=off (tests/watertight_ref_shim.cpp), the exact negation of a shared edge's two edge
functions, the launch plan of a watertight scene, and the refusals that need no device.  DESIGN.md par. 4.6."""
import ctypes as C

import numpy as np
import pytest

import tinybvh_amd as tb
from tinybvh_amd import _capi

import test_launch_plan_host as P
import watertight_lib as W
from watertight_lib import watertight_refs   # noqa: F401  (session fixture)

F = np.float32
lib = _capi.lib


def _p(a):
    return C.c_void_p(a.ctypes.data)


def batch(test, rays, tris9, roles=0, want_uvw=False):
    rays = np.ascontiguousarray(rays); tris9 = np.ascontiguousarray(tris9, F).reshape(-1, 9)
    n = rays.shape[0]
    acc, tuv = np.full(n, 7, np.uint8), np.zeros((n, 3), F)
    uvw = np.zeros((n, 3), F) if want_uvw else None
    tb.check(lib.tbvh_debug_tri_test_batch(test, roles, _p(rays), _p(tris9), n, _p(acc), _p(tuv), _p(uvw) if want_uvw else None), "tbvh_debug_tri_test_batch")
    return (acc, tuv, uvw) if want_uvw else (acc, tuv)


def same_bits_or_both_nan(a, b):
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def random_pairs(n, seed):
    """rays and triangles of several kinds: aimed into the triangle, at a vertex, at a point of an edge, unrelated"""
    rng = np.random.default_rng(seed)
    tri = rng.uniform(-2, 2, (n, 3, 3)).astype(F)
    O = rng.uniform(-4, 4, (n, 3)).astype(F)
    kind = rng.integers(0, 4, n)
    w = rng.dirichlet((1, 1, 1), n).astype(F)
    e = rng.random(n).astype(F)
    inside = (tri * w[:, :, None]).sum(1)
    vertex = tri[np.arange(n), rng.integers(0, 3, n)]
    k = rng.integers(0, 3, n)
    edge = tri[np.arange(n), k] * e[:, None] + tri[np.arange(n), (k + 1) % 3] * (1 - e)[:, None]
    other = rng.uniform(-2, 2, (n, 3)).astype(F)
    target = np.where((kind == 0)[:, None], inside, np.where((kind == 1)[:, None], vertex, np.where((kind == 2)[:, None], edge, other))).astype(F)
    return W.make_rays(O, target - O), tri.reshape(n, 9)


def special_pairs():
    """degenerate and zero-area triangles, a NaN vertex, every sign of the dominant axis (D[kz] < 0 swaps kx, ky), axis-parallel rays, a triangle behind the ray"""
    O, D, T = [], [], []
    base = np.array([[0, 0, 5], [1, 0, 5], [0, 1, 5]], F)
    for axis in range(3):
        for sign in (1, -1):
            d = np.zeros(3, F); d[axis] = sign
            tri = np.roll(base, axis - 2, 1) * F(sign)
            for o in ([0.2, 0.2, 0.0], [0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.5, 0.5, 0.0], [2.0, 2.0, 0.0]):   # inside, at v0, at v1, on the edge v1-v2, outside
                O.append(np.roll(np.array(o, F), axis - 2) * F(sign)); D.append(d + np.array([1e-3, -2e-3, 3e-3], F) * (0 if o[0] == 0.2 else 1)); T.append(tri)
    z = np.array([0.25, 0.25, 0], F)
    for tri in ([[0, 0, 5], [0, 0, 5], [0, 0, 5]], [[0, 0, 5], [1, 1, 5], [2, 2, 5]], [[0, 0, 5], [1, 0, 5], [np.nan, 1, 5]], [[np.nan] * 3] * 3, [[0, 0, -5], [1, 0, -5], [0, 1, -5]],
                [[0, 0, 5], [1, 0, 5], [0, 1, np.inf]], [[0.25, 0.25, 1], [0.25, 0.25, 2], [0.25, 0.25, 3]]):
        O.append(z); D.append(np.array([0, 0, 1], F)); T.append(np.array(tri, F))
    return W.make_rays(np.array(O, F), np.array(D, F)), np.array(T, F).reshape(-1, 9)


def aimed_pairs():
    """every aimed ray of star12 against the triangle the brute force reports for it and against that triangle's neighbour in the quad"""
    verts, rays, g = W.fixture_inputs(12)
    n = int(g["n_aimed"])
    prim = g["wt"][:n, 3].astype(np.int64)
    tri = verts[:, :3].reshape(-1, 9)
    return np.concatenate([rays[:n], rays[:n]]), np.concatenate([tri[prim], tri[prim ^ 1]])


def test_the_arithmetic_is_the_uncontracted_reference_bit_for_bit(watertight_refs):
    ref = watertight_refs["wt"]
    n_hit = 0
    for rays, tris in (random_pairs(100_000, 3), special_pairs(), aimed_pairs()):
        want_acc, want_tuv, want_occ = ref.pairs(rays, tris)
        acc, tuv = batch(tb.TRITEST_WATERTIGHT, rays, tris)
        assert np.array_equal(acc, want_acc), ("accept differs", np.flatnonzero(acc != want_acc)[:5])
        hit = acc == 1
        assert same_bits_or_both_nan(tuv[hit], want_tuv[hit]).all(), "t, u, v differ in bits"
        occ, _ = batch(tb.TRITEST_WATERTIGHT, rays, tris, roles=1)   # TriOccludes' vertex roles: another summation order of the same edge functions
        assert np.array_equal(occ, want_occ), ("occlusion differs", np.flatnonzero(occ != want_occ)[:5])
        n_hit += int(hit.sum())
    assert n_hit > 40_000   # the comparison is not vacuous


def test_one_pair_per_call_agrees_with_the_batch():
    rays, tris = random_pairs(300, 9)
    acc, tuv = batch(tb.TRITEST_WATERTIGHT, rays, tris)
    for i in range(rays.shape[0]):
        t, u, v = C.c_float(0), C.c_float(0), C.c_float(0)
        tri = tris[i].reshape(3, 3).copy()
        r = lib.tbvh_host_tri_test(tb.TRITEST_WATERTIGHT, _p(rays[i:i + 1]), _p(tri[0]), _p(tri[1]), _p(tri[2]), C.byref(t), C.byref(u), C.byref(v))
        assert r == int(acc[i])
        if r:
            assert np.array_equal(np.array([t.value, u.value, v.value], F).view(np.uint32), tuv[i].view(np.uint32))


def test_test_0_is_the_existing_moller_trumbore_export_bit_for_bit():
    for rays, tris in (random_pairs(100_000, 4), special_pairs()):
        t9 = tris.reshape(-1, 3, 3)
        e = np.concatenate([t9[:, 0], t9[:, 1] - t9[:, 0], t9[:, 2] - t9[:, 0]], 1).astype(F)   # {v0, e1, e2}, the subtraction rounded once as in the export
        od = np.ascontiguousarray(np.concatenate([rays["O"], rays["D"]], 1), F)
        tm = np.ascontiguousarray(rays["t"], F)
        n = rays.shape[0]
        ab, af, tb_, tf = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros((n, 3), F), np.zeros((n, 3), F)
        tb.check(lib.tbvh_debug_tri_test_flat(_p(od), _p(np.ascontiguousarray(e)), _p(tm), n, _p(ab), _p(af), _p(tb_), _p(tf)), "tbvh_debug_tri_test_flat")
        acc, tuv = batch(tb.TRITEST_MOLLER_TRUMBORE, rays, tris)
        assert np.array_equal(acc, ab)
        assert same_bits_or_both_nan(tuv[acc == 1], tb_[acc == 1]).all()


# Which of tri_test_wt's three edge functions belongs to edge k (corner k -> corner (k + 1) % 3) of a triangle, in IntersectTri's roles C, A, B = v0, v1, v2:
# U = Cx By - Cy Bx is the edge v2 -> v0's, V = Ax Cy - Ay Cx the edge v0 -> v1's, W = Bx Ay - By Ax the edge v1 -> v2's, each as seen from the far end
# (U = e( v0 -> v2 ) = -e( v2 -> v0 ) in exact arithmetic and, product by product, in floating point).
EDGE_FUNCTION = {0: 1, 1: 2, 2: 0}
EDGE_CHUNK = 32


def _edge_chunks(N):
    """(rays tiled, triangles of side a, of side b, columns, same direction) per chunk of EDGE_CHUNK interior edges: EVERY interior edge against EVERY aimed ray"""
    verts, rays, g = W.fixture_inputs(N)
    rays = rays[:int(g["n_aimed"])]
    tri = verts[:, :3].reshape(-1, 9)
    edges = W.interior_edges(N)
    assert len(edges) == 3 * tri.shape[0] // 2   # closed: every edge has exactly two triangles
    for at in range(0, len(edges), EDGE_CHUNK):
        e = np.array([(a, ea, b, eb, same) for a, ea, b, eb, same in edges[at:at + EDGE_CHUNK]], np.int64)
        n = rays.shape[0]
        yield (np.tile(rays, e.shape[0]), np.repeat(tri[e[:, 0]], n, 0), np.repeat(tri[e[:, 2]], n, 0), np.repeat(np.array([EDGE_FUNCTION[k] for k in e[:, 1]]), n),
               np.repeat(np.array([EDGE_FUNCTION[k] for k in e[:, 3]]), n), np.repeat(e[:, 4].astype(bool), n), tri, e)


@pytest.mark.parametrize("N", [4, 12])
def test_every_interior_edge_has_exactly_opposite_edge_functions_in_its_two_triangles_for_every_aimed_ray(N):
    pairs = zeros = opposite = 0
    for rays, ta, tb_, ca, cb, same, _, _ in _edge_chunks(N):
        _, _, fa = batch(tb.TRITEST_WATERTIGHT, rays, ta, want_uvw=True)
        _, _, fb = batch(tb.TRITEST_WATERTIGHT, rays, tb_, want_uvw=True)
        a = fa[np.arange(fa.shape[0]), ca]; b = fb[np.arange(fb.shape[0]), cb]
        # two triangles that run along their shared edge in opposite directions (the faces of one cube side): exact negatives, or both zero; in the same
        # direction (where two cube sides with opposite windings meet): the same bits — either way exactly one side of the edge is inside each
        neg = (a.view(np.uint32) ^ np.uint32(0x80000000)) == b.view(np.uint32)
        both_zero = (a == 0) & (b == 0)
        bad = np.where(same, a.view(np.uint32) != b.view(np.uint32), ~(neg | both_zero))
        opposite += int((~same).sum())
        assert not bad.any(), ("an edge's two edge functions are not exact negatives", N, int(bad.sum()), a[bad][:3], b[bad][:3])
        pairs += a.size; zeros += int(both_zero.sum())
    assert pairs == (18 * N * N) * (108 * N * N) and zeros < pairs // 2 and opposite > pairs // 2   # every edge x every aimed ray, and real numbers were compared


def test_the_reference_s_expression_built_with_contraction_breaks_the_negation(watertight_refs):
    """the same check over the reference's edge-function expression as each build of the shim contracts it (tests/watertight_ref_shim.cpp: wref_edge): the
    contracted build has violations, the uncontracted one has none and equals the library's edge functions bit for bit"""
    bad = {"wt": 0, "wt_fma": 0}
    for k, (rays, ta, _, ca, _, _, _, e) in enumerate(_edge_chunks(12)):
        if k >= 8:   # 256 edges x 15 552 rays
            break
        t3 = ta.reshape(-1, 3, 3)
        # the directed edge whose function column ca is: U = e( v0 -> v2 ), V = e( v1 -> v0 ), W = e( v2 -> v1 )
        src = np.array([0, 1, 2])[ca]; dst = np.array([2, 0, 1])[ca]
        P = t3[np.arange(t3.shape[0]), src]; Q = t3[np.arange(t3.shape[0]), dst]
        for name in bad:
            f = watertight_refs[name].edge(rays, np.concatenate([P, Q], 1)); r = watertight_refs[name].edge(rays, np.concatenate([Q, P], 1))
            ok = ((f.view(np.uint32) ^ np.uint32(0x80000000)) == r.view(np.uint32)) | ((f == 0) & (r == 0))
            bad[name] += int((~ok).sum())
            if name == "wt":
                _, _, fa = batch(tb.TRITEST_WATERTIGHT, rays, ta, want_uvw=True)
                assert np.array_equal(fa[np.arange(fa.shape[0]), ca].view(np.uint32), f.view(np.uint32))   # the library's edge function IS the uncontracted expression
    print("edge functions that are not exact negatives across 256 edges x 15 552 rays: contracted build", bad["wt_fma"], "uncontracted", bad["wt"])
    assert bad["wt"] == 0 and bad["wt_fma"] >= 1


def test_the_reference_built_with_contraction_leaks_and_without_it_does_not(watertight_refs):
    """why the library's form is the uncontracted one: g++ -mfma fuses Cx * By - Cy * Bx, the two triangles of an edge no longer compute exact negatives, and
    rays aimed at edges slip through the reference's own watertight brute force"""
    verts, rays, g = W.fixture_inputs(12)
    n = int(g["n_aimed"])
    fma, _ = watertight_refs["wt_fma"].brute(verts, rays[:n])
    wt, _ = watertight_refs["wt"].brute(verts, rays[:n])
    print("star12 aimed rays missed by the watertight brute force: with contraction", W.misses(fma), "without", W.misses(wt))
    assert W.misses(fma) >= 1 and W.misses(fma) == int(g["fma_misses"])
    assert W.misses(wt) == 0
    assert np.array_equal(W.hit_fields(wt), g["wt"][:n])   # the golden is this build's


def test_the_goldens_hold_what_the_issue_demands_of_them():
    for N in (4, 12):
        _, rays, g = W.fixture_inputs(N)
        mt_bvh, mt, wt_bvh, wt = (int(x) for x in g["counts"])
        assert wt == 0 and mt > 0 and mt_bvh >= mt and wt_bvh >= 1, (N, mt_bvh, mt, wt_bvh, wt)
        assert int(g["n_aimed"]) == 108 * N * N and rays.shape[0] == 108 * N * N + W.N_RANDOM
        assert (g["wt"][:int(g["n_aimed"]), 0].view(F) < W.BVH_FAR).all()


def plan23(f, tri_test):
    a = np.array([f[k] for k in P.FACTS] + [tri_test], np.uint64)
    out = np.full(len(P.PLAN) + 1, 0xDEAD, np.uint32)
    tb.check(lib.tbvh_debug_launch_plan(_p(a), a.size, _p(out), out.size), "tbvh_debug_launch_plan")
    return dict(zip(P.PLAN + ("watertight",), (int(x) for x in out)))


def test_a_watertight_scene_never_gets_the_packet_kernel_or_two_flavors_and_test_0_gets_todays_plan():
    rng = np.random.default_rng(5)
    blobs = (1, 48 * P.MB - 1, 48 * P.MB, 196 * P.MB, 384 * P.MB, 384 * P.MB + 1, 3000 * P.MB)
    ns = (1, 131072, 3 * 2 ** 18, 3 * 2 ** 19, 2 ** 21 - 1, 2 ** 21, 6 * 2 ** 20, 12 * 2 ** 20, 2 ** 24)
    n_probed = 0
    for _ in range(3000):
        pick = lambda xs: xs[int(rng.integers(len(xs)))]
        bit = lambda p1: int(rng.random() < p1)
        f = P.facts(isTlas=bit(0.1), layout=pick((P.CWBVH, P.CWBVH, P.CWBVH, P.BVH_GPU, P.BVH4_GPU)), variant=pick((0, 0, 0, 0, 88, 90, 91, 92, 72)), blobBytes=pick(blobs),
                    n=pick(ns), sizeKnown=bit(0.8), any=bit(0.5), gridOverride=bit(0.15), numCUs=pick((256, 304)), blocks=pick((256 * 24, 304 * 24)),
                    raysPerBlock=pick((128, 96)), expFlags=pick((0, 0, 0, 4, 16, 64)), cohTunerMode=pick((0, 0, 0, 1, 2, 3)), decided0=pick((0, 1, 2, 3)),
                    decided1=pick((0, 1, 2, 3)), decided2=pick((0, 1, 2, 3)), decided3=pick((0, 1, 2, 3)), hasPadded=bit(0.3), hasHybrid=bit(0.7), hasTrisPadded=bit(0.7),
                    probeMemoryOn=bit(0.8), skipTiming=bit(0.2))
        today = P.plan(f)
        n_probed += today["probed"] or today["probedSmall"]
        p0 = plan23(f, 0)
        assert {k: p0[k] for k in P.PLAN} == today and p0["watertight"] == 0   # test 0: exactly the plan it gets today
        p1 = plan23(f, 1)
        if f["isTlas"]:
            assert p1["watertight"] == 0   # (a TLAS has no test of its own)
            continue
        # never probed: no coherent flavor, so no packet kernel (a tuner's schedule 3 included), no two-flavor launch, no verdict slot; one kernel on the packed nodes
        assert p1["watertight"] == 1 and not p1["probed"] and not p1["probedSmall"] and not p1["probedSmallCancelled"] and not p1["tunerMeasures"]
        assert p1["shape"] == P.ONE and not p1["autoPad"] and not p1["soloCandidate"] and not p1["wantsVerdictSlot"]
        assert p1["blocksBase"] == today["blocksBase"] and p1["small"] == today["small"] and p1["huge"] == today["huge"]
    assert n_probed >= 100   # the sweep is not vacuous: it reaches, many times over, the probed launches the mode takes away


def test_refusals_that_need_no_device():
    E = -1   # TBVH_E_INVALID
    assert lib.tbvh_set_triangle_test(None, 1, None, 0, 0) == E
    assert lib.tbvh_scene_triangle_test(None) == E
    rays, tris = random_pairs(1, 1)
    t = C.c_float(0)
    tri = tris.reshape(3, 3).copy()
    assert lib.tbvh_host_tri_test(2, _p(rays), _p(tri[0]), _p(tri[1]), _p(tri[2]), C.byref(t), C.byref(t), C.byref(t)) == E
    assert lib.tbvh_host_tri_test(1, None, _p(tri[0]), _p(tri[1]), _p(tri[2]), C.byref(t), C.byref(t), C.byref(t)) == E
    assert lib.tbvh_debug_tri_test_batch(3, 0, _p(rays), _p(tris), 1, _p(np.zeros(1, np.uint8)), _p(np.zeros(3, F)), None) == E
    assert lib.tbvh_debug_tri_test_batch(1, 0, None, _p(tris), 1, _p(np.zeros(1, np.uint8)), _p(np.zeros(3, F)), None) == E
    with pytest.raises(ValueError):
        tb._Scene.SetTriangleTest(object(), "woop")


def tlas_plan(blas_words, any_hit_seen=1, cap8=100, cap4=100):
    facts = np.array([len(blas_words), any_hit_seen, 1, cap8, cap4] + list(blas_words), np.uint64)
    out = np.full(13 + len(blas_words), 0xDEAD, np.uint32)
    tb.check(lib.tbvh_debug_tlas_plan(_p(facts), facts.size, _p(out), out.size), "tbvh_debug_tlas_plan")
    return out


def test_a_tlas_over_watertight_blases_is_served_by_k_tlas8_alone():
    """tlas_plan.h, sentence 18: per-BLAS fact bit 11 = watertight.  Every BLAS through BVH8_CWBVH arrays (its own, or its 8-wide copy), one class for both kinds of
    query, the 8-wide tree, family Tlas8 (2); never Tlas4 (1), Tlas2 (4) or the flat loop (5).  Without the bit the same BLASes get the plan they get today."""
    CW, B2, B4, HAS8, HAS4, WT = 10, 5, 8, 1 << 9, 1 << 10, 1 << 11
    for words in ([CW | HAS4, B2 | HAS8 | HAS4, B4 | HAS8], [B2 | HAS8 | HAS4], [CW, CW | HAS4], [B4 | HAS8, B4 | HAS8]):
        for seen in (0, 1):
            today = tlas_plan(words, seen)
            wt = tlas_plan([w | WT for w in words], seen)
            n = len(words)
            assert wt[0] == CW and wt[4] == CW and wt[2] == 2 and wt[6] == 2 and wt[1] == 0 and wt[5] == 0, (words, wt)    # class BVH8_CWBVH, family Tlas8, no mix: both kinds
            assert wt[3] == 8 and wt[7] == 8 and wt[8] == 0 and wt[9] == 1 and wt[10] == 1 and wt[11] == 0, (words, wt)    # 8-byte entries, no class of its own, 8-wide tree, no 4-wide
            assert [int(v) for v in wt[13:]] == [0 if (w & 0xff) == CW else 1 | 1 << 8 for w in words]                    # own arrays / the 8-wide copy, for both kinds
            assert np.array_equal(tlas_plan(words, seen), today)
            assert today[2] != 2 or (today[0] == CW)                                                                        # (today's closest-hit family is whatever it was)
    # the 8-wide tree beyond its index range: the plan says so (the caller turns that into an error, never another kernel's launch)
    big = tlas_plan([CW | WT], cap8=0x01000000)
    assert big[10] == 0 and big[2] != 2
