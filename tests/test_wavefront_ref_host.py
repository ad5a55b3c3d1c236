"""The path tracer's reference (tests/wavefront_ref.py) checked on its own, and the inputs of tests/test_wavefront_paths_gpu.py checked against its cap on
undecided paths: the reference runs as a complete path tracer over the oracle's traversal, on the CPU, at the GPU tests' sizes and seeds."""
import numpy as np
import pytest

import tinybvh_amd as tb
import wavefront_ref as wr
import wavefront_scenes as ws

UNDECIDED_CAP = 0.005


# ---- the reference by itself ---------------------------------------------------------------------------------------------------

def _one_diffuse_vertex(n, r0=None, r1=None, letter=False, normal=(0.3, 0.9, -0.2)):
    """n camera paths that hit one diffuse triangle at a fixed point, with chosen bounce numbers: feeds Shade through a blue-noise table (the only way in)."""
    N = np.asarray(normal, np.float64); N /= np.linalg.norm(N)
    a = np.cross(N, [1.0, 0.0, 0.0]); a /= np.linalg.norm(a); b = np.cross(N, a)
    tri = np.array([[-a - b, 3 * a - b, -a + 3 * b]]) * 2.0
    verts = ws.pack(tri, ws.DIFFUSE | 0xFFFFFF)
    D = -N + 0.2 * a; D /= np.linalg.norm(D)
    rays, aux = wr.make_queue(tb.RAY_DTYPE, tb.PATH_AUX_DTYPE, -3.0 * D, np.broadcast_to(D, (n, 3)), 1.0, 3.0, 1.0, wr.path_word(np.arange(n), 0, wr.PATH_LAST_SPECULAR))
    rays["prim"] = 0
    table = np.zeros(128 * 128 * 8, np.uint32)
    if r0 is not None:
        table[wr.blue_noise_index(np.arange(n), 128, 1)] = (np.asarray(r0, np.uint32) << 16) | (np.asarray(r1, np.uint32) << 8)     # page 1 = noise1 -> the bounce
    P = wr.Params((0.0, 50.0, 0.0), max_depth=2, seed=1, light_size=(9.0, 5.0), sample_index=0, blue_noise=table if r0 is not None else None, width=128, height=128,
                  reference_letter=letter)
    return wr.shade(rays, aux, wr.Geometry(verts=verts), P, 0), np.sign(N @ -D) * N


def test_malley_directions_have_unit_length_and_the_cosine_of_their_draw():
    r0, r1 = np.meshgrid(np.arange(0, 256, 5), np.arange(0, 256, 5)); r0, r1 = r0.ravel(), r1.ravel()
    ref, N = _one_diffuse_vertex(r0.size, r0, r1)
    R = ref["bounce_D"][0]
    assert ref["want_bounce"].all()
    assert np.abs(np.linalg.norm(R, axis=1) - 1).max() < 1e-12
    r1f = r1 * float(np.float32(0.00392))
    assert np.abs(R @ N - np.sqrt(1 - r1f)).max() < 1e-6          # (N here is the float64 normal; Shade's is the float32 triangle's: 2^-24 apart)
    assert np.abs(ref["bounce_pdf"][0] - np.maximum(R @ N, 1e-6) * wr.INV_PI).max() < 1e-6
    # the bound: worst case over some sixty roundings on the chain (edges, cross product, two normalisations, basis, trig), never zero, never absurd
    e = ref["bounce_D"][1]
    assert (e > 2.0 ** -24).all() and (e < 128 * 2.0 ** -23).all()


def test_cosine_pdf_integrates_to_one():
    """pdf(R) = max(N.R, 1e-6) / pi over the hemisphere about N, by quadrature in (cos theta, phi)."""
    m = 2000
    mu = (np.arange(m) + 0.5) / m
    assert abs((mu * wr.INV_PI).sum() / m * 2 * np.pi - 1.0) < 1e-6


def test_mis_weights_sum_to_the_single_strategy_estimate():
    """One emitter point seen from one diffuse vertex.  Reached by a light sample Shade gives f cos / (p_light + p_brdf); reached by the bounce (at the next
    vertex) T / (p_light + p_brdf) with T = f cos, the postponed p_brdf in D.w.  With both strategies at the same direction the two estimates, each times its
    own pdf, sum to f cos: sum_s p_s * (f cos / (p_l + p_b)) = f cos — the one-strategy estimate times its pdf."""
    lamp = ws.grid((-4.5, 4.0, -2.5), (0, 0, 5), (9, 0, 0), 1, 1, ws.LIGHT | 0xFFFFFF)
    floor = ws.grid((-8, 0, -8), (16, 0, 0), (0, 0, 16), 1, 1, ws.DIFFUSE | 0x808080)
    verts = np.concatenate([floor, lamp])
    geo = wr.Geometry(verts=verts)
    Le = (3.0, 2.0, 1.0)
    P = wr.Params((0.0, 4.0, 0.0), Le, max_depth=2, seed=9, light_size=(9.0, 5.0), width=64, height=64)
    n = 64
    I = np.array([1.0, 0.0, 0.5])
    O = I + np.array([0.3, 2.0, -0.4])
    D = (I - O) / np.linalg.norm(I - O)
    rays, aux = wr.make_queue(tb.RAY_DTYPE, tb.PATH_AUX_DTYPE, O, np.broadcast_to(D, (n, 3)), 1.0, np.linalg.norm(I - O), 1.0, wr.path_word(np.arange(n), 0, wr.PATH_LAST_SPECULAR))
    rays["prim"] = 0
    s0 = wr.shade(rays, aux, geo, P, 0)
    assert s0["want_shadow"].all()
    L, dist = s0["shadow_D"][0], s0["shadow_tmax"][0] + 2 * P.eps
    rho = 0x80 * wr.BYTE
    p_b = L[:, 1] * wr.INV_PI
    p_l = 1.0 / np.minimum(wr.TWO_PI, 45.0 / dist ** 2 * np.abs(L[:, 1]))
    fcos = rho * wr.INV_PI * L[:, 1]
    nee = s0["contrib"][0] / np.array(Le)                                  # Shade's light-sampling estimate, per unit radiance
    assert np.allclose(nee, (fcos / (p_l + p_b))[:, None], rtol=1e-12)
    # the bounce strategy along the same directions: a path arriving at the lamp with T = f cos (Shade's bounce throughput) and D.w = p_b
    I32 = rays["O"].astype(np.float64) + rays["t"][:, None].astype(np.float64) * rays["D"]
    t_l = (4.0 - I32[:, 1]) / L[:, 1]
    r1, a1 = wr.make_queue(tb.RAY_DTYPE, tb.PATH_AUX_DTYPE, I32, L, p_b, t_l, np.broadcast_to(fcos[:, None], (n, 3)), wr.path_word(np.arange(n), 1, wr.PATH_VIA_DIFFUSE))
    r1["O"] = I32.astype(np.float32); r1["prim"] = 2
    s1 = wr.shade(r1, a1, geo, P, 1)
    assert s1["mis_light"].all()
    bsdf = s1["term"][0] / np.array(Le)
    p_b32, L32, t32 = r1["instIdx"].view(np.float32).astype(np.float64), r1["D"].astype(np.float64), r1["t"].astype(np.float64)
    p_l1 = 1.0 / np.minimum(wr.TWO_PI, 45.0 / t32 ** 2 * np.abs(L32[:, 1]))
    assert np.allclose(bsdf, (fcos.astype(np.float32).astype(np.float64) / (p_l1 + p_b32))[:, None], rtol=1e-12)
    # and the sum over the two strategies, each estimate weighted with its pdf
    total = p_l[:, None] * nee + p_b[:, None] * bsdf
    assert np.allclose(total, fcos[:, None], rtol=1e-5)


def test_blue_noise_indices_of_a_hand_computed_pixel():
    """Pixel (x 5, y 40) of a 72 x 52 image: index 40 * 72 + 5 = 2885; Noise( 2885 % 52, 2885 / 52, page ) = ( 25, 55 ); page 3 -> word 3 * 16384 + 55 * 128 + 25."""
    assert int(wr.blue_noise_index(2885, 52, 3)) == 3 * 16384 + 55 * 128 + 25
    assert int(wr.blue_noise_index(2885, 72, 3)) != int(wr.blue_noise_index(2885, 52, 3))
    assert int(wr.blue_noise_index(52 * 130 + 25, 52, 0)) == (2 << 7) + 25                                  # y = 130 wraps to 2


def test_path_word_packing_and_rng():
    assert int(wr.path_word(0x123456, 7, wr.PATH_VIA_DIFFUSE)) == 0x12345672
    assert int(wr.path_word(1, 15, 1)) == 0x1F1 and int(wr.path_word(1, 16, 1)) == 0x101                 # the depth nibble
    assert int(wr.wang(np.uint32(0))) == 3232319850 and wr.clamp_depth(0) == 3 and wr.clamp_depth(9) == 8 and wr.clamp_depth(5) == 5
    f = wr.rnd_stream(np.array([1], np.uint32), 2)
    assert f[0][0] == (270369 >> 8) / 16777216.0 and f[1][0] == (67634689 >> 8) / 16777216.0             # xorshift32 from 1: 270369, 67634689
    assert float(wr.rnd_stream(np.array([0], np.uint32), 1)[0][0]) == f[0][0]                             # state 0 is replaced by 1


def test_error_bounds_follow_the_operations():
    a, b = wr.F(np.array([1.0])), wr.F(np.array([1.0 + 2.0 ** -20]))
    d = a - b                                          # cancellation: the bound is half an ulp of the (tiny) result, no more — operands exact
    assert d.e[0] == wr.U * abs(d.v[0])
    c = (wr.F(np.array([1.25])) * 3.0) - (b * 3.0)                          # ... but rounded operands carry their magnitudes into it
    assert c.e[0] >= 2 * wr.U * 3.0
    assert (a * 2.0).e[0] == 0 and (a + 0.0).e[0] == 0 and (a * 0.5).e[0] == 0       # cannot round
    assert np.isclose(wr.fsqrt(wr.F(np.array([4.0]), np.array([1e-6]))).e[0], 2.5e-7 + wr.U * 2, rtol=1e-3)


# ---- the GPU tests' inputs: undecided paths under the cap, every class of Shade present ---------------------------------------

_traced = {}


def traced(name, oracle):
    if name not in _traced:
        scene, cam, kw, depth, seed = ws.CASES[name]()
        _traced[name] = ws.trace_cpu(oracle, scene, cam, seed, depth, **kw)
    return _traced[name]


@pytest.mark.parametrize("name", sorted(ws.CASES))
def test_undecided_paths_stay_under_the_cap(name, oracle):
    stages = traced(name, oracle)
    share = ws.undecided_share(stages)
    print(name, "live", [s["ref"]["n"] for s in stages], "shadow", [int(s["ref"]["want_shadow"].sum()) for s in stages], "undecided", share)
    assert max(share) <= UNDECIDED_CAP, share
    for s in stages:   # ... and of the shadow queue
        und = (s["ref"]["undecided"][s["ref"]["want_shadow"]] != 0).sum()
        assert und <= UNDECIDED_CAP * max(1, s["shadow"].shape[0]), (und, s["shadow"].shape[0])


def test_every_class_of_shade_occurs_in_scene_a(oracle):
    c = ws.classes(traced("scene_a", oracle))
    c["one_bounce_stop"] = ws.classes(traced("scene_a_one_bounce", oracle))["one_bounce_stop"]
    print(c)
    assert all(v > 0 for v in c.values()), c
    # the mirror chain reaches the last stage the frame allows, still specular
    last = traced("scene_a_chain", oracle)[7]["ref"]
    assert ((last["flags"] & wr.PATH_LAST_SPECULAR) != 0).sum() > 0
    # every material among the first hits
    r0 = traced("scene_a", oracle)[0]["ref"]
    assert r0["miss"].any() and r0["emitter"].any() and r0["specular"].any() and r0["diffuse"].any()


def test_edge_scenes_reach_their_edges(oracle):
    g = traced("grazing", oracle)[0]
    xs_clamped = g["ref"]["decisions"]["clamp"]
    L = g["ref"]["shadow_D"][0][g["ref"]["want_shadow"]]
    assert (np.abs(L[:, 1]) < 0.01).sum() > 100                        # grazing: the solid angle nears 0
    dist = g["ref"]["shadow_tmax"][0][g["ref"]["want_shadow"]] + 0.002
    assert (45.0 / dist ** 2 * np.abs(L[:, 1]) > wr.TWO_PI).sum() > 0   # ... and passes 2 pi right under a sample
    assert xs_clamped["relevant"].sum() == g["ref"]["want_shadow"].sum()
    n = traced("near_point_light", oracle)[0]["ref"]
    assert n["diffuse"].all() and 0 < (n["diffuse"] & ~n["want_shadow"]).sum() < n["n"] // 4 and not n["ndl_rejected"].any()


# ---- undecided paths: flagged, flipped, and held to the side the device took ------------------------------------------------------

def _floor_in_the_lights_plane(n=256):
    """Camera paths onto a floor that contains the point light: N.L is a residue of the inputs' float32 rounding, of either sign and of the size of the
    kernel's own rounding, so `ndl > 0` is undecided for most paths."""
    verts = ws.grid((-4, 0, -4), (8, 0, 0), (0, 0, 8), 1, 1, ws.DIFFUSE | 0x808080)
    rng = np.random.default_rng(3)
    O = np.array([0.3, 2.7, -0.4])
    I = np.stack([rng.uniform(-3, 3, n), np.zeros(n), rng.uniform(-3, 3, n)], -1)
    D = I - O; t = np.linalg.norm(D, axis=1); D /= t[:, None]
    rays, aux = wr.make_queue(tb.RAY_DTYPE, tb.PATH_AUX_DTYPE, O, D, 1.0, t, 1.0, wr.path_word(np.arange(n), 0, wr.PATH_LAST_SPECULAR))
    rays["prim"] = (I[:, 0] < I[:, 2]).astype(np.uint32)          # which of the two triangles: same plane, same material
    P = wr.Params((0.5, 0.0, 0.7), (2.0, 2.0, 2.0), max_depth=1, seed=4, width=16, height=16)
    return rays, aux, wr.Geometry(verts=verts), P


def test_undecided_paths_are_flagged_and_flip_takes_the_other_side():
    rays, aux, geo, P = _floor_in_the_lights_plane()
    a = wr.shade(rays, aux, geo, P, 0)
    und = (a["undecided"] & wr.DEC_NDL) != 0
    assert und.sum() > a["n"] // 2 and (a["undecided"] & ~wr.DEC_NDL == 0).all()
    assert 0 < a["want_shadow"][und].sum() < und.sum()             # the residue falls on both sides
    b = wr.shade(rays, aux, geo, P, 0, flip=wr.DEC_NDL)
    assert np.array_equal(b["want_shadow"], ~a["want_shadow"]) and np.array_equal(b["undecided"], a["undecided"])
    half = np.where(np.arange(a["n"]) % 2 == 0, wr.DEC_NDL, 0)
    c = wr.shade(rays, aux, geo, P, 0, flip=half)
    assert np.array_equal(c["want_shadow"], np.where(half != 0, ~a["want_shadow"], a["want_shadow"]))


def test_the_gpu_tests_hold_an_undecided_path_to_the_side_it_took():
    """check_shade of tests/test_wavefront_paths_gpu.py on a made-up device that took the other side on every second path: accepted; the same with one
    shadow ray's reach off by more than its bound: refused.  A decided path has no such licence."""
    import test_wavefront_paths_gpu as gpu_tests
    rays, aux, geo, P = _floor_in_the_lights_plane()
    und = wr.shade(rays, aux, geo, P, 0)["undecided"] != 0
    half = np.where(und & (np.arange(rays.shape[0]) % 2 == 0), wr.DEC_NDL, 0)
    dev = wr.shade(rays, aux, geo, P, 0, flip=half)
    w = dev["want_shadow"]
    sh, sh_aux = wr.make_queue(tb.RAY_DTYPE, tb.PATH_AUX_DTYPE, dev["shadow_O"][0][w], dev["shadow_D"][0][w], 1.0, dev["shadow_tmax"][0][w], dev["contrib"][0][w],
                               dev["pixel"][w].astype(np.uint32))
    ref, u = gpu_tests.check_shade(rays, aux, geo, P, 0, shadow=(sh, sh_aux))
    assert u == und.sum() and np.array_equal(ref["want_shadow"], w)
    k = int(np.flatnonzero(und[dev["pixel"][w]])[0])                # a shadow ray of an undecided path
    bad = sh.copy(); bad["t"][k] *= np.float32(1.001)              # (its contribution is all rounding residue: the reach is what has a tight bound)
    with pytest.raises(AssertionError, match="neither side"):
        gpu_tests.check_shade(rays, aux, geo, P, 0, shadow=(bad, sh_aux))
    # a decided path gets no such licence: the ordinary floor under the light, one contribution off
    P2 = wr.Params((0.5, 3.0, 0.7), (2.0, 2.0, 2.0), max_depth=1, seed=4, width=16, height=16)
    d2 = wr.shade(rays, aux, geo, P2, 0)
    assert d2["want_shadow"].all() and not d2["undecided"].any()
    sh, sh_aux = wr.make_queue(tb.RAY_DTYPE, tb.PATH_AUX_DTYPE, d2["shadow_O"][0], d2["shadow_D"][0], 1.0, d2["shadow_tmax"][0], d2["contrib"][0], d2["pixel"].astype(np.uint32))
    gpu_tests.check_shade(rays, aux, geo, P2, 0, shadow=(sh, sh_aux))
    sh_aux["T"][7] *= np.float32(1.0001)
    with pytest.raises(AssertionError, match="decided paths differ"):
        gpu_tests.check_shade(rays, aux, geo, P2, 0, shadow=(sh, sh_aux))
