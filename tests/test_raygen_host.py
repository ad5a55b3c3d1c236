"""The references of raygen_ref.py, checked on the CPU before anything on a GPU is held to them: the float32 restatements against the
float64 references on the very inputs test_raygen_gpu.py uses, the host generators of tinybvh_amd.rays against the same float64
references, the integer parts (pixel order, WangHash, xorshift32, Morton interleave) against second, naive implementations, and the
ray-bin key at its edges."""
import os

import numpy as np
import pytest

import raygen_ref as G
import tinybvh_amd as tb
from tinybvh_amd import rays as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F = np.float32


@pytest.fixture(scope="module")
def traced(oracle):
    """The primary batches of G.TRACED_VIEWS traced by the CPU oracle (the GPU test traces them with scene.Intersect): name -> (verts, records)."""
    out = {}
    for name in G.TRACED_VIEWS:
        verts = np.load(os.path.join(GOLDEN, name + ".npz"))["verts"]
        h = tb.HostBVH(verts, tb.LAYOUT_CWBVH, threads=1)
        out[name] = (verts, oracle.bvh2_intersect(h.bvh2_nodes(), h.bvh2_prim_idx(), verts, G.traced_view_rays(name)))
    return out


def test_pixel_order_is_the_speedtests_loop_nest():
    """tiles row by row, 4x4 pixels per tile with x fastest, spp samples per pixel (tiny_bvh_speedtest.cpp:526-533), written as the loops"""
    for w, h, sx, sy in ((8, 4, 1, 1), (12, 8, 2, 2), (4, 8, 3, 2)):
        want = [(px * sx + s % sx, py * sy + s // sx)
                for ty in range(h // 4) for tx in range(w // 4) for y in range(4) for x in range(4)
                for px, py in [(tx * 4 + x, ty * 4 + y)] for s in range(sx * sy)]
        nu, nv = G.pixel_map(w, h, sx, sy, 0, len(want))
        assert list(zip(nu.tolist(), nv.tolist())) == want
        nu2, nv2 = G.pixel_map(w, h, sx, sy, 5, 7)
        assert list(zip(nu2.tolist(), nv2.tolist())) == want[5:12]
    # the far end of a 65536 x 65536 image at 2 x 2 samples: the last ray is sample 3 of pixel (65535, 65535)
    nu, nv = G.pixel_map(65536, 65536, 2, 2, 2 ** 34 - 1, 1)
    assert (int(nu[0]), int(nv[0])) == (131071, 131071)


@pytest.mark.parametrize("name", list(G.primary_cases()))
def test_primary_restatement_and_host_generator_within_f64_bound(name):
    cam, first, n = G.primary_cases()[name]
    ref = G.primary_f64(cam, first, n)
    got = G.primary_f32(cam, first, n)
    G.compare_f64(got, ref, "restated " + name)
    host = R.primary(cam, first, n)
    G.compare_f64(host, ref, "rays.primary " + name)
    assert np.array_equal(host["O"], got["O"]) and np.array_equal(host["mask"], got["mask"]) and np.array_equal(host["t"], got["t"])
    assert np.array_equal(got["rD"], tb.safercp(got["D"]))


def test_primary_zero_components():
    cam, first, n = G.primary_cases()["symmetric"]
    r = G.primary_f32(cam, first, n)
    nu, nv = G.pixel_map(cam.width, cam.height, cam.spp_x, cam.spp_y, first, n)
    col, row = nu == cam.width * cam.spp_x // 2, nv == cam.height * cam.spp_y // 2
    assert col.sum() == cam.height * cam.spp_y and row.sum() == cam.width * cam.spp_x
    assert (r["D"][col, 0] == 0).all() and (r["rD"][col, 0] == G.FAR).all() and (r["D"][~col, 0] != 0).all()
    assert (r["D"][row, 1] == 0).all() and (r["rD"][row, 1] == G.FAR).all()
    cam, first, n = G.primary_cases()["negative_zero"]
    r = G.primary_f32(cam, first, n)
    assert r["D"][0, 0] == 0 and np.signbit(r["D"][0, 0]) and r["rD"][0, 0] == G.FAR


def test_safercp_edges():
    x = np.array([0.0, -0.0, 1e-12, -1e-12, 1.0000001e-12, -1.0000001e-12, 1e-20, -1e-20, 0.5, -4.0, np.inf, -np.inf], F)
    want = np.array([1e30, 1e30, 1e30, -1e30, 1 / F(1.0000001e-12), -1 / F(1.0000001e-12), 1e30, -1e30, 2.0, -0.25, 0.0, -0.0], F)
    for f in (G.safercp_f32, tb.safercp):
        assert np.array_equal(f(x).view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("name", list(G.TRACED_VIEWS))
def test_bounce_restatement_within_f64_bound_and_under_the_knife_edge_cap(traced, name):
    verts, rec = traced[name]
    hit = rec["t"] < G.FAR
    assert 0.2 < hit.mean() < 0.95, hit.mean()        # hits and misses mixed
    batches = []
    for seed in G.BOUNCE_SEEDS:
        assert G.seeds_ok(seed, rec.shape[0])
        ref = G.bounce_f64(rec, verts, seed)
        assert ref["knife"].sum() <= G.KNIFE_CAP * rec.shape[0]       # the reference alone stays under the cap
        got = G.bounce_f32(rec, verts, seed)
        G.compare_f64(got, ref, f"restated bounce {name} seed {seed}")
        assert np.array_equal(got["rD"], tb.safercp(got["D"]))
        batches.append(got)
    assert not np.array_equal(batches[0]["D"], batches[1]["D"])


def test_bounce_construction(traced):
    """What the contract says, looked at directly on the float64 reference: a bounce leaves on the side the ray came from, misses spawn at
    O + 20 D unreversed, and the batch is not degenerate (directions spread over the hemisphere)."""
    verts, rec = traced["soup_2k"]
    ref = G.bounce_f64(rec, verts, G.BOUNCE_SEEDS[0])
    hit = rec["t"] < G.FAR
    D_in = rec["D"].astype(np.float64)
    N = G._tri_normal64(verts, np.where(hit, rec["prim"], 0))
    front = np.where(((N * D_in).sum(1) > 0)[:, None], -N, N)      # the normal on the incoming ray's side
    sure = hit & ~ref["knife"]
    assert ((front * ref["D"]).sum(1)[sure] >= 0).all()
    assert ((N * D_in).sum(1)[hit] > 0).sum() > 100                 # triangles seen from their back side are in the batch
    miss = ~hit
    I = rec["O"].astype(np.float64) + 20.0 * D_in
    R0 = G.bounce_draws(G.BOUNCE_SEEDS[0], rec.shape[0]).astype(np.float64) - 0.5
    assert np.allclose(ref["O"][miss], (I + float(G.BOUNCE_OFFSET) * R0 / np.linalg.norm(R0, axis=1, keepdims=True))[miss], rtol=0, atol=1e-12)
    assert np.abs(ref["D"].mean(axis=0)).max() < 0.6 and len(np.unique(ref["D"].round(3), axis=0)) > 0.99 * rec.shape[0]


@pytest.mark.parametrize("name", list(G.TRACED_VIEWS))
def test_shadow_restatement_and_host_generator_within_f64_bound(traced, name):
    _, rec = traced[name]
    for eps in (G.SHADOW_EPS, 0.0):
        ref = G.shadow_f64(rec, G.SHADOW_LIGHT, eps)
        got = G.shadow_f32(rec, G.SHADOW_LIGHT, eps)
        G.compare_f64(got, ref, f"restated shadow {name} eps {eps}")
        G.compare_f64(R.shadow(rec, G.SHADOW_LIGHT, eps), ref, f"rays.shadow {name} eps {eps}")
        assert np.array_equal(got["rD"], tb.safercp(got["D"]))


def test_shadow_light_on_the_hit_point():
    rec = tb.make_rays(np.array([[1.0, 2.0, 3.0]], F), np.array([[0.0, 0.0, 1.0]], F))
    rec["t"] = 2.0
    for eps in (G.SHADOW_EPS, 0.0):
        r = G.shadow_f32(rec, (1.0, 2.0, 5.0), eps)
        assert np.array_equal(r["O"][0], [1, 2, 5]) and np.array_equal(r["D"][0].view(np.uint32), [0, 0, 0])
        assert (r["rD"][0] == G.FAR).all() and r["t"][0] == -F(eps)
        ref = G.shadow_f64(rec, (1.0, 2.0, 5.0), eps)
        assert ref["t"][0] == -float(F(eps)) and not np.isnan(ref["O"]).any() and not np.isnan(ref["D"]).any()


def test_wang_hash_and_xorshift_known_answers():
    """against a loop over Python integers masked to 32 bits, for 1000 ray indices of which half lie at and above 2^32"""
    M = 0xFFFFFFFF

    def wang(s):
        s = ((s ^ 61) ^ (s >> 16)) & M
        s = (s * 9) & M
        s = s ^ (s >> 4)
        s = (s * 0x27d4eb2d) & M
        return s ^ (s >> 15)

    def draws(s):
        out = []
        for _ in range(3):
            s ^= (s << 13) & M
            s ^= s >> 17
            s ^= (s << 5) & M
            out.append(s)
        return out

    idx = list(range(500)) + [2 ** 32 - 2 + k for k in range(250)] + [2 ** 34 - 250 + k for k in range(250)]
    for seed in (0, 5, 0x9E3779B9, M):
        want_state = [wang((seed + i * 747796405 + (i >> 32)) & M) for i in idx]
        got_state = G.ray_seeds(seed, np.array(idx, np.uint64))
        assert got_state.tolist() == want_state
        assert G.xorshift_draws(got_state).tolist() == [draws(s) for s in want_state]
    # the index within the call counts in full: i and i + 2^32 draw differently
    assert G.ray_seeds(5, [7])[0] != G.ray_seeds(5, [7 + 2 ** 32])[0]
    # float32( draw ) * float32( 2.3283064365387e-10 ), spelled out for the largest and smallest draws
    assert G.DRAW_SCALE == F(2.0 ** -32)
    d = np.array([[1, 0x7FFFFFFF, 0xFFFFFFFF]], np.uint32).astype(F) * G.DRAW_SCALE
    assert d.dtype == F and d.tolist() == [[2.0 ** -32, 0.5, 1.0]]


def test_morton_interleave_against_a_per_bit_loop():
    c = np.arange(64, dtype=np.uint32)
    x, y, z = [a.reshape(-1) for a in np.meshgrid(c, c, c, indexing="ij")]
    got = G.morton3(x, y, z, 6)
    for i in range(0, x.size, 1):
        code = 0
        for j in range(6):
            code |= ((int(x[i]) >> j) & 1) << (3 * j) | ((int(y[i]) >> j) & 1) << (3 * j + 1) | ((int(z[i]) >> j) & 1) << (3 * j + 2)
        assert code == int(got[i])
    assert len(np.unique(got)) == 64 ** 3 and int(got.max()) == 2 ** 18 - 1


def test_bin_key_edges():
    bounds = (0.0, 0.0, 0.0, 8.0, 8.0, 8.0)
    inf, nan = np.inf, np.nan
    O = np.array([[0, 0, 0], [8, 8, 8], [-1, 9, 4], [3, 3.9999998, 4], [nan, inf, -inf], [7.9999995, 1e30, -1e30]], F)
    assert G.bin_cells(O, bounds, 3).tolist() == [[0, 0, 0], [7, 7, 7], [0, 7, 4], [3, 3, 4], [0, 7, 0], [7, 7, 0]]
    assert G.bin_cells(O, bounds, 0).tolist() == [[0, 0, 0]] * 6
    # no extent, or a reversed one, on an axis: scale 0, every finite origin in cell 0 of that axis (an infinite one gives inf * 0 = NaN -> 0)
    assert G.bin_cells(O, (0, 2, 0, 8, 2, 8), 3)[:, 1].tolist() == [0] * 6
    assert G.bin_cells(O, (0, 8, 0, 8, 0, 8), 3)[:, 1].tolist() == [0] * 6
    r = tb.make_rays(np.array([[1, 2, 3]] * 4, F), np.array([[1, 1, 1], [-1, 1, 1], [1, 1, -1], [-0.0, -1, 0.0]], F), normalize=False)
    cell = int(G.morton3([1], [2], [3], 3)[0])
    assert cell == 0b110101      # x = 001 -> bit 0; y = 010 -> bit 4; z = 011 -> bits 2 and 5
    assert G.bin_keys(r, bounds, 3, 0).tolist() == [cell] * 4
    assert G.bin_keys(r, bounds, 3, 1).tolist() == [cell << 3 | o for o in (0, 4, 1, 2)]        # -0.0 is not negative
    assert G.bin_keys(r, bounds, 3, 2).tolist() == [o << 9 | cell for o in (0, 4, 1, 2)]
    assert G.bin_keys(r, bounds, 0, 1).tolist() == [0, 4, 1, 2] and G.bin_count(0, 0) == 1 and G.bin_count(6, 1) == 2 ** 21 and G.bin_count(6, 0) == 2 ** 18
