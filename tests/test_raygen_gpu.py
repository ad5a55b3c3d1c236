"""The device ray generators (k_gen_primary, k_gen_bounce, k_gen_shadow behind tbvh_generate_{primary,bounce,shadow}_device) held to the
references of raygen_ref.py, which are written from the header's contract and checked on the CPU by test_raygen_host.py.  Every large
measurement of this repository traces what these kernels write, and the parity tests hand the oracle the very same rays: only a
reference of the generators themselves notices a wrong one.

Per record: the fields no generator computes are exact (mask 0xFFFF, instIdx, inst, u, v, prim 0, t = tmax), rD is bit-equal to
tb.safercp of the device's own D, O / D / t lie inside the float64 reference's running-error bound (raygen_ref.py: "The bound"), and
O / D / t are bit-equal to the float32 restatement (the library is built without contraction and with correctly rounded divide and
square root).  Bounce rays whose sign decisions lie within 1e-6 of zero in float64 may be the reversed ray; at most 0.1 % of a batch.

Figures.  Every test prints, before it asserts, the largest distance from the float64 reference (absolute, and as a share of the
bound) and the largest ulp distance from the restatement.  NOT YET MEASURED ON HARDWARE: no MI355X could be had while these tests were
written, so the bit equality is still an expectation.  What is measured is the float32 restatement itself (test_raygen_host.py, the
same inputs) — D within 2.98e-7 of float64 for primary rays (0.35 of the bound), 1.51e-7 for bounce rays (0.24), 2.49e-7 for shadow
rays (0.26); O within 3.3e-6 (bounce, 0.97) and 6.0e-5 (shadow, whose misses start 1000 units out; 0.96); shadow t within 1.2e-4
(0.41); no ray of the four bounce batches lies on a knife edge.  The first hardware run either confirms these figures or is a finding.
"""
import os

import numpy as np
import pytest

import raygen_ref as G
import tinybvh_amd as tb

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F = np.float32
POISON = 0xA5
INVALID = -1   # TBVH_E_INVALID


def generate(ctx, n, call, prefill=None, lead=0):
    """Run call(d_out) on a poisoned device buffer of lead + n + 1 records (d_out = the record after the lead) and return the n records;
    the records around them must come back untouched."""
    buf = np.full((lead + n + 1) * 64, POISON, np.uint8)
    if prefill is not None:
        buf[lead * 64:(lead + n) * 64] = prefill.view(np.uint8)
    d = ctx.malloc(buf.nbytes)
    try:
        ctx.to_device(d, buf)
        call(d + lead * 64)
        ctx.synchronize()
        ctx.from_device(buf, d)
    finally:
        ctx.free(d)
    assert (buf[:lead * 64] == POISON).all() and (buf[(lead + n) * 64:] == POISON).all(), "the generator wrote outside its n records"
    return buf[lead * 64:(lead + n) * 64].copy().view(tb.RAY_DTYPE)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def hold(got, ref32, ref64, label):
    """The checks common to all three generators."""
    assert (got["mask"] == 0xFFFF).all() and (got["instIdx"] == 0).all() and (got["inst"] == 0).all() and (got["prim"] == 0).all(), label
    assert (bits(got["u"]) == 0).all() and (bits(got["v"]) == 0).all(), label
    assert np.array_equal(bits(got["rD"]), bits(tb.safercp(got["D"]))), label
    zero = got["D"] == 0
    assert (bits(got["rD"][zero]) == bits(G.FAR)).all(), label          # +0.0 and -0.0 both give +1e30
    assert not np.isnan(got["O"]).any() and not np.isnan(got["D"]).any() and not np.isnan(got["rD"]).any() and not np.isnan(got["t"]).any(), label
    fig = G.compare_f64(got, ref64, label)
    ulps = {f: G.ulp_distance(got[f], ref32[f]) for f in ("O", "D", "t")}
    differ = {f: int((bits(got[f]) != bits(ref32[f])).sum()) for f in ("O", "D", "t")}
    print("f32", label, "max ulp distance", ulps, "differing words", differ)
    assert np.array_equal(bits(got["t"]), bits(ref32["t"])), label
    assert np.array_equal(bits(got["O"]), bits(ref32["O"])) and np.array_equal(bits(got["D"]), bits(ref32["D"])), (label, ulps, differ)
    assert got.tobytes() == ref32.tobytes(), label
    return fig


# ---- primary ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(G.primary_cases()))
def test_primary(ctx, name):
    cam, first, n = G.primary_cases()[name]
    got = generate(ctx, n, lambda d: ctx.generate_primary(cam, d, first, n))
    assert (bits(got["t"]) == bits(G.FAR)).all()
    hold(got, G.primary_f32(cam, first, n), G.primary_f64(cam, first, n), "primary " + name)
    if name == "odd_slice":      # the same slice of the image generated whole
        total = cam.width * cam.height * cam.spp_x * cam.spp_y
        whole = generate(ctx, total, lambda d: ctx.generate_primary(cam, d, 0, total))
        assert got.tobytes() == whole[first:first + n].tobytes()
    if name == "symmetric":      # the sample column at u = 1/2: D.x == 0 exactly, rD.x = +1e30; the row at v = 1/2 likewise in y
        nu, nv = G.pixel_map(cam.width, cam.height, cam.spp_x, cam.spp_y, first, n)
        col, row = nu == cam.width * cam.spp_x // 2, nv == cam.height * cam.spp_y // 2
        assert col.sum() == cam.height * cam.spp_y and row.sum() == cam.width * cam.spp_x
        assert (got["D"][col, 0] == 0).all() and (bits(got["rD"][col, 0]) == bits(G.FAR)).all() and (got["D"][~col, 0] != 0).all()
        assert (got["D"][row, 1] == 0).all() and (bits(got["rD"][row, 1]) == bits(G.FAR)).all()
    if name == "negative_zero":
        assert bits(got["D"][0, 0]) == 0x80000000 and bits(got["rD"][0, 0]) == bits(G.FAR)


@pytest.mark.parametrize("width,height,spp_x,spp_y", [(0, 32, 2, 2), (64, 0, 2, 2), (0, 0, 1, 1), (6, 32, 2, 2), (64, 30, 2, 2), (64, 32, 0, 2), (64, 32, 2, 0)])
def test_primary_refuses_bad_cameras(ctx, width, height, spp_x, spp_y):
    cam = G.oblique_camera(width, height, spp_x, spp_y)

    def call(d):
        with pytest.raises(tb.TbvhError) as e:
            ctx.generate_primary(cam, d, 0, 256)
        assert e.value.code == INVALID
    out = generate(ctx, 256, call)
    assert (out.view(np.uint8) == POISON).all()       # nothing was launched
    good, first, n = G.primary_cases()["spp1x1"]
    got = generate(ctx, n, lambda d: ctx.generate_primary(good, d, first, n))
    assert got.tobytes() == G.primary_f32(good, first, n).tobytes()


# ---- bounce and shadow: inputs traced on the device ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def traced(ctx):
    """name -> (verts, device copy of verts, the primary batch of G.TRACED_VIEWS[name] after scene.Intersect)"""
    out, scenes = {}, []
    for name in G.TRACED_VIEWS:
        verts = np.ascontiguousarray(np.load(os.path.join(GOLDEN, name + ".npz"))["verts"], F)
        sc = tb.BVH8_CWBVH(ctx).Build(verts, threads=1)
        rec = sc.Intersect(G.traced_view_rays(name))
        d_verts = ctx.malloc(verts.nbytes)
        ctx.to_device(d_verts, verts)
        out[name] = (verts, d_verts, rec)
        scenes.append(sc)
    yield out
    for sc in scenes:
        sc.free()
    for _, d_verts, _ in out.values():
        ctx.free(d_verts)


def device_bounce(ctx, d_verts, rec, seed, in_place=False, lead=0):
    n = rec.shape[0]
    if in_place:
        return generate(ctx, n, lambda d: ctx.generate_bounce(d_verts, d, d, n, seed), prefill=rec, lead=lead)
    d_in = ctx.malloc(n * 64)
    try:
        ctx.to_device(d_in, rec)
        return generate(ctx, n, lambda d: ctx.generate_bounce(d_verts, d_in, d, n, seed), lead=lead)
    finally:
        ctx.free(d_in)


@pytest.mark.parametrize("seed", G.BOUNCE_SEEDS)
@pytest.mark.parametrize("name", list(G.TRACED_VIEWS))
def test_bounce(ctx, traced, name, seed):
    verts, d_verts, rec = traced[name]
    hit = rec["t"] < G.FAR
    assert 0.2 < hit.mean() < 0.95       # hits and misses mixed
    got = device_bounce(ctx, d_verts, rec, seed)
    assert (bits(got["t"]) == bits(G.FAR)).all()
    ref64 = G.bounce_f64(rec, verts, seed)
    hold(got, G.bounce_f32(rec, verts, seed), ref64, f"bounce {name} seed {seed}")
    # the construction itself, on the device's output: a bounce leaves on the side its ray came from (triangles seen from behind included),
    # and no two rays of the batch share a direction
    D_in = rec["D"].astype(np.float64)
    N = G._tri_normal64(verts, np.where(hit, rec["prim"], 0))
    behind = (N * D_in).sum(1) > 0
    assert (behind & hit).sum() > 100 and (name != "soup_2k" or (~behind & hit).sum() > 100)     # (the atrium's floor is seen from one side only)
    front = np.where(behind[:, None], -N, N)
    assert ((front * got["D"]).sum(1)[hit & ~ref64["knife"]] >= -1e-6).all()
    assert len(np.unique(bits(got["D"]), axis=0)) == rec.shape[0]


def test_bounce_seeds_repeats_and_in_place(ctx, traced):
    verts, d_verts, rec = traced["soup_2k"]
    a, b = G.BOUNCE_SEEDS
    out_a = device_bounce(ctx, d_verts, rec, a)
    assert device_bounce(ctx, d_verts, rec, a).tobytes() == out_a.tobytes()                     # the same seed: the same bytes
    assert (bits(device_bounce(ctx, d_verts, rec, b)["D"]) != bits(out_a["D"])).any(axis=1).mean() > 0.999   # another seed: another batch
    assert device_bounce(ctx, d_verts, rec, a, in_place=True).tobytes() == out_a.tobytes()      # d_out == d_in
    # in place at an offset into a larger buffer, as the benchmark bounces the tail of its batch: the stream follows the index within the call
    k = 4097
    tail = device_bounce(ctx, d_verts, rec[k:], a, in_place=True, lead=k)
    assert tail.tobytes() == device_bounce(ctx, d_verts, rec[k:], a).tobytes()
    assert tail.tobytes() == G.bounce_f32(rec[k:], verts, a).tobytes()
    assert tail.tobytes() != out_a[k:].tobytes()


def device_shadow(ctx, rec, light, eps):
    n = rec.shape[0]
    d_in = ctx.malloc(n * 64)
    try:
        ctx.to_device(d_in, rec)
        return generate(ctx, n, lambda d: ctx.generate_shadow(d_in, d, n, light, eps))
    finally:
        ctx.free(d_in)


@pytest.mark.parametrize("eps", [G.SHADOW_EPS, 0.0])
@pytest.mark.parametrize("name", list(G.TRACED_VIEWS))
def test_shadow(ctx, traced, name, eps):
    _, _, rec = traced[name]
    hit = rec["t"] < G.FAR
    assert hit.any() and (~hit).any()
    got = device_shadow(ctx, rec, G.SHADOW_LIGHT, eps)
    ref64 = G.shadow_f64(rec, G.SHADOW_LIGHT, eps)
    hold(got, G.shadow_f32(rec, G.SHADOW_LIGHT, eps), ref64, f"shadow {name} eps {eps}")
    # misses start 1000 along the ray, not 1e30
    far = rec["O"].astype(np.float64) + 1000.0 * rec["D"].astype(np.float64)
    assert (np.abs(got["O"] - far)[~hit] < 1e-3).all()


@pytest.mark.parametrize("eps", [G.SHADOW_EPS, 0.0])
def test_shadow_light_on_the_hit_point(ctx, traced, eps):
    """dist == 0: D = 0, rD = +1e30, t = -eps and no NaN anywhere; the record's neighbours are ordinary rays.  O + t D is exact for the
    hand-made record (1, 2, 3) + 2 (0, 0, 1), so the light at (1, 2, 5) lies on it whatever the rounding."""
    _, _, rec = traced["soup_2k"]
    rec = rec[:129].copy()
    rec[64] = tb.make_rays(np.array([[1.0, 2.0, 3.0]], F), np.array([[0.0, 0.0, 1.0]], F))[0]
    rec["t"][64] = 2.0
    light = (1.0, 2.0, 5.0)
    got = device_shadow(ctx, rec, light, eps)
    hold(got, G.shadow_f32(rec, light, eps), G.shadow_f64(rec, light, eps), f"shadow on the light eps {eps}")
    r = got[64]
    assert r["O"].tolist() == [1.0, 2.0, 5.0] and bits(r["D"]).tolist() == [0, 0, 0]
    assert (bits(r["rD"]) == bits(G.FAR)).all() and bits(r["t"]) == bits(F(0) - F(eps))
