"""The device-resident path tracer held to a reference path by path: the queues Generate, Shade and Connect leave behind (Wavefront.debug_queues) against
tests/wavefront_ref.py evaluated on the device's own float32 records, every float within the bound the reference derives for it, everything that involves no
arithmetic bitwise; Extend and Connect against the oracle; the accumulator against the per-pixel sum of the contributions.  Stage d's bounce rays are read after a
render with max_depth d + 2, its shadow rays after one with max_depth d + 1 (include/tinybvh_amd_debug.h), so each case is a handful of single-frame renders."""
import numpy as np
import pytest

import tinybvh_amd as tb
import wavefront_ref as wr
import wavefront_scenes as ws
from oracle_lib import compare_hits

pytestmark = pytest.mark.gpu

WORST = {}          # field -> worst observed error / bound over the module (printed per test; a ratio above 1 fails where it is found)


def note(field, ratio):
    WORST[field] = max(WORST.get(field, 0.0), float(ratio))


# ---- a scene on the device, with what the oracle needs --------------------------------------------------------------------------

class Device:
    def __init__(self, ctx, scene, layout=tb.LAYOUT_CWBVH):
        self.ctx, self.scene, self.bufs = ctx, scene, []
        if isinstance(scene, ws.TwoLevel):
            self.blas = [tb.LAYOUT_CLASSES[l](ctx).Build(v) for l, v in zip(scene.layouts, scene.blas_verts)]
            self.sc = tb.TLAS(ctx).Build(scene.instances, self.blas)          # (fills invTransform and the bounds of scene.instances, as the host build did)
            scene.host = self.sc.host
            self.d_verts = 0
            self.blas_ptrs = [self.upload(v) for v in scene.blas_verts]
        else:
            self.sc = tb.LAYOUT_CLASSES[layout](ctx).Build(scene.verts)
            scene.host = self.sc.host                                         # the BVH2 this device tree was made from
            self.d_verts = self.upload(scene.verts)
        self.wfs = {}

    def upload(self, a):
        d = self.ctx.malloc(a.nbytes); self.ctx.to_device(d, a); self.bufs.append(d)
        return d

    def wavefront(self, W, H, band=None):
        key = (W, H, band)
        if key not in self.wfs:
            wf = tb.Wavefront(self.ctx, W, H)
            if band:
                wf.set_band(*band)
            if isinstance(self.scene, ws.TwoLevel):
                wf.set_blas_vertices(self.blas_ptrs)
            self.wfs[key] = wf
        return self.wfs[key]

    def frame(self, cam, kw, K, seed, band=None, rows=None):
        """One cleared frame: (stats, accumulator (pixels, 3) float64, queues)."""
        wf = self.wavefront(int(cam.width), rows or int(cam.height), band)
        kw = dict(kw)
        wf.set_blue_noise(kw.pop("blue_noise", None))
        st = wf.render(self.sc, self.d_verts, cam, max_depth=K, seed=seed, **kw)
        q = wf.debug_queues()
        return st, wf.read().reshape(-1, 4)[:, :3].astype(np.float64), q

    def close(self):
        for wf in self.wfs.values():
            wf.close()
        for d in self.bufs:
            self.ctx.free(d)
        self.sc.free()
        for b in getattr(self, "blas", []):
            b.free()


# ---- comparisons ------------------------------------------------------------------------------------------------------------------

def ratio(dev, ref):
    """|device - reference| / bound, elementwise; where the bound is 0 the values must be equal (0 or inf)."""
    v, e = ref
    d = np.abs(np.asarray(dev, np.float64) - v)
    e = np.broadcast_to(e, v.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(e > 0, d / np.where(e > 0, e, 1.0), np.where(d == 0, 0.0, np.inf))


def check_record_words(rays, what):
    """What involves no arithmetic, bitwise: O.w = 0xFFFF, rD = 1 / D of the device's OWN D (correctly rounded division; +-1e30 inside the 1e-12 window)."""
    assert (rays["mask"] == 0xFFFF).all(), what
    assert np.array_equal(rays["rD"].view(np.uint32), tb.safercp(rays["D"]).view(np.uint32)), what


def check_generate(q, cam, seed, first_row=0, rows=None):
    g = wr.generate(cam, seed, first_row, rows)
    n = g["n"]
    assert q["path_counts"][0] == n
    rays, aux = q["rays"][0][:n], q["aux"][0][:n]
    check_record_words(rays, "generate")
    assert np.array_equal(rays["O"].view(np.uint32), np.broadcast_to(g["O"], (n, 3)).view(np.uint32))
    assert np.array_equal(aux["pixel"], g["word"]) and (aux["T"] == 1.0).all() and (rays["instIdx"] == np.float32(1.0).view(np.uint32)).all()
    assert np.unique(aux["pixel"]).size == n
    r = np.stack([ratio(rays["D"][:, k], (g["D"][k].v, g["D"][k].e)) for k in range(3)], -1)
    note("generate D", r.max())
    assert r.max() <= 1.0, r.max()


def check_extend(scene, orc, rays):
    """The hit records Extend left in a path queue against the oracle on the same rays, under the rule of tests/test_gpu_parity.py."""
    if rays.shape[0] == 0:
        return
    fresh = rays.copy()
    fresh["t"] = np.float32(1e30); fresh["u"] = 0; fresh["v"] = 0; fresh["prim"] = 0; fresh["inst"] = 0
    want = scene.intersect(orc, fresh)
    c = compare_hits(rays, want, rtol=1e-5)
    assert c["hitmiss"] == 0 and c["prim_real"] == 0 and c["t_bad"] == 0 and c["uv_bad"] == 0 and c["tie"] == 0, c
    assert c["onsurf"] <= max(4, c["n"] // 5000), c
    assert c["bit_identical"] == c["same_prim"], c
    if isinstance(scene, ws.TwoLevel):
        h = (rays["t"] < np.float32(1e30)) & (rays["prim"] == want["prim"])
        assert np.array_equal(rays["inst"][h], want["inst"][h])


def check_connect(scene, orc, shadow, occ):
    """Connect's any-hit flags of the device's own shadow rays against the oracle: equal, ray by ray."""
    if shadow.shape[0]:
        want = scene.occluded(orc, shadow)
        assert np.array_equal(occ, want), int((occ != want).sum())


def by_pixel(pixels, n_pixels, what):
    """slot[pixel] of a queue's entries (-1: none); a pixel occurs at most once per queue."""
    assert np.unique(pixels).size == pixels.size, what
    slot = np.full(n_pixels, -1, np.int64)
    slot[pixels] = np.arange(pixels.size)
    return slot


def compare_queue(ref, kind, rays, aux, n_pixels, worst):
    """Per path of the stage: does the device's queue hold (or not hold) what the reference says, every field within its bound?"""
    bounce = kind == "bounce"
    pix = (aux["pixel"] >> np.uint32(8)) if bounce else aux["pixel"]
    slot = by_pixel(pix.astype(np.int64), n_pixels, kind)
    s = slot[ref["pixel"]]
    assert (s >= 0).sum() == pix.size, f"{kind}: entries of pixels no live path has"
    want = ref["want_" + kind]
    ok = (s >= 0) == want
    both = np.flatnonzero((s >= 0) & want)
    k = s[both]
    sub = lambda f: (ref[f][0][both], ref[f][1][both])
    fields = {"O": ratio(rays["O"][k], sub(kind + "_O")).max(1) if both.size else np.zeros(0), "D": ratio(rays["D"][k], sub(kind + "_D")).max(1) if both.size else np.zeros(0)}
    if bounce:
        fields["pdf"] = ratio(rays["instIdx"][k].view(np.float32), sub("bounce_pdf"))
        fields["T"] = ratio(aux["T"][k], sub("bounce_T")).max(1) if both.size else np.zeros(0)
        exact = aux["pixel"][k] == ref["bounce_word"][both]
    else:
        fields["tmax"] = ratio(rays["t"][k], sub("shadow_tmax"))
        fields["contribution"] = ratio(aux["T"][k], sub("contrib")).max(1) if both.size else np.zeros(0)
        exact = rays["instIdx"][k] == np.float32(1.0).view(np.uint32)
    good = exact.copy()
    for name, r in fields.items():
        good &= r <= 1.0
        worst.setdefault(kind + " " + name, []).append((both, r))
    ok[both] &= good
    return ok


def check_shade(rays_in, aux_in, geo, P, d, shadow=None, bounce=None):
    """One Shade stage: its input (live entries, with Extend's hit records) through the reference; the shadow queue and / or the bounce queue it wrote, matched
    by pixel.  A path undecided at this stage may have gone either way on its undecided decisions, but must match the reference on that side.  Returns the
    reference's output (on the side the device took) and the number of undecided paths."""
    n_pixels = P.width * P.height
    ref = wr.shade(rays_in, aux_in, geo, P, d)
    assert np.unique(ref["pixel"]).size == ref["n"]

    def compare(r, worst):
        ok = np.ones(r["n"], bool)
        if shadow is not None:
            ok &= compare_queue(r, "shadow", shadow[0], shadow[1], n_pixels, worst)
        if bounce is not None:
            ok &= compare_queue(r, "bounce", bounce[0], bounce[1], n_pixels, worst)
        return ok

    worst = {}
    ok = compare(ref, worst)
    und = ref["undecided"]
    assert ok[und == 0].all(), (f"stage {d}: {int((~ok & (und == 0)).sum())} decided paths differ", {k: max((float(r.max()) for _, r in v if r.size), default=0.0) for k, v in worst.items()})
    for name, lst in worst.items():      # the worst error / bound over the decided paths
        for both, r in lst:
            m = und[both] == 0
            if m.any():
                note(name, r[m].max())
    bad = ~ok
    side = np.zeros(ref["n"], np.int64)
    for mask in range(1, 64):
        if not bad.any():
            break
        flip = np.where(bad & ((mask & ~und) == 0), mask, 0)
        if not flip.any():
            continue
        alt = wr.shade(rays_in, aux_in, geo, P, d, flip=flip)
        got = compare(alt, {}) & (flip != 0)
        side[got] = mask
        bad &= ~got
    assert not bad.any(), f"stage {d}: {int(bad.sum())} undecided paths match the reference on neither side"
    if side.any():
        ref = wr.shade(rays_in, aux_in, geo, P, d, flip=side)
    return ref, int((und != 0).sum())


def live_pair(q, which, count):
    return q["rays"][which][:count], q["aux"][which][:count]


class Accumulator:
    """The per-pixel sums the images must follow: image(K) - image(K - 1) = stage K - 1's terminal contributions + its unoccluded shadow contributions, within
    the bound of the contributions themselves plus half an ulp of the running sum per float addition into the pixel, for both images."""

    def __init__(self, n_pixels):
        self.count = np.zeros(n_pixels); self.mag = np.zeros((n_pixels, 3)); self.prev_img = np.zeros((n_pixels, 3)); self.prev_err = np.zeros((n_pixels, 3))

    def stage(self, img, ref, shadow_aux, occ):
        n_pixels = img.shape[0]
        want = np.zeros((n_pixels, 3)); err = np.zeros((n_pixels, 3))
        t = ref["terminal"]
        np.add.at(want, ref["pixel"][t], ref["term"][0][t]); np.add.at(err, ref["pixel"][t], ref["term"][1][t])
        np.add.at(self.count, ref["pixel"][t], 1); np.add.at(self.mag, ref["pixel"][t], np.abs(ref["term"][0][t]) + ref["term"][1][t])
        lit = occ == 0
        c = shadow_aux["T"][lit].astype(np.float64); p = shadow_aux["pixel"][lit].astype(np.int64)
        np.add.at(want, p, c); np.add.at(self.count, p, 1); np.add.at(self.mag, p, np.abs(c))
        add_err = wr.U * np.maximum(self.count - 1, 0)[:, None] * self.mag
        bound = err + add_err + self.prev_err
        diff = np.abs(img - self.prev_img - want)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(bound > 0, diff / np.where(bound > 0, bound, 1.0), np.where(diff == 0, 0.0, np.inf))
        note("accumulator", r.max())
        assert r.max() <= 1.0, (r.max(), int((r > 1).sum()))
        self.prev_img, self.prev_err = img, add_err


def check_frames(dev, orc, cam, kw, seed, depth):
    """Renders with max_depth = 1 .. depth over one seed, each checked stage by stage.  Returns per stage the reference's output for the render in which the
    stage was the last ("ref"), for the one in which it wrote bounce rays ("ref_bounce"), and the device's occlusion flags; and the number of undecided paths met."""
    scene = dev.scene
    W, H = int(cam.width), int(cam.height)
    n = W * H
    acc = Accumulator(n)
    stages, undecided = [], 0
    for K in range(1, depth + 1):
        P = wr.Params(max_depth=K, seed=seed, width=W, height=H, **kw)
        st, img, q = dev.frame(cam, kw, K, seed)
        pc, sc = q["path_counts"], q["shadow_counts"]
        assert st["extend_rays"] == pc[:K] and st["shadow_rays"] == sc[:K]
        assert pc[0] == n and all(pc[d + 1] <= pc[d] for d in range(K)) and pc[K] == 0
        if K == 1:
            check_generate(q, cam, seed)
        last = (K - 1) & 1
        rays_in, aux_in = live_pair(q, last, pc[K - 1])
        check_record_words(rays_in, f"path queue of stage {K - 1}")
        check_extend(scene, orc, rays_in)
        shadow = (q["shadow"][:sc[K - 1]], q["shadow_aux"][:sc[K - 1]])
        occ = q["occ"][:sc[K - 1]]
        check_record_words(shadow[0], f"shadow queue of stage {K - 1}")
        check_connect(scene, orc, shadow[0], occ)
        ref, u = check_shade(rays_in, aux_in, scene.geo, P, K - 1, shadow=shadow)
        undecided += u
        if u == 0:
            assert sc[K - 1] == int(ref["want_shadow"].sum())
        if K >= 2:   # the stage before: its input is intact in the other buffer, its bounce rays are the last stage's input
            prev_in = live_pair(q, last ^ 1, pc[K - 2])
            refb, ub = check_shade(prev_in[0], prev_in[1], scene.geo, P, K - 2, bounce=(rays_in, aux_in))
            if ub == 0:
                assert pc[K - 1] == int(refb["want_bounce"].sum())
            stages[K - 2]["ref_bounce"] = refb
        acc.stage(img, ref, shadow[1], occ)
        stages.append({"ref": ref, "occ": occ})
    return stages, undecided


def report(name):
    print(f"[{name}] worst error / bound so far:", {k: round(v, 4) for k, v in sorted(WORST.items())})


def frame_queues(q, depth):
    """Everything debug_queues defines after a render of `depth` stages, order-free: the counters, the inputs of the last two stages, the shadow queue, its flags."""
    pc, sc = q["path_counts"], q["shadow_counts"]
    out = [pc, sc, queue_set(*live_pair(q, (depth - 1) & 1, pc[depth - 1]))]
    if depth >= 2:
        out.append(queue_set(*live_pair(q, (depth - 2) & 1, pc[depth - 2])))
    ns = sc[depth - 1]
    o = np.argsort(q["shadow_aux"]["pixel"][:ns], kind="stable")
    return out + [queue_set(q["shadow"][:ns], q["shadow_aux"][:ns]), q["occ"][:ns][o].tobytes()]


def queue_set(rays, aux):
    """A queue's live entries as a set: sorted by the aux word (unique per queue), as raw bytes."""
    o = np.argsort(aux["pixel"], kind="stable")
    return rays[o].tobytes(), aux[o].tobytes()


# ---- Scene A ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dev_a(ctx):
    scene = ws.SingleLevel(ws.scene_a_verts())
    d = Device(ctx, scene)
    yield d
    d.close()


@pytest.mark.parametrize("layout", [tb.LAYOUT_CWBVH, tb.LAYOUT_BVH_GPU], ids=["cwbvh", "bvh_gpu"])
def test_scene_a_stage_by_stage(ctx, oracle, dev_a, layout):
    """Stages 0 .. 3 of the room: Generate, Extend, Shade (shadow and bounce output), Connect, the accumulator and the statistics; every branch of Shade is taken."""
    scene, cam, kw, depth, seed = ws.CASES["scene_a"]()
    dev = dev_a if layout == tb.LAYOUT_CWBVH else Device(ctx, scene, layout)
    try:
        stages, und = check_frames(dev, oracle, cam, kw, seed, depth)
        c = ws.classes(stages)
        print("classes", c, "undecided", und)
        assert all(v > 0 for k, v in c.items() if k != "one_bounce_stop"), c
        r0 = stages[0]["ref"]
        assert r0["miss"].any() and r0["emitter"].any() and r0["specular"].any() and r0["diffuse"].any()
    finally:
        if dev is not dev_a:
            dev.close()
    report("scene a")


def test_one_diffuse_bounce_ends_paths_at_the_second_diffuse_vertex(oracle, dev_a):
    scene, cam, kw, depth, seed = ws.CASES["scene_a_one_bounce"]()
    stages, _ = check_frames(dev_a, oracle, cam, kw, seed, depth)
    c = ws.classes(stages)
    stops = [int(s["ref_bounce"]["stopped"].sum()) for s in stages[:-1]]
    assert stops[0] == 0 and stops[1] > 500 and stops[2] > 0, stops
    assert c["diffuse_mirror_diffuse"] > 0, c                                       # ... and a mirror in between clears PATH_VIA_DIFFUSE: such a path goes on
    report("one diffuse bounce")


def test_mirror_chain_to_depth_8_and_the_clamps_of_max_depth(oracle, dev_a):
    """Two facing mirrors carry specular paths to the last stage a frame can have: the depth nibble, PATH_LAST_SPECULAR and the throughput after seven mirrors.
    max_depth 9 is 8, max_depth 0 is 3: the same counters and the same queues."""
    scene, cam, kw, depth, seed = ws.CASES["scene_a_chain"]()
    W, H = int(cam.width), int(cam.height)
    P = wr.Params(max_depth=8, seed=seed, width=W, height=H, **kw)
    st, img, q = dev_a.frame(cam, kw, 8, seed)
    pc, sc = q["path_counts"], q["shadow_counts"]
    assert st["extend_rays"] == pc[:8] and st["shadow_rays"] == sc[:8] and pc[8] == 0
    rays7, aux7 = live_pair(q, 1, pc[7])
    rays6, aux6 = live_pair(q, 0, pc[6])
    assert ((aux7["pixel"] >> np.uint32(4)) & 15 == 7).all() and ((aux6["pixel"] >> np.uint32(4)) & 15 == 6).all()
    chain = (aux7["pixel"] & 15) == wr.PATH_LAST_SPECULAR
    assert chain.sum() > 0
    check_extend(dev_a.scene, oracle, rays7)
    shadow = (q["shadow"][:sc[7]], q["shadow_aux"][:sc[7]])
    check_connect(dev_a.scene, oracle, shadow[0], q["occ"][:sc[7]])
    ref7, u7 = check_shade(rays7, aux7, dev_a.scene.geo, P, 7, shadow=shadow)
    ref6, u6 = check_shade(rays6, aux6, dev_a.scene.geo, P, 6, bounce=(rays7, aux7))
    assert not ref7["want_bounce"].any()
    if u7 == 0:
        assert sc[7] == int(ref7["want_shadow"].sum())
    if u6 == 0:
        assert pc[7] == int(ref6["want_bounce"].sum())
    for K, same_as in ((9, 8), (0, 3)):
        sa, _, qa = dev_a.frame(cam, kw, K, seed)
        sb, _, qb = dev_a.frame(cam, kw, same_as, seed)
        assert frame_queues(qa, same_as) == frame_queues(qb, same_as)
        if K == 9:
            assert sa["extend_rays"][:8] == sb["extend_rays"] and sa["shadow_rays"][:8] == sb["shadow_rays"]
    report("mirror chain")


def test_point_light(oracle, dev_a):
    scene, cam, kw, depth, seed = ws.CASES["scene_a_point_light"]()
    stages, _ = check_frames(dev_a, oracle, cam, kw, seed, depth)
    assert stages[0]["ref"]["want_shadow"].sum() > 1000 and not stages[1]["ref"]["mis_light"].any()      # no MIS without an area
    report("point light")


def test_reference_letter_switches_each_show(oracle, dev_a):
    """TBVH_WF_REFERENCE_LETTER changes three places; each is seen by a checked field: the bounce direction (tools.cl's half sphere: the bounce queue), the sky
    after a diffuse bounce without the postponed pdf and the emitter reached by a bounce at weight 0 (both: the accumulator)."""
    scene, cam, kw, depth, seed = ws.CASES["scene_a_letter"]()
    stages, _ = check_frames(dev_a, oracle, cam, kw, seed, depth)
    later = stages[1:]
    assert sum(int((s["ref"]["miss"] & ((s["ref"]["flags"] & wr.PATH_VIA_DIFFUSE) != 0)).sum()) for s in later) > 0
    assert sum(int(s["ref"]["mis_light"].sum()) for s in later) > 0
    for s in later:   # an emitter found by a bounce adds nothing
        assert (s["ref"]["term"][0][s["ref"]["mis_light"]] == 0).all()
    # the checks can tell the two modes apart: the same stage-0 input through the default shading gives other bounce rays, and another sky weight
    W, H = int(cam.width), int(cam.height)
    st, img, q = dev_a.frame(cam, kw, 2, seed)
    pc = q["path_counts"]
    plain = wr.shade(*live_pair(q, 0, pc[0]), dev_a.scene.geo, wr.Params(max_depth=2, seed=seed, width=W, height=H, **dict(kw, reference_letter=False)), 0)
    assert (~compare_queue(plain, "bounce", *live_pair(q, 1, pc[1]), W * H, {})).sum() > 1000
    report("reference letter")


@pytest.mark.parametrize("case", ["scene_a_blue_0", "scene_a_blue_3", "scene_a_blue_4", "scene_a_blue_off"])
def test_blue_noise(oracle, dev_a, case):
    """A seeded table on a non-square image: sample_index 0 and 3 take page pairs (0, 1) and (6, 7) at x = pixel % height, y = pixel / height for the first
    vertex — the first word to the light sample, the second to the bounce —; 4 and 0xFFFFFFFF take the RNG."""
    scene, cam, kw, depth, seed = ws.CASES[case]()
    stages, _ = check_frames(dev_a, oracle, cam, kw, seed, depth)
    assert stages[0]["ref"]["want_shadow"].sum() > 1000 and stages[0]["ref_bounce"]["want_bounce"].sum() > 1000
    report(case)


@pytest.mark.parametrize("case", ["scene_a", "scene_a_blue_0"])
def test_band_rendered_alone_repeats_the_full_image(oracle, dev_a, case):
    """Rows 20 .. 35 of the 72 x 52 image as an object of their own: the queues are the full image's entries for those rows bit for bit (the RNG and the blue
    noise are keyed by the pixel's index in the FULL image), with the band's own pixel numbering in the aux words; the accumulator follows within the add order."""
    scene, cam, kw, depth, seed = ws.CASES[case]()
    W, H, first, rows = int(cam.width), int(cam.height), 20, 16
    off = first * W
    for K in (1, 2):
        stf, imgf, qf = dev_a.frame(cam, kw, K, seed)
        stb, imgb, qb = dev_a.frame(cam, kw, K, seed, band=(first, H), rows=rows)
        if K == 1:
            check_generate(qb, cam, seed, first, rows)
        for w in range(K):
            d = w                                                   # buffer w holds the input of stage w for K <= 2
            rf, af = live_pair(qf, w, qf["path_counts"][d]); rb, ab = live_pair(qb, w, qb["path_counts"][d])
            pf = (af["pixel"] >> np.uint32(8)).astype(np.int64)
            m = (pf >= off) & (pf < off + rows * W)
            af_local = af[m].copy(); af_local["pixel"] = ((pf[m] - off).astype(np.uint32) << np.uint32(8)) | (af["pixel"][m] & np.uint32(255))
            assert m.sum() == rb.shape[0] and queue_set(rf[m], af_local) == queue_set(rb, ab), (K, w)
        ns_f, ns_b = qf["shadow_counts"][K - 1], qb["shadow_counts"][K - 1]
        sf, saf = qf["shadow"][:ns_f], qf["shadow_aux"][:ns_f]
        m = (saf["pixel"] >= off) & (saf["pixel"] < off + rows * W)
        saf_local = saf[m].copy(); saf_local["pixel"] -= np.uint32(off)
        assert m.sum() == ns_b and queue_set(sf[m], saf_local) == queue_set(qb["shadow"][:ns_b], qb["shadow_aux"][:ns_b]), K
        assert np.array_equal(qf["occ"][:ns_f][m][np.argsort(saf_local["pixel"])], qb["occ"][:ns_b][np.argsort(qb["shadow_aux"]["pixel"][:ns_b])])
        # the same contributions in another order: at most K additions per pixel (one terminal or shadow contribution per stage), the first of them exact, each
        # other half an ulp of a partial sum, which is at most the final one (contributions are non-negative) — in each of the two images
        part = imgf[off:off + rows * W]
        bound = 2 * wr.U * (K - 1) * np.maximum(part, imgb) * (1 + 2.0 ** -20)
        assert (part >= 0).all() and (np.abs(part - imgb) <= bound).all()


def test_the_same_render_twice_gives_the_same_queues(dev_a):
    scene, cam, kw, depth, seed = ws.CASES["scene_a"]()
    a, b = dev_a.frame(cam, kw, 3, seed)[2], dev_a.frame(cam, kw, 3, seed)[2]
    assert frame_queues(a, 3) == frame_queues(b, 3)


# ---- Scene B: instances -----------------------------------------------------------------------------------------------------------

def test_scene_b_through_instances(ctx, oracle):
    """Diffuse and mirror BLASes of three layouts under non-uniform scales, rotations and a mirrored instance: the triangle comes from the instance's BLAS (byte
    44 of the hit record names the instance), the normal goes through the transposed inverse; next event estimation and bounces leave instanced diffuse surfaces."""
    scene, cam, kw, depth, seed = ws.CASES["scene_b"]()
    dev = Device(ctx, scene)
    try:
        assert np.linalg.det(scene.instances["transform"][2].reshape(4, 4)[:3, :3]) < 0
        stages, _ = check_frames(dev, oracle, cam, kw, seed, depth)
        r0 = stages[0]["ref"]
        inst0 = dev.frame(cam, kw, 1, seed)[2]["rays"][0]["inst"][: r0["n"]]
        for i in (1, 2):      # the scaled and the mirrored ball: shadow and bounce rays start there
            on = ~r0["miss"] & (inst0 == i)
            assert (on & r0["want_shadow"]).sum() > 20, i
        assert (~r0["miss"] & (inst0 == 3) & r0["specular"]).sum() > 20
        assert stages[1]["ref"]["n"] > 500 and stages[2]["ref"]["n"] > 100
    finally:
        dev.close()
    report("scene b")


# ---- two scripted edges -----------------------------------------------------------------------------------------------------------

def test_grazing_light_and_the_solid_angle_clamp(ctx, oracle):
    scene, cam, kw, depth, seed = ws.CASES["grazing"]()
    dev = Device(ctx, scene)
    try:
        stages, _ = check_frames(dev, oracle, cam, kw, seed, depth)
        r = stages[0]["ref"]
        L = r["shadow_D"][0][r["want_shadow"]]
        dist = r["shadow_tmax"][0][r["want_shadow"]] + 0.002
        assert (np.abs(L[:, 1]) < 0.01).sum() > 100 and (45.0 / dist ** 2 * np.abs(L[:, 1]) > wr.TWO_PI).sum() > 0
    finally:
        dev.close()
    report("grazing")


def test_no_shadow_ray_closer_to_the_point_light_than_two_eps(ctx, oracle):
    scene, cam, kw, depth, seed = ws.CASES["near_point_light"]()
    dev = Device(ctx, scene)
    try:
        stages, _ = check_frames(dev, oracle, cam, kw, seed, depth)
        r = stages[0]["ref"]
        assert 0 < (r["diffuse"] & ~r["want_shadow"]).sum() < r["n"] // 4 and not r["ndl_rejected"].any()
    finally:
        dev.close()
    report("near point light")
