"""Shade pinned to the reference: the reference's OWN wavefront.cl — Generate, { Extend, Shade } x 3, Connect,
run through ROCm OpenCL by oracle/ref_ocl.cpp exactly as tiny_bvh_gpu.cpp:128-158 drives it — and this library's
device-resident path tracer in TBVH_WF_REFERENCE_LETTER mode render the same scene (Sponza stand-in + the demo's 9 x 5 light
quad at (-22, 12, 2), tiny_bvh_gpu.cpp:93-94) from the same camera with the same blue-noise table; the converged images must
agree: mean relative difference of 8 x 8-pixel block averages below 1 %.  The two sides use different random streams, so
the comparison is statistical; 8 x 8 blocks of a 512-sample image carry ~0.3 % noise."""
import os

import numpy as np
import pytest

import tinybvh_amd as tb
from tinybvh_amd import rays as R
from tinybvh_amd import scenes
from oracle_lib import REFOCL_PATH, ReferenceOpenCL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def u2f(u):
    return np.frombuffer(np.array([u], np.uint32).tobytes(), np.float32)[0]


def demo_scene():
    verts = scenes.atrium(40_000, seed=1)
    verts[:, 3] = u2f(0x00C0C0C0)                                    # AddMesh( ..., c ): the colour goes into every w (tiny_bvh_gpu.cpp:48-49)
    # AddQuad( (-22, 12, 2), 9, 5, 0x1ffffff ): the light source as geometry (tiny_bvh_gpu.cpp:51-59, 94)
    w, d, pos = 9.0, 5.0, np.array([-22.0, 12.0, 2.0], np.float32)
    q = np.array([[-w, 0, -d], [w, 0, -d], [w, 0, d], [-w, 0, -d], [w, 0, d], [-w, 0, d]], np.float32) * 0.5 + pos
    quad = np.zeros((6, 4), np.float32); quad[:, :3] = q; quad[:, 3] = u2f(0x01FFFFFF)
    return np.ascontiguousarray(np.concatenate([quad, verts]))


def blue_noise():
    # the table of the reference's blue_noise_128x128x8_2d.raw in size and type, seeded: any table serves, both sides get the same one
    return np.random.default_rng(5).integers(0, 1 << 32, 128 * 128 * 8, dtype=np.uint64).astype(np.uint32)


def blocks(img, b=8):
    h, w = img.shape[:2]
    return img[..., :3].reshape(h // b, b, w // b, b, 3).mean((1, 3))


# Connect deposits a shadow ray's contribution with a plain read-modify-write (wavefront.cl:272: accumulator[pixel] += T4).  Two
# shadow rays of one pixel (first and second path vertex) are in flight together in the single Connect launch, and on this
# OpenCL stack the earlier contribution is lost almost every time (measured on MI355X, light only: next-event estimation at
# the first vertex alone 0.0164, at the second alone 0.0400, both 0.0393 instead of 0.0564).  This library accumulates with
# atomicAdd.  For the full-pipeline comparison the test compiles the reference's kernel with that ONE statement made atomic;
# the unpatched reference is compared where the race cannot happen (one iteration: at most one shadow ray per pixel).
ATOMIC_CONNECT = ("void kernel Connect(=>void atomic_add_f( volatile global float* p, const float v ) { union { uint u; float f; } o, n; "
                  "do { o.f = *p; n.f = o.f + v; } while (atomic_cmpxchg( (volatile global uint*)p, o.u, n.u ) != o.u); }\nvoid kernel Connect(;;"
                  "accumulator[as_uint( O4.w )] += T4;=>{ volatile global float* ap = (volatile global float*)(accumulator + as_uint( O4.w )); "
                  "atomic_add_f( ap, T4.x ); atomic_add_f( ap + 1, T4.y ); atomic_add_f( ap + 2, T4.z ); }")


def setup(ctx):
    if not os.path.exists(REFOCL_PATH):
        pytest.skip("oracle/_ref/libtinybvh_refocl.so not built (needs the reference checkout at build time)")
    try:
        ocl = ReferenceOpenCL()
    except (RuntimeError, OSError) as e:
        pytest.skip(f"no OpenCL runtime for the reference kernels: {e}")
    verts = demo_scene()
    W, H = 256, 128
    sc = tb.BVH8_CWBVH(ctx).Build(verts)
    cam = R.camera(*scenes.SPONZA_CAMERAS[0], W, H, 1, 1)
    noise = blue_noise()
    d_verts = ctx.malloc(verts.nbytes); ctx.to_device(d_verts, verts)
    wf = tb.Wavefront(ctx, W, H)
    wf.set_blue_noise(noise)

    def reference(frames, iterations, patch=""):
        h = sc.host
        return ocl.wavefront(h.blob(0, np.uint32, 4), h.blob(1, np.uint32, 4), verts, noise, list(cam.eye), list(cam.p1), list(cam.p2), list(cam.p3), W, H, frames,
                             iterations, patch)

    def mine(frames, iterations, letter=True):
        for f in range(frames):
            wf.render(sc, d_verts, cam, (-22.0, 12.0, 2.0), (25.0, 25.0, 22.0), sky_lo=(0.7, 0.7, 1.2), sky_hi=(0.7, 0.7, 1.2), eps=1e-4, max_depth=iterations,
                      seed=1000 + f, clear=(f == 0), stats=False, light_size=(9.0, 5.0), one_diffuse_bounce=True, reference_letter=letter, sample_index=f)
        return wf.read() / frames

    def done():
        wf.close(); ctx.free(d_verts); sc.free()
    return reference, mine, done


def compare(a_img, b_img):
    a, b = blocks(a_img), blocks(b_img)
    assert np.isfinite(a).all() and np.isfinite(b).all() and a.mean() > 0.05
    return float(np.abs(a - b).mean() / a.mean()), float((b.mean() - a.mean()) / a.mean())


def test_first_vertex_matches_the_unpatched_reference(ctx):
    """Generate, Extend, Shade of the first path vertex (sky, emitter seen directly, next-event estimation with MIS) and Connect, against
    wavefront.cl exactly as shipped."""
    reference, mine, done = setup(ctx)
    rel, bias = compare(reference(512, 1), mine(512, 1))
    print(f"one iteration, unpatched reference: mean relative block difference {rel:.4f}, mean bias {bias:+.4f}")
    assert rel < 0.01 and abs(bias) < 0.005, (rel, bias)
    done()


def test_converged_image_matches_wavefront_cl(ctx):
    """The whole frame loop (3 iterations) against wavefront.cl with Connect's accumulation made atomic (see ATOMIC_CONNECT)."""
    reference, mine, done = setup(ctx)
    frames = 512
    ref = reference(frames, 3, ATOMIC_CONNECT)
    rel, bias = compare(ref, mine(frames, 3))
    print(f"reference-letter mode vs wavefront.cl (atomic Connect): mean relative block difference {rel:.4f}, mean bias {bias:+.4f}")
    assert rel < 0.01 and abs(bias) < 0.005, (rel, bias)
    # the library's default shading (the intent, not the letter) is a different estimator: it must differ measurably
    # from the letter — otherwise the flag would be testing nothing
    rel_intent, _ = compare(ref, mine(frames, 3, letter=False))
    print(f"default shading vs wavefront.cl: mean relative block difference {rel_intent:.4f}")
    assert rel_intent > 2 * rel
    # and the unpatched reference shows the lost contributions: darker than both
    rel_raw, bias_raw = compare(reference(frames, 3), ref)
    print(f"wavefront.cl as shipped vs with the atomic Connect: relative block difference {rel_raw:.4f}, bias of the atomic version {bias_raw:+.4f}")
    assert bias_raw > 0.02
    done()


def test_blue_noise_table_is_used(ctx):
    """Frames 0..3 take the first vertex's random numbers from the table (wavefront.cl:183-189): an all-zero table sends every
    light sample of those frames to one corner of the light and every bounce along N + (1, 0, 0), so the image of such a
    frame differs from the same frame rendered without a table; frame 4 does not look at the table at all."""
    verts = demo_scene()
    W, H = 128, 64
    sc = tb.BVH8_CWBVH(ctx).Build(verts)
    d_verts = ctx.malloc(verts.nbytes); ctx.to_device(d_verts, verts)
    cam = R.camera(*scenes.SPONZA_CAMERAS[0], W, H, 1, 1)
    wf = tb.Wavefront(ctx, W, H)
    kw = dict(sky_lo=(0.7, 0.7, 1.2), sky_hi=(0.7, 0.7, 1.2), eps=1e-4, max_depth=3, seed=7, clear=True, stats=False, light_size=(9.0, 5.0), one_diffuse_bounce=True)

    def frame(idx):
        wf.render(sc, d_verts, cam, (-22.0, 12.0, 2.0), (25.0, 25.0, 22.0), sample_index=idx, **kw)
        return wf.read().copy()
    plain0, plain4 = frame(0), frame(4)
    wf.set_blue_noise(np.zeros(128 * 128 * 8, np.uint32))
    zero0, zero4 = frame(0), frame(4)
    same = lambda x, y: np.allclose(x, y, rtol=1e-4, atol=1e-5)   # float atomics: the order of a pixel's few additions is free
    assert not same(plain0, zero0) and abs(float(plain0.mean() - zero0.mean())) > 1e-3 * float(plain0.mean())
    assert same(plain4, zero4)
    with pytest.raises(tb.TbvhError):
        wf.set_blue_noise(np.zeros(100, np.uint32))
    wf.set_blue_noise(None)
    assert same(frame(0), plain0)
    wf.close(); ctx.free(d_verts); sc.free()
