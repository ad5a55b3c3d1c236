"""CreateOpacityMicroMap restated (DESIGN.md par. 15), without a GPU: the plain-C restatement (tests/oracle_omm.c) equals the real reference word for word,
the goldens under tests/golden/omm are the generators' inputs with the restatement's words and are not vacuous, the library's host path (omm.h through
tbvh_host_bake_opacity_micromaps) equals the restatement, and the entry points validate what the header says they validate.  Everything is equality of
words: the same float operations on the same inputs."""
import ctypes as C

import numpy as np
import pytest

import tinybvh_amd as tb
from tinybvh_amd import _capi
import omm_lib as O
from omm_lib import omm_oracle, omm_ref  # noqa: F401  (fixtures)


def one_by_one():
    """the mesh over two 1 x 1 textures: alpha 3 (just opaque) and alpha 2 (just not)"""
    return [np.array([[(3 << 24) | 0x123456]], np.uint32), np.array([[(2 << 24) | 0xFFFFFF]], np.uint32)]


def cases():
    """(name, uv, tri_texture, textures) of every input the goldens and the GPU tests use"""
    uv, tt = O.mesh()
    return [("mesh", uv, tt, O.textures()), ("1x1", uv, tt, one_by_one()), ("swapped", uv, tt, O.textures()[::-1]),
            ("all textured", uv, (np.arange(tt.size) % 2).astype(np.uint32), O.textures())]


def test_restatement_is_the_real_reference(omm_oracle, omm_ref):
    for name, uv, tt, tex in cases():
        for N in O.ALL_N:
            a, b = omm_oracle.bake(uv, tt, tex, N), omm_ref.bake(uv, tt, tex, N)
            assert np.array_equal(a, b), f"{name} N={N}: {int((a != b).any(1).sum())} triangles differ"
    uv, tt = O.mesh(600, seed=9)
    assert np.array_equal(omm_oracle.bake(uv, tt, O.textures(), 8), omm_ref.bake(uv, tt, O.textures(), 8))


def test_goldens_match_the_generators_and_the_restatement(omm_oracle):
    uv, tt = O.mesh()
    tex = O.textures()
    uvi, idx = O.indexed(uv)
    for N in O.GOLDEN_N:
        g = O.golden(N)
        assert int(g["N"]) == N and g["words"].shape == (O.GOLDEN_TRIS, O.words_per_tri(N))
        for key, want in (("uv", uv), ("uv_shared", uvi), ("indices", idx), ("tri_texture", tt), ("tex0", tex[0]), ("tex1", tex[1])):
            assert g[key].dtype == want.dtype and g[key].shape == want.shape and g[key].tobytes() == want.tobytes(), (N, key)
        assert np.array_equal(g["words"], omm_oracle.bake(uv, tt, tex, N)), N


def test_goldens_are_not_vacuous(omm_oracle):
    """over the textured triangles of each golden: between 20 and 80 % of the bits set, at least half of them mixed, one fully clear, one fully set; the
    untextured third is all ones, padding included; the alpha test is hit from both sides and the clamp to the last texel is taken"""
    for N in O.GOLDEN_N:
        g = O.golden(N)
        O.check_not_vacuous(g["words"], g["tri_texture"], N)
        none = g["tri_texture"] == O.NO_TEXTURE
        assert abs(int(none.sum()) * 3 - O.GOLDEN_TRIS) <= 3 and (g["words"][none] == 0xFFFFFFFF).all()
        if N * N % 32:
            assert not (g["words"][~none][:, -1] >> (N * N % 32)).any(), "a textured triangle's unused high bits stay 0"
        for k in ("tex0", "tex1"):
            assert set(np.unique(g[k] >> 24)) == set(O.ALPHAS.tolist()), k
        assert omm_oracle.clamped(g["uv"], g["tri_texture"], [g["tex0"], g["tex1"]], N) >= 2 * (4 * N - 1) * 2 * N


def test_host_bake_is_the_restatement(omm_oracle):
    for name, uv, tt, tex in cases():
        for N in O.ALL_N:
            assert np.array_equal(tb.host_bake_opacity_micromaps(uv, tex, N, tri_texture=tt), omm_oracle.bake(uv, tt, tex, N)), (name, N)
    for N in O.GOLDEN_N:
        g = O.golden(N)
        assert np.array_equal(tb.host_bake_opacity_micromaps(g["uv"], [g["tex0"], g["tex1"]], N, tri_texture=g["tri_texture"]), g["words"]), N
    uv, tt = O.mesh()
    for n in (1, 63, 64, 65):
        assert np.array_equal(tb.host_bake_opacity_micromaps(uv[:3 * n], O.textures(), 8, tri_texture=tt[:n]), omm_oracle.bake(uv[:3 * n], tt[:n], O.textures(), 8)), n
    # tri_texture = None: every triangle uses texture 0; one texture passed bare; an RGBA byte texture is the same texels
    t0 = O.textures()[0]
    want = omm_oracle.bake(uv, np.zeros(tt.size, np.uint32), [t0], 4)
    assert np.array_equal(tb.host_bake_opacity_micromaps(uv, t0, 4), want)
    assert np.array_equal(tb.host_bake_opacity_micromaps(uv, [t0.view(np.uint8).reshape(64, 64, 4)], 4), want)


def test_flat_and_indexed_forms_agree():
    for N in O.GOLDEN_N:
        g = O.golden(N)
        tex = [g["tex0"], g["tex1"]]
        assert int(g["indices"].max()) == g["uv_shared"].shape[0] - 1 and g["uv_shared"].shape[0] < g["uv"].shape[0]
        got = tb.host_bake_opacity_micromaps(g["uv_shared"], tex, N, indices=g["indices"], tri_texture=g["tri_texture"])
        assert np.array_equal(got, g["words"]), N


def test_an_interleaved_array_is_used_in_place():
    g = O.golden(4)
    inter = np.full((g["uv"].shape[0], 5), 7.5, np.float32)   # x y z u v
    inter[:, 3:5] = g["uv"]
    view = inter[:, 3:5]
    src, keep = tb._omm_source(view, [g["tex0"], g["tex1"]], None, g["tri_texture"])
    assert src.uv == inter.ctypes.data + 12 and src.uv_stride_bytes == 20 and keep[0] is view
    assert np.array_equal(tb.host_bake_opacity_micromaps(view, [g["tex0"], g["tex1"]], 4, tri_texture=g["tri_texture"]), g["words"])
    first = np.full((g["uv"].shape[0], 3), -3.25, np.float32)   # u v w: uv[:, :2]
    first[:, :2] = g["uv"]
    src, keep = tb._omm_source(first[:, :2], [g["tex0"], g["tex1"]], None, g["tri_texture"])
    assert src.uv == first.ctypes.data and src.uv_stride_bytes == 12
    assert np.array_equal(tb.host_bake_opacity_micromaps(first[:, :2], [g["tex0"], g["tex1"]], 4, tri_texture=g["tri_texture"]), g["words"])


def _source(g, **over):
    """a tbvh_omm_source over a golden's indexed form, fields overridden"""
    tex = [np.ascontiguousarray(g["tex0"]), np.ascontiguousarray(g["tex1"])]
    uv, idx, tt = np.ascontiguousarray(g["uv_shared"]), np.ascontiguousarray(g["indices"]).reshape(-1), np.ascontiguousarray(g["tri_texture"])
    idx, tt = over.pop("idx", idx), over.pop("tt", tt)
    arr = (_capi.AlphaTexture * 2)(*[_capi.AlphaTexture(C.c_void_p(t.ctypes.data), t.shape[1], t.shape[0]) for t in tex])
    src = _capi.OmmSource(C.c_void_p(uv.ctypes.data), uv.shape[0], 8, 0, C.c_void_p(idx.ctypes.data), tt.size, C.c_void_p(tt.ctypes.data), arr, 2)
    for k, v in over.items():
        setattr(src, k, v)
    return src, (tex, uv, idx, tt, arr)


def test_refusals():
    lib = _capi.lib
    g = O.golden(4)
    out = np.full((O.GOLDEN_TRIS, 1), 0x5A5A5A5A, np.uint32)
    po = C.c_void_p(out.ctypes.data)
    src, keep = _source(g)
    assert lib.tbvh_host_bake_opacity_micromaps(C.byref(src), 4, po) == 0 and np.array_equal(out, g["words"])
    out[:] = 0x5A5A5A5A
    for N in (0, 5, 128, 3, 65):
        assert lib.tbvh_host_bake_opacity_micromaps(C.byref(src), N, po) == -1, N
        assert b"power of two" in lib.tbvh_last_error()
    assert lib.tbvh_host_bake_opacity_micromaps(None, 4, po) == -1 and b"null source" in lib.tbvh_last_error()
    assert lib.tbvh_host_bake_opacity_micromaps(C.byref(src), 4, None) == -1
    bad = g["indices"].reshape(-1).copy(); bad[3 * 41 + 2] = g["uv_shared"].shape[0]; bad[3 * 77] = 0xFFFFFFFF
    s2, k2 = _source(g, idx=bad)
    assert lib.tbvh_host_bake_opacity_micromaps(C.byref(s2), 4, po) == -1 and b"triangle 41" in lib.tbvh_last_error()
    badt = g["tri_texture"].copy(); badt[100] = 2; badt[200] = 0xFFFFFFFE
    s3, k3 = _source(g, tt=badt)
    assert lib.tbvh_host_bake_opacity_micromaps(C.byref(s3), 4, po) == -1 and b"triangle 100" in lib.tbvh_last_error()
    for field, value in (("n_tris", 0), ("n_uv", 0), ("uv", None), ("uv_stride_bytes", 4), ("uv_stride_bytes", 10), ("on_device", 1), ("textures", None)):
        s4, k4 = _source(g, **{field: value})
        assert lib.tbvh_host_bake_opacity_micromaps(C.byref(s4), 4, po) == -1, field
    s5, k5 = _source(g)
    k5[4][1].width = 0                                        # a zero-sized texture
    assert lib.tbvh_host_bake_opacity_micromaps(C.byref(s5), 4, po) == -1 and b"texture 1" in lib.tbvh_last_error()
    s6, k6 = _source(g, indices=None)                         # flat form over too few UVs
    assert lib.tbvh_host_bake_opacity_micromaps(C.byref(s6), 4, po) == -1
    s7, k7 = _source(g, tri_texture=None, n_textures=0)       # texture 0 for everyone, and no texture
    assert lib.tbvh_host_bake_opacity_micromaps(C.byref(s7), 4, po) == -1
    assert (out == 0x5A5A5A5A).all(), "nothing is written when the source is refused"
    # the device entry points refuse null objects and bad sources before they touch a device
    assert lib.tbvh_bake_opacity_micromaps(None, C.byref(src), 4, po) == -1
    assert lib.tbvh_bake_set_opacity_micromaps(None, C.byref(src), 4) == -1
    with pytest.raises(tb.TbvhError) as e:
        tb.host_bake_opacity_micromaps(g["uv_shared"], [g["tex0"], g["tex1"]], 4, indices=bad, tri_texture=g["tri_texture"])
    assert e.value.code == -1
    with pytest.raises(tb.TbvhError):
        tb.host_bake_opacity_micromaps(g["uv"], [g["tex0"], g["tex1"]], 5, tri_texture=g["tri_texture"])


def test_no_word_outside_a_triangles_own_is_touched(omm_oracle):
    """guard words around the output; and baking triangles one at a time into a guarded buffer of one triangle's words gives the whole bake's words"""
    lib = _capi.lib
    uv, tt = O.mesh()
    tex = O.textures()
    for N in O.ALL_N:
        W, n, G = O.words_per_tri(N), tt.size, 64
        want = omm_oracle.bake(uv, tt, tex, N)
        buf = np.full(G + n * W + G, 0xDEADBEEF, np.uint32)
        src, keep = tb._omm_source(uv, tex, None, tt)
        assert lib.tbvh_host_bake_opacity_micromaps(C.byref(src), N, C.c_void_p(buf.ctypes.data + 4 * G)) == 0
        assert (buf[:G] == 0xDEADBEEF).all() and (buf[G + n * W:] == 0xDEADBEEF).all(), N
        assert np.array_equal(buf[G:G + n * W].reshape(n, W), want), N
        for i in (0, 4, 7, 10, 12, 16, 299):
            one = np.full(G + W + G, 0xDEADBEEF, np.uint32)
            src, keep = tb._omm_source(uv[3 * i:3 * i + 3], tex, None, tt[i:i + 1])
            assert lib.tbvh_host_bake_opacity_micromaps(C.byref(src), N, C.c_void_p(one.ctypes.data + 4 * G)) == 0
            assert (one[:G] == 0xDEADBEEF).all() and (one[G + W:] == 0xDEADBEEF).all() and np.array_equal(one[G:G + W], want[i]), (N, i)
