"""GetShadingData restated (DESIGN.md par. 16), without a GPU: the plain-C restatement (tests/oracle_shade.c), the real reference (tests/shade_ref_shim.cpp,
skipped without a checkout) and the library's host path (shade.h through tbvh_host_shade_hits) agree bit for bit on every defined record, the goldens under
tests/golden/shade are the generators' inputs with the reference's records, and the entry points validate what the header says they validate.  Everything
is equality of bits: the same float operations on the same inputs.  The records whose reference read lies outside its texture are held to the
restatement's clamp only and never shown to the real reference."""
import ctypes as C

import numpy as np
import pytest

import tinybvh_amd as tb
import shade_lib as L
import shade_fixtures as F
from shade_fixtures import shade_oracle, shade_ref, shade_sets  # noqa: F401  (fixtures)

SETS = ["traced", "synthetic"]


def bits(a):
    return np.ascontiguousarray(np.asarray(a), np.float32).view(np.uint32)


def test_abi_has_the_shading_entry_points():
    for name in ("tbvh_shading_create", "tbvh_shading_set_fat_tris", "tbvh_shading_fat_tris", "tbvh_shading_download_fat_tris", "tbvh_shading_free",
                 "tbvh_shade_hits", "tbvh_shade_hits_device", "tbvh_shade_continue_device", "tbvh_host_shade_hits"):
        assert hasattr(tb.lib, name), name
    assert tb.lib.tbvh_abi_version() == 5
    assert tb.FATTRI_DTYPE == L.FATTRI_DTYPE and tb.MATERIAL_DTYPE == L.MATERIAL_DTYPE and tb.FATTRI_DTYPE.itemsize == 192


@pytest.mark.parametrize("name", SETS)
def test_host_path_is_the_restatement(shade_sets, name):
    sc = F.scene()
    r, inst, want, _ = shade_sets[name]
    for rays in (r, F.ShadeScene.stride128(r)):
        got = tb.host_shade_hits(sc.materials, sc.textures, sc.fat, rays, inst)
        assert np.array_equal(bits(got), bits(want)), f"{int((bits(got) != bits(want)).any(1).sum())} records differ"
    miss = r["t"] >= 1e30
    assert miss.any() and (want[miss, 3] == -1).all() and not np.delete(bits(want[miss]), 3, 1).any()


@pytest.mark.parametrize("name", SETS)
def test_restatement_is_the_real_reference(shade_sets, shade_ref, name):
    sc = F.scene()
    r, inst, want, flags = shade_sets[name]
    ask = (flags & (L.NO_SURFACE | L.REF_OUT_OF_BOUNDS)) == 0          # in-range hits whose texel reads lie inside the textures
    assert ask.sum() >= (r["t"] < 1e30).sum() - 16
    real = shade_ref.shade(sc.materials, sc.textures, sc.fat, r[ask], inst)
    diff = (bits(real)[:, :11] != bits(want[ask])[:, :11]).any(1)
    assert not diff.any(), f"{int(diff.sum())} of {int(ask.sum())} records differ, first {np.flatnonzero(ask)[np.argmax(diff)]}"   # zero exceptions


def test_single_blas_is_instance_0_with_the_identity(shade_oracle):
    sc = F.scene()
    r = sc.synthetic_records()
    r = r[np.isin(r["inst"], (0, 3))].copy()                            # records of slot 0's triangles
    ident = tb.make_instances(np.eye(4, dtype=np.float32)[None], [0])
    r0 = r.copy(); r0["inst"] = 0
    want, _ = shade_oracle.shade(sc.materials, sc.textures, sc.fat, r0, ident)
    alone, _ = shade_oracle.shade(sc.materials, sc.textures, sc.fat[:1], r, None)        # inst is not looked at
    got = tb.host_shade_hits(sc.materials, sc.textures, sc.fat[:1], r, None)
    assert np.array_equal(bits(alone), bits(want)) and np.array_equal(bits(got), bits(want))


@pytest.mark.parametrize("name", SETS)
def test_goldens_match_the_generators_and_all_three(shade_sets, name):
    sc = F.scene()
    r, inst, want, flags = shade_sets[name]
    g = L.golden(name)
    assert g["records"].tobytes() == r.tobytes() and g["instances"].tobytes() == inst.tobytes()
    assert np.array_equal(g["from_reference"], (flags & (L.NO_SURFACE | L.REF_OUT_OF_BOUNDS)) == 0)
    assert np.array_equal(g["want"], bits(want))                        # the real reference's words 0..10 where it was asked, the restatement's elsewhere
    assert np.array_equal(bits(tb.host_shade_hits(sc.materials, sc.textures, sc.fat, g["records"], g["instances"])), g["want"])


def test_the_clamp_reads_the_last_texel(shade_sets):
    sc = F.scene()
    r, _, want, flags = shade_sets["synthetic"]
    oob = (flags & L.REF_OUT_OF_BOUNDS).astype(bool)
    for i in np.flatnonzero(oob):
        mat = sc.materials[sc.fat[0]["material"][r["prim"][i]]]
        assert bits(want[i])[11] == sc.textures[mat["color_texture"]].reshape(-1)[-1]
    inb = (flags & L.WRAPPED).astype(bool) & ~oob & (r["prim"] == F.TRI_WRAP_U)
    tex = sc.textures[0]
    assert inb.any() and (bits(want[inb])[:, 11] == tex[2, 0]).all()   # v = 0.5 of 3 rows: row 1, column `width` = the next row's first texel


def _call_host(mats, tex, slots, rays, inst=None):
    return tb.host_shade_hits(mats, tex, slots, rays, inst)


def test_validation():
    sc = F.scene()
    r = sc.synthetic_records()[:64].copy()
    inst = sc.instances
    bad = sc.materials.copy(); bad["normal_texture"][2] = 4
    with pytest.raises(tb.TbvhError) as e:
        _call_host(bad, sc.textures, sc.fat, r, inst)
    assert e.value.code == -5 and "material 2" in str(e.value) and "texture 4" in str(e.value)
    f = sc.fat[0].copy(); f["material"][[123, 400]] = [4, 9]
    with pytest.raises(tb.TbvhError) as e:
        _call_host(sc.materials, sc.textures, [f, sc.fat[1]], r, inst)
    assert e.value.code == -5 and "triangle 123" in str(e.value)
    out = np.zeros((64, 12), np.float32)
    mats = sc.materials
    tex = [np.ascontiguousarray(t) for t in sc.textures]
    arr = (tb.AlphaTexture * 4)(*[tb.AlphaTexture(C.c_void_p(t.ctypes.data), t.shape[1], t.shape[0]) for t in tex])
    slots = [np.ascontiguousarray(x) for x in sc.fat]
    ptrs = (C.c_void_p * 2)(*[x.ctypes.data for x in slots])
    counts = np.array([x.size for x in slots], np.uint64)
    P = lambda a: C.c_void_p(a.ctypes.data)

    def call(m=P(mats), nm=4, t=arr, nt=4, p=ptrs, c=P(counts), ns=2, i=P(inst), ni=5, rays=P(r), n=64, stride=64, o=P(out)):
        return tb.lib.tbvh_host_shade_hits(m, nm, t, nt, p, c, ns, i, ni, rays, n, stride, o)
    assert call() == 0
    for kw in (dict(m=None), dict(nm=0), dict(t=None), dict(p=None), dict(ns=0), dict(rays=None), dict(o=None), dict(stride=48), dict(stride=72),
               dict(rays=C.c_void_p(r.ctypes.data + 4)), dict(o=C.c_void_p(out.ctypes.data + 8)), dict(i=C.c_void_p(inst.ctypes.data + 4)), dict(ni=0)):
        assert call(**kw) == -1, kw
    zero = (tb.AlphaTexture * 4)(*[tb.AlphaTexture(C.c_void_p(t.ctypes.data), 0 if k == 1 else t.shape[1], t.shape[0]) for k, t in enumerate(tex)])
    assert call(t=zero) == -1 and "texture 1" in tb.lib.tbvh_last_error().decode()
    # a record whose inst / prim is no instance / triangle: "no surface", TBVH_E_FORMAT after every record was written
    rb = r.copy(); rb["inst"][3] = 5; rb["prim"][7] = 1 << 30
    out[:] = 9
    assert call(rays=P(rb)) == -5
    good = np.asarray(_call_host(sc.materials, sc.textures, sc.fat, r, inst))
    keep = np.ones(64, bool); keep[[3, 7]] = False
    assert np.array_equal(bits(out[keep]), bits(good[keep])) and (out[[3, 7], 3] == -1).all() and not np.delete(bits(out[[3, 7]]), 3, 1).any()


# ---- the FatTri half of SetPose ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pose_cases():
    return F.pose_cases()


@pytest.mark.parametrize("kind", ["skin", "morph"])
def test_posed_fat_tris_are_the_real_setpose(shade_ref, pose_cases, kind):
    """tbvh_host_pose_* + the host form of the update = the real Mesh::SetPose bytewise: vertex0..2, vN0..2 and Nx Ny Nz for a skin, vertex0..2 and vN0..2 for a morph
    pose; every other byte of every record unchanged"""
    fat, c = F.scene().fat[0], pose_cases[kind]
    for frame in (0, 1):
        if kind == "skin":
            real = shade_ref.setpose_skin(fat, c["rest"], c["joints"], c["weights"], c["normals"], c["mats"][frame])
        else:
            real = shade_ref.setpose_morph(fat, c["positions"], c["normals"], c["weights"][frame])
        got = F.host_posed(c, kind, frame)
        assert got.tobytes() == real.tobytes(), f"{kind} frame {frame}: {int((L.words(got) != L.words(real)).any(1).sum())} records differ"
        fields = L.skin_fields() if kind == "skin" else L.morph_fields()
        assert L.only_these_changed(fat, got, fields)
        for f in fields:
            assert not np.array_equal(got[f], fat[f]), f                # ... and those did change
    if kind == "morph":
        assert np.array_equal(F.host_posed(c, kind, 0)["vN1"], F.host_posed(c, kind, 1)["vN1"])   # the normals take no weights: the reference's arithmetic


@pytest.mark.parametrize("kind,name", [("skin", "pose_skin"), ("skin_indexed", "pose_skin"), ("morph", "pose_morph")])
def test_pose_goldens_match_the_host_path(pose_cases, kind, name):
    g, fat = L.golden(name), F.scene().fat[0]
    a, b = F.host_posed(pose_cases[kind], kind, 0), F.host_posed(pose_cases[kind], kind, 1)
    assert g["written"].shape == (fat.size, 24) and g["written_b"].shape == (L.POSE_SMALL, 24)
    assert np.array_equal(L.words(a)[:, L.WRITTEN_WORDS], g["written"]) and np.array_equal(L.words(b)[:L.POSE_SMALL, L.WRITTEN_WORDS], g["written_b"])
    assert L.only_these_changed(fat, a, L.morph_fields() if kind == "morph" else L.skin_fields())


def test_pose_update_validation(pose_cases):
    c, fat = pose_cases["skin_indexed"], F.scene().fat[0]
    v = tb.host_pose_skin(c["rest"], c["joints"], c["weights"], c["mats"][0])
    n = tb.host_pose_skin_normals(c["normals"], c["joints"], c["weights"], c["mats"][0])
    bad = c["indices"].copy(); bad[17, 1] = v.shape[0]
    with pytest.raises(tb.TbvhError) as e:
        tb.host_pose_fat_tris(fat, v, n, indices=bad)
    assert e.value.code == -5 and "triangle 17" in str(e.value)
    with pytest.raises(tb.TbvhError) as e:                              # without indices: three vertices per triangle
        tb.host_pose_fat_tris(fat, v, n)
    assert e.value.code == -1
    for name in ("tbvh_pose_attach_fat_tris", "tbvh_host_pose_skin_normals", "tbvh_host_pose_morph_normals", "tbvh_host_pose_update_fat_tris"):
        assert hasattr(tb.lib, name), name
