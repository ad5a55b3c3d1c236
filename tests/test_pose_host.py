"""Mesh::SetPose restated (DESIGN.md par. 14), without a GPU: the plain-C restatement (tests/oracle_pose.c) equals the real reference bit for bit, the
goldens under tests/golden/pose equal the restatement, the library's host path (pose.h through tbvh_host_pose_skin / _morph) equals the restatement, and
the entry points validate what the header says they validate.  Everything is equality of bytes: the same float operations on the same inputs."""
import ctypes as C

import numpy as np
import pytest

import tinybvh_amd as tb
from tinybvh_amd import _capi
import pose_lib as P
from pose_lib import pose_oracle, pose_ref  # noqa: F401  (fixtures)


def same_bytes(a, b):
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def skin_cases():
    """(name, rest, joints, weights, mats) of every skin input the goldens and the GPU tests use, both frames"""
    out = []
    for indexed in (False, True):
        rest, joints, weights, jy, _ = P.skinned_bunny(indexed=indexed)
        for frame, scale in ((1, False), (2, True)):
            out.append((f"indexed={indexed} frame={frame}", rest, joints, weights, P.joint_mats(jy, frame, scale)))
    rest, joints, weights, jy, _ = P.skinned_bunny()
    out.append(("one joint", rest, np.zeros_like(joints), weights, P.joint_mats(jy[P.N_JOINTS // 2:P.N_JOINTS // 2 + 1], 3)))
    return out


def test_restatement_is_the_real_reference(pose_oracle, pose_ref):
    for name, rest, joints, weights, mats in skin_cases():
        assert same_bytes(pose_oracle.skin(rest, joints, weights, mats), pose_ref.skin(rest, joints, weights, mats)), name
    rest, joints, weights, mats = P.random_skin(6000)
    a, b = pose_oracle.skin(rest, joints, weights, mats), pose_ref.skin(rest, joints, weights, mats)
    assert same_bytes(a, b), f"{int((a.view(np.uint32) != b.view(np.uint32)).any(1).sum())} of 6000 random vertices differ"
    for n in (1, 2, 64, 65):   # the shim pads to a multiple of 3: sizes that are none
        assert same_bytes(pose_oracle.skin(rest[:n], joints[:n], weights[:n], mats), pose_ref.skin(rest[:n], joints[:n], weights[:n], mats)), n
    pos, w = P.morph_bunny()
    for k in range(w.shape[0]):
        assert same_bytes(pose_oracle.morph(pos, w[k]), pose_ref.morph(pos, w[k])), k
    rng = np.random.default_rng(3)
    pos = rng.uniform(-2, 2, (3, 6000, 3)).astype(np.float32)
    wt = rng.uniform(-1, 1, 2).astype(np.float32)
    assert same_bytes(pose_oracle.morph(pos, wt), pose_ref.morph(pos, wt))
    assert same_bytes(pose_oracle.morph(pos[:1], []), pose_ref.morph(pos[:1], []))


def test_goldens_match_the_generators_and_the_restatement(pose_oracle):
    for name, indexed in (("skin_bunny16", False), ("skin_indexed", True)):
        g = P.golden(name)
        rest, joints, weights, jy, idx = P.skinned_bunny(indexed=indexed)
        assert same_bytes(g["rest"], rest[:, :3]) and np.array_equal(g["joints"], joints) and same_bytes(g["weights"], weights), name
        assert same_bytes(g["mats"][0], P.joint_mats(jy, 1)) and same_bytes(g["mats"][1], P.joint_mats(jy, 2, scale=True)), name
        r4 = P.rest4(g)
        assert same_bytes(g["out"], pose_oracle.skin(r4, g["joints"], g["weights"], g["mats"][0])), name
        assert g["out_b"].shape[0] == P.SMALL
        assert same_bytes(g["out_b"], pose_oracle.skin(r4, g["joints"], g["weights"], g["mats"][1])[:P.SMALL]), name
        assert not g["out"][:, 3].view(np.uint32).any(), "w of a skinned vertex is +0"
        if indexed:
            assert np.array_equal(g["indices"], idx) and int(g["indices"].max()) == r4.shape[0] - 1
        else:
            assert g["mats1"].shape == (1, 16)
            assert same_bytes(g["out1"], pose_oracle.skin(r4, np.zeros_like(g["joints"]), g["weights"], g["mats1"]))
    g = P.golden("morph_bunny16")
    pos, w = P.morph_bunny()
    assert same_bytes(g["positions"], pos) and same_bytes(g["weights"], w) and pos.shape[0] == 4
    assert same_bytes(g["out"], pose_oracle.morph(pos, w[0]))
    assert same_bytes(g["out_b"], pose_oracle.morph(pos, w[1])[:P.SMALL])
    assert (g["out"][:, 3] == 1).all()


def test_fixtures_hold_both_branches_of_the_divide(pose_oracle):
    """ts_transform_point divides whenever row_3 != 1: one-hot weights on a rigid matrix give exactly 1, weights normalised in fp32 often do not.  Every
    skin input — and its first SMALL vertices, and the small sizes the GPU tests cut — holds vertices of both kinds."""
    for name, rest, joints, weights, mats in skin_cases():
        for n in (63, P.SMALL, rest.shape[0]):
            div = pose_oracle.skin_divides(rest[:n], joints[:n], weights[:n], mats)
            assert 0 < div < n, (name, n, div)
            assert n - div >= n // 5, (name, n, div)   # the one-hot fifth at least
        assert pose_oracle.skin_divides(rest, joints, weights, mats) > rest.shape[0] // 20, name
    rest, joints, weights, mats = P.random_skin(6000)
    div = pose_oracle.skin_divides(rest, joints, weights, mats)
    assert 600 < div < 4800, div


def test_host_pose_is_the_restatement(pose_oracle):
    for name, rest, joints, weights, mats in skin_cases():
        assert same_bytes(tb.host_pose_skin(rest, joints, weights, mats), pose_oracle.skin(rest, joints, weights, mats)), name
    rest, joints, weights, mats = P.random_skin(6000)
    assert same_bytes(tb.host_pose_skin(rest, joints, weights, mats), pose_oracle.skin(rest, joints, weights, mats))
    for n in (1, 63, 64, 65, P.SMALL):
        assert same_bytes(tb.host_pose_skin(rest[:n], joints[:n], weights[:n], mats), pose_oracle.skin(rest[:n], joints[:n], weights[:n], mats)), n
    # (n, 3) rest positions are the same vertices
    assert same_bytes(tb.host_pose_skin(rest[:, :3], joints, weights, mats), pose_oracle.skin(rest, joints, weights, mats))
    pos, w = P.morph_bunny()
    for k in range(w.shape[0]):
        assert same_bytes(tb.host_pose_morph(pos, w[k]), pose_oracle.morph(pos, w[k])), k
    for n in (1, 63, 64, 65, P.SMALL):
        cut = np.ascontiguousarray(pos[:, :n])
        assert same_bytes(tb.host_pose_morph(cut, w[1]), pose_oracle.morph(cut, w[1])), n


def test_a_non_rigid_last_row_divides(pose_oracle):
    """a projective joint matrix: every vertex takes the reciprocal-then-multiply branch"""
    rest, joints, weights, mats = P.random_skin(500)
    mats = mats.copy()
    mats[:, 12:16] = np.array([0.01, -0.02, 0.03, 1.5], np.float32)
    want = pose_oracle.skin(rest, joints, weights, mats)
    assert pose_oracle.skin_divides(rest, joints, weights, mats) == 500
    assert same_bytes(tb.host_pose_skin(rest, joints, weights, mats), want)


def test_zero_targets_copy_the_base_with_w_one():
    pos, _ = P.morph_bunny(n_targets=0)
    assert pos.shape[0] == 1
    out = tb.host_pose_morph(pos, [])
    assert same_bytes(out[:, :3], pos[0]) and (out[:, 3] == 1).all()


def test_validation():
    lib = _capi.lib
    rest, joints, weights, mats = P.random_skin(100)
    out = np.full((100, 4), 7.0, np.float32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    bad = joints.copy(); bad[41, 2] = 24; bad[77, 0] = 99
    assert lib.tbvh_host_pose_skin(p(rest), 100, p(bad), p(weights), p(mats), 24, p(out)) == -5   # TBVH_E_FORMAT
    assert b"vertex 41" in lib.tbvh_last_error()
    assert (out == 7.0).all(), "nothing is written when the indices are refused"
    assert lib.tbvh_host_pose_skin(p(rest), 100, p(joints), p(weights), p(mats), 23, p(out)) == -5   # some index is 23 (24 joints drawn)
    assert lib.tbvh_host_pose_skin(None, 100, p(joints), p(weights), p(mats), 24, p(out)) == -1
    assert lib.tbvh_host_pose_skin(p(rest), 0, p(joints), p(weights), p(mats), 24, p(out)) == -1
    assert lib.tbvh_host_pose_skin(p(rest), 100, p(joints), p(weights), p(mats), 0, p(out)) == -1
    assert lib.tbvh_host_pose_morph(None, 10, 0, None, p(out)) == -1
    assert lib.tbvh_host_pose_morph(p(rest), 10, 2, None, p(out)) == -1   # targets without weights
    # the device entry points refuse null objects and arrays before they touch a device
    h = C.c_void_p()
    assert lib.tbvh_pose_create_skin(None, p(rest), 100, p(joints), p(weights), 24, 0, C.byref(h)) == -1
    assert lib.tbvh_pose_create_morph(None, p(rest), 100, 0, 0, C.byref(h)) == -1
    assert lib.tbvh_pose_set_skin(None, p(mats), 24, 0) == -1 and lib.tbvh_pose_set_morph(None, None, 0, 0) == -1
    assert lib.tbvh_pose_refit(None, None) == -1 and lib.tbvh_pose_download(None, p(out), 100) == -1
    assert lib.tbvh_pose_vertices(None, None, None) == -1
    lib.tbvh_pose_free(None)
    with pytest.raises(tb.TbvhError) as e:
        tb.host_pose_skin(rest, bad, weights, mats)
    assert e.value.code == -5
