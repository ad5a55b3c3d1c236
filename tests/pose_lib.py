"""Shared by the pose tests (test_pose_host.py, test_pose_gpu.py), tools/make_pose_golden.py and tools/pose_anim_bench.py (so: NumPy and the compilers only, no
GPU library): deterministic skinned / morphed versions of the committed
bunny, the plain-C restatement of Mesh::SetPose (tests/oracle_pose.c), the real reference behind tests/pose_ref_shim.cpp (compiled per session into a
pytest temp dir when the reference checkout is present), the two session fixtures over them, and the goldens under tests/golden/pose (DESIGN.md par. 14)."""
import ctypes as C
import os

import numpy as np

import native_build as nb
from native_build import _p, _u32, _vp

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "pose")
GOLDEN_STEP = 16        # every 16th triangle of the bunny
N_JOINTS = 24
SMALL = 3 * 313         # the second frame of a golden is kept for this many vertices only (file size)


def bunny(step=8):
    """every step-th triangle of the committed bunny, vertices compacted: (positions (n, 4) with w = 0, indices (m, 3)) — as tests/mesh_lib.py cuts it"""
    d = np.load(os.path.join(HERE, "golden", "meshes", "bunny.npz"))
    idx = d["indices"][::step]
    used, inv = np.unique(idx.reshape(-1), return_inverse=True)
    pos = np.zeros((used.size, 4), np.float32)
    pos[:, :3] = d["positions"][used]
    return pos, np.ascontiguousarray(inv.reshape(-1, 3).astype(np.uint32))


def flatten(pos, idx):
    return np.ascontiguousarray(pos[idx.reshape(-1)])


# ---- the restatement and the real reference ------------------------------------------------------------------------------------------------
class _PoseFns:
    """skin(rest (n, 4), joints (n, 4), weights (n, 4), mats (J, 16)) and morph(positions (T + 1, n, 3), weights (T,)): (n, 4) posed vertices"""

    def __init__(self, so, prefix):
        self.lib = L = C.CDLL(so)
        self._skin = getattr(L, prefix + "_skin"); self._morph = getattr(L, prefix + "_morph")
        self._skin.restype = None; self._morph.restype = None
        self._with_count = prefix == "pref"   # (the shim takes the joint count; the restatement has no use for it)
        if prefix == "porc":
            L.porc_skin_divides.restype = _u32
            L.porc_skin_divides.argtypes = [_vp, _u32, _vp, _vp, _vp]

    def skin(self, rest, joints, weights, mats):
        rest = np.ascontiguousarray(rest, np.float32); joints = np.ascontiguousarray(joints, np.uint32); weights = np.ascontiguousarray(weights, np.float32)
        mats = np.ascontiguousarray(mats, np.float32).reshape(-1, 16)
        assert rest.shape == weights.shape == joints.shape and rest.shape[1] == 4 and int(joints.max()) < mats.shape[0]
        out = np.full((rest.shape[0], 4), np.nan, np.float32)
        if self._with_count:
            self._skin(_p(rest), _u32(rest.shape[0]), _p(joints), _p(weights), _p(mats), _u32(mats.shape[0]), _p(out))
        else:
            self._skin(_p(rest), _u32(rest.shape[0]), _p(joints), _p(weights), _p(mats), _p(out))
        return out

    def morph(self, positions, weights):
        pos = np.ascontiguousarray(positions, np.float32); w = np.ascontiguousarray(weights, np.float32).reshape(-1)
        assert pos.ndim == 3 and pos.shape[2] == 3 and pos.shape[0] == w.size + 1
        out = np.full((pos.shape[1], 4), np.nan, np.float32)
        wp = w if w.size else np.zeros(1, np.float32)
        self._morph(_p(pos), _u32(pos.shape[1]), _u32(w.size), _p(wp), _p(out))
        return out

    def skin_divides(self, rest, joints, weights, mats):
        """how many vertices take the divide branch of ts_transform_point (row_3 != 1)"""
        rest = np.ascontiguousarray(rest, np.float32); joints = np.ascontiguousarray(joints, np.uint32); weights = np.ascontiguousarray(weights, np.float32)
        mats = np.ascontiguousarray(mats, np.float32).reshape(-1, 16)
        return int(self.lib.porc_skin_divides(_p(rest), _u32(rest.shape[0]), _p(joints), _p(weights), _p(mats)))


def compile_oracle(d):
    return _PoseFns(nb.compile_c_oracle(d, "oracle_pose"), "porc")


def compile_ref_shim(d):
    """The real Mesh::SetPose with oracle/Makefile's flags; None when the reference is absent"""
    so = nb.compile_ref_shim(d, "pose_ref_shim.cpp", scene_header=True, need=("tiny_bvh.h", "tiny_scene.h"))
    return so and _PoseFns(so, "pref")


pose_oracle = nb.oracle_fixture("oracle_pose", compile_oracle)
pose_ref = nb.ref_fixture("pose_ref", compile_ref_shim)


# ---- generators ----------------------------------------------------------------------------------------------------------------------------
def skeleton(pos, n_joints=N_JOINTS):
    """A chain of joints along y over the mesh's height.  (joints (n, 4) uint32, weights (n, 4) float32, the joints' heights): every vertex is bound
    to its (up to) four nearest joints with weights 1 / (distance + 2 % of the height), normalised in fp32 — their sum is then 1 only up to rounding, which
    is what sends a vertex into ts_transform_point's divide branch; every 5th vertex is bound to its nearest joint alone (weights 1, 0, 0, 0), which gives
    row_3 == 1 exactly under a matrix whose last row is 0, 0, 0, 1."""
    y = pos[:, 1].astype(np.float32)
    lo, hi = float(y.min()), float(y.max())
    jy = np.linspace(lo, hi, n_joints).astype(np.float32) if n_joints > 1 else np.array([(lo + hi) / 2], np.float32)
    d = np.abs(y[:, None] - jy[None, :]).astype(np.float32)
    k = min(4, n_joints)
    near = np.argsort(d, axis=1, kind="stable")[:, :k]
    joints = np.zeros((pos.shape[0], 4), np.uint32)
    joints[:, :k] = near
    w = np.zeros((pos.shape[0], 4), np.float32)
    w[:, :k] = np.float32(1) / (np.take_along_axis(d, near, 1) + np.float32(0.02 * (hi - lo)))
    if k < 4:   # fewer than four joints: the remaining slots repeat joint 0 with a share of the weight (no weight is skipped for being anything)
        w[:, k:] = w[:, :1] * np.float32(0.5)
    w = (w / w.sum(1, dtype=np.float32)[:, None]).astype(np.float32)
    w[::5] = np.array([1, 0, 0, 0], np.float32)
    return joints, w, jy


def joint_mats(jy, frame, scale=False):
    """Rigid joint matrices (row-major, last row 0 0 0 1) for one frame: joint j turns about the z axis through (0, jy[j], 0) by an angle that swings along the
    chain, and shifts a little; scale=True multiplies in a non-uniform scale about the same pivot."""
    n = jy.size
    j = np.arange(n, dtype=np.float64)
    a = 0.35 * np.sin(0.7 * frame + 0.3 * j) * (j / max(n - 1, 1) + 0.25)
    ext = float(jy.max() - jy.min()) if n > 1 else 1.0
    M = np.zeros((n, 4, 4), np.float64)
    M[:, 3, 3] = 1
    c, s = np.cos(a), np.sin(a)
    R = np.zeros((n, 3, 3)); R[:, 0, 0] = c; R[:, 0, 1] = -s; R[:, 1, 0] = s; R[:, 1, 1] = c; R[:, 2, 2] = 1
    if scale:
        R = R @ np.diag([1.3, 0.8, 1.1])
    piv = np.zeros((n, 3)); piv[:, 1] = jy
    t = np.stack([0.03 * ext * np.sin(0.5 * frame + j), np.zeros(n), 0.02 * ext * np.cos(0.9 * frame + 0.5 * j)], 1)
    M[:, :3, :3] = R
    M[:, :3, 3] = piv - np.einsum("nij,nj->ni", R, piv) + t
    return np.ascontiguousarray(M.reshape(n, 16).astype(np.float32))


def skinned_bunny(step=GOLDEN_STEP, indexed=False, n_joints=N_JOINTS):
    """(rest (n, 4) w = 0, joints, weights, joint heights, indices or None): the flat form has 3 vertices per triangle, the indexed one shared vertices"""
    pos, idx = bunny(step)
    if not indexed:
        pos, idx = flatten(pos, idx), None
    joints, weights, jy = skeleton(pos, n_joints)
    return np.ascontiguousarray(pos, np.float32), joints, weights, jy, idx


def morph_bunny(step=GOLDEN_STEP, n_targets=3, seed=31):
    """positions (n_targets + 1, n, 3) of the flat bunny: the base and smooth displacements of it; and two weight sets"""
    pos, idx = bunny(step)
    base = flatten(pos, idx)[:, :3]
    ext = float(np.linalg.norm(base.max(0) - base.min(0)))
    rng = np.random.default_rng(seed)
    out = [base]
    for t in range(n_targets):
        k = (rng.uniform(4.0, 12.0, (3, 3)) / ext).astype(np.float32); ph = rng.uniform(0, 6.28, 3).astype(np.float32)
        d = np.stack([np.sin(base @ k[0] + ph[0]), np.sin(base @ k[1] + ph[1]), np.sin(base @ k[2] + ph[2])], 1).astype(np.float32)
        out.append((base + np.float32(0.05 * ext) * d).astype(np.float32))
    weights = np.array([[0.25, -0.5, 0.8125], [1.0, 0.3, 0.0]], np.float32)[:, :n_targets]
    return np.ascontiguousarray(np.stack(out), np.float32), weights


def random_skin(n=6000, n_joints=24, seed=7):
    """random vertices, rigid random joint matrices, random joints and normalised random weights (a fifth of the vertices one-hot)"""
    rng = np.random.default_rng(seed)
    rest = np.zeros((n, 4), np.float32); rest[:, :3] = rng.uniform(-2, 2, (n, 3))
    joints = rng.integers(0, n_joints, (n, 4)).astype(np.uint32)
    w = rng.random((n, 4), dtype=np.float32) + np.float32(0.01)
    w = (w / w.sum(1, dtype=np.float32)[:, None]).astype(np.float32)
    w[::5] = np.array([1, 0, 0, 0], np.float32)
    q, _ = np.linalg.qr(rng.normal(size=(n_joints, 3, 3)))
    M = np.zeros((n_joints, 4, 4)); M[:, :3, :3] = q; M[:, :3, 3] = rng.uniform(-1, 1, (n_joints, 3)); M[:, 3, 3] = 1
    return rest, joints, w, np.ascontiguousarray(M.reshape(n_joints, 16).astype(np.float32))


# ---- goldens -------------------------------------------------------------------------------------------------------------------------------
def golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def rest4(g):
    """the golden's rest positions as the (n, 4) array the library takes"""
    r = np.zeros((g["rest"].shape[0], 4), np.float32)
    r[:, :3] = g["rest"]
    return r


def make_golden(ref, out_dir=GOLDEN):
    """Inputs and the REAL reference's posed vertices (ref: compile_ref_shim's).  skin_bunny16 / skin_indexed: frame 0 rigid, whole mesh (`out`); frame 1
    with the non-uniform scale, the first SMALL vertices (`out_b`); skin_bunny16 also the whole mesh under ONE joint (`mats1`, `out1`: every index 0).
    morph_bunny16: 3 targets, weight set 0 for the whole mesh, set 1 for the first SMALL vertices."""
    os.makedirs(out_dir, exist_ok=True)
    for name, indexed in (("skin_bunny16", False), ("skin_indexed", True)):
        rest, joints, weights, jy, idx = skinned_bunny(indexed=indexed)
        mats = np.stack([joint_mats(jy, 1), joint_mats(jy, 2, scale=True)])
        d = dict(rest=np.ascontiguousarray(rest[:, :3]), joints=joints, weights=weights, mats=mats, out=ref.skin(rest, joints, weights, mats[0]),
                 out_b=ref.skin(rest[:SMALL], joints[:SMALL], weights[:SMALL], mats[1]))
        if indexed:
            d["indices"] = idx
        else:
            d["mats1"] = joint_mats(jy[N_JOINTS // 2:N_JOINTS // 2 + 1], 3)
            d["out1"] = ref.skin(rest, np.zeros_like(joints), weights, d["mats1"])
        np.savez_compressed(os.path.join(out_dir, name + ".npz"), **d)
    pos, w = morph_bunny()
    np.savez_compressed(os.path.join(out_dir, "morph_bunny16.npz"), positions=pos, weights=w, out=ref.morph(pos, w[0]),
                        out_b=ref.morph(np.ascontiguousarray(pos[:, :SMALL]), w[1]))
