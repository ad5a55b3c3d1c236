"""BVH_Double on the host: the record layouts, the two double-precision builders, the restated oracle against brute force, and the
tiny_hip.h binding against the real tiny_bvh.h when it is present."""
import numpy as np
import pytest

import tinybvh_amd as tb
from tinybvh_amd import scenes
from double_lib import instance_scene, odbl, random_rays_dbl, rotated_soup, to_dbl  # noqa: F401 (odbl: fixture)
from native_build import syntax_check


def test_record_layouts():
    assert tb.RAYEX_DTYPE.itemsize == 128 and tb.INSTANCE_EX_DTYPE.itemsize == 320 and tb.NODE_DBL_DTYPE.itemsize == 64
    f = tb.RAYEX_DTYPE.fields
    assert [f[k][1] for k in ("O", "D", "rD", "t", "u", "v", "inst", "prim", "instIdx", "mask")] == [0, 24, 48, 72, 80, 88, 96, 104, 112, 120]
    f = tb.INSTANCE_EX_DTYPE.fields
    assert [f[k][1] for k in ("transform", "invTransform", "aabbMin", "blasIdx", "aabbMax", "mask")] == [0, 128, 256, 280, 288, 312]
    f = tb.NODE_DBL_DTYPE.fields
    assert [f[k][1] for k in ("aabbMin", "aabbMax", "leftFirst", "triCount")] == [0, 24, 48, 56]
    assert tb.LAYOUT_BVH_DOUBLE == 3
    r = tb.make_rays_ex(np.zeros((2, 3)), np.array([[0.0, 0.0, 2.0], [3.0, 4.0, 0.0]]))
    assert np.allclose(r["D"][1], [0.6, 0.8, 0.0], rtol=1e-15, atol=0) and np.isinf(r["rD"][0][:2]).all() and r["rD"][0][2] == 1.0
    assert (r["t"] == 1e300).all() and (r["mask"] == 0xFFFF).all()


def check_tree(nodes, idx, n_prims, prim_box):
    """Every reachable node box contains its children / primitives exactly (no slack), and the leaves partition the index array."""
    assert len(idx) == n_prims and np.array_equal(np.sort(idx), np.arange(n_prims))
    covered = np.zeros(len(idx), np.int64)
    stack = [0]
    while stack:
        i = stack.pop()
        n = nodes[i]
        if n["triCount"] > 0:
            s, c = int(n["leftFirst"]), int(n["triCount"])
            covered[s:s + c] += 1
            lo, hi = prim_box(idx[s:s + c])
            assert (n["aabbMin"] == lo).all() and (n["aabbMax"] == hi).all(), i   # a leaf box is exactly its primitives' box
        else:
            a, b = nodes[int(n["leftFirst"])], nodes[int(n["leftFirst"]) + 1]
            assert (n["aabbMin"] == np.minimum(a["aabbMin"], b["aabbMin"])).all() and (n["aabbMax"] == np.maximum(a["aabbMax"], b["aabbMax"])).all(), i
            stack += [int(n["leftFirst"]), int(n["leftFirst"]) + 1]
    assert (covered == 1).all()


def test_host_builder_blas_far_from_origin():
    v = rotated_soup(20_000) * 1e-3 + np.array([1.3e7, 4.0e6, -7.0e6])
    h = tb.host_build_double(v)
    nodes, idx = h.nodes(), h.prim_idx()
    assert nodes[0]["leftFirst"] == 1   # root's children 1 and 2, as after the reference's builder
    tri = v.reshape(-1, 3, 3)
    check_tree(nodes, idx, tri.shape[0], lambda p: (tri[p].reshape(-1, 3).min(0), tri[p].reshape(-1, 3).max(0)))


def invert_and_bound(T, bb):
    """BLASInstanceEx::InvertTransform + Update (tiny_bvh.h:8432-8472) restated in numpy, one instance."""
    T = [float(x) for x in T]
    iT = [0.0] * 16
    iT[0] = T[5] * T[10] * T[15] - T[5] * T[11] * T[14] - T[9] * T[6] * T[15] + T[9] * T[7] * T[14] + T[13] * T[6] * T[11] - T[13] * T[7] * T[10]
    iT[1] = -T[1] * T[10] * T[15] + T[1] * T[11] * T[14] + T[9] * T[2] * T[15] - T[9] * T[3] * T[14] - T[13] * T[2] * T[11] + T[13] * T[3] * T[10]
    iT[2] = T[1] * T[6] * T[15] - T[1] * T[7] * T[14] - T[5] * T[2] * T[15] + T[5] * T[3] * T[14] + T[13] * T[2] * T[7] - T[13] * T[3] * T[6]
    iT[3] = -T[1] * T[6] * T[11] + T[1] * T[7] * T[10] + T[5] * T[2] * T[11] - T[5] * T[3] * T[10] - T[9] * T[2] * T[7] + T[9] * T[3] * T[6]
    iT[4] = -T[4] * T[10] * T[15] + T[4] * T[11] * T[14] + T[8] * T[6] * T[15] - T[8] * T[7] * T[14] - T[12] * T[6] * T[11] + T[12] * T[7] * T[10]
    iT[5] = T[0] * T[10] * T[15] - T[0] * T[11] * T[14] - T[8] * T[2] * T[15] + T[8] * T[3] * T[14] + T[12] * T[2] * T[11] - T[12] * T[3] * T[10]
    iT[6] = -T[0] * T[6] * T[15] + T[0] * T[7] * T[14] + T[4] * T[2] * T[15] - T[4] * T[3] * T[14] - T[12] * T[2] * T[7] + T[12] * T[3] * T[6]
    iT[7] = T[0] * T[6] * T[11] - T[0] * T[7] * T[10] - T[4] * T[2] * T[11] + T[4] * T[3] * T[10] + T[8] * T[2] * T[7] - T[8] * T[3] * T[6]
    iT[8] = T[4] * T[9] * T[15] - T[4] * T[11] * T[13] - T[8] * T[5] * T[15] + T[8] * T[7] * T[13] + T[12] * T[5] * T[11] - T[12] * T[7] * T[9]
    iT[9] = -T[0] * T[9] * T[15] + T[0] * T[11] * T[13] + T[8] * T[1] * T[15] - T[8] * T[3] * T[13] - T[12] * T[1] * T[11] + T[12] * T[3] * T[9]
    iT[10] = T[0] * T[5] * T[15] - T[0] * T[7] * T[13] - T[4] * T[1] * T[15] + T[4] * T[3] * T[13] + T[12] * T[1] * T[7] - T[12] * T[3] * T[5]
    iT[11] = -T[0] * T[5] * T[11] + T[0] * T[7] * T[9] + T[4] * T[1] * T[11] - T[4] * T[3] * T[9] - T[8] * T[1] * T[7] + T[8] * T[3] * T[5]
    iT[12] = -T[4] * T[9] * T[14] + T[4] * T[10] * T[13] + T[8] * T[5] * T[14] - T[8] * T[6] * T[13] - T[12] * T[5] * T[10] + T[12] * T[6] * T[9]
    iT[13] = T[0] * T[9] * T[14] - T[0] * T[10] * T[13] - T[8] * T[1] * T[14] + T[8] * T[2] * T[13] + T[12] * T[1] * T[10] - T[12] * T[2] * T[9]
    iT[14] = -T[0] * T[5] * T[14] + T[0] * T[6] * T[13] + T[4] * T[1] * T[14] - T[4] * T[2] * T[13] - T[12] * T[1] * T[6] + T[12] * T[2] * T[5]
    iT[15] = T[0] * T[5] * T[10] - T[0] * T[6] * T[9] - T[4] * T[1] * T[10] + T[4] * T[2] * T[9] + T[8] * T[1] * T[6] - T[8] * T[2] * T[5]
    det = T[0] * iT[0] + T[1] * iT[4] + T[2] * iT[8] + T[3] * iT[12]
    if det != 0:
        inv = 1.0 / det
        iT = [x * inv for x in iT]
    lo, hi = [float(np.float32(1e30))] * 3, [-float(np.float32(1e30))] * 3
    for j in range(8):
        p = (bb[3] if j & 1 else bb[0], bb[4] if j & 2 else bb[1], bb[5] if j & 4 else bb[2])
        t = [T[0] * p[0] + T[1] * p[1] + T[2] * p[2] + T[3], T[4] * p[0] + T[5] * p[1] + T[6] * p[2] + T[7], T[8] * p[0] + T[9] * p[1] + T[10] * p[2] + T[11]]
        w = T[12] * p[0] + T[13] * p[1] + T[14] * p[2] + T[15]
        if w != 1:
            rw = 1.0 / w
            t = [x * rw for x in t]
        lo = [l if l < x else x for l, x in zip(lo, t)]
        hi = [h if h > x else x for h, x in zip(hi, t)]
    return np.array(iT), np.array(lo), np.array(hi)


def test_host_builder_tlas():
    blas_verts, inst = instance_scene(300)
    inst["transform"][7, 12:] = [1e-3, 0.0, 0.0, 1.0]   # a projective row: the w != 1 divide of tinybvh_transform_point
    bounds = np.stack([np.concatenate([v.min(0), v.max(0)]) for v in blas_verts])
    h = tb.host_build_tlas_double(inst, bounds)
    for i in range(inst.shape[0]):
        iT, lo, hi = invert_and_bound(inst["transform"][i], bounds[inst["blasIdx"][i]])
        assert np.array_equal(inst["invTransform"][i], iT) and np.array_equal(inst["aabbMin"][i], lo) and np.array_equal(inst["aabbMax"][i], hi), i
    check_tree(h.nodes(), h.prim_idx(), inst.shape[0], lambda p: (inst["aabbMin"][p].min(0), inst["aabbMax"][p].max(0)))


def brute_force(verts, rays, chunk=64):
    """Closest hit over ALL triangles, the arithmetic of BVH_Double::Intersect (numpy float64 operations are single IEEE operations)."""
    tri = verts.reshape(-1, 3, 3)
    v0, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    best = np.full(rays.shape[0], np.inf); prim = np.zeros(rays.shape[0], np.int64); count = np.zeros(rays.shape[0], np.int64)
    for s in range(0, rays.shape[0], chunk):
        O = rays["O"][s:s + chunk, None, :]; D = rays["D"][s:s + chunk, None, :]; tmax = rays["t"][s:s + chunk, None]
        hx = D[..., 1] * e2[None, :, 2] - D[..., 2] * e2[None, :, 1]
        hy = D[..., 2] * e2[None, :, 0] - D[..., 0] * e2[None, :, 2]
        hz = D[..., 0] * e2[None, :, 1] - D[..., 1] * e2[None, :, 0]
        a = e1[None, :, 0] * hx + e1[None, :, 1] * hy + e1[None, :, 2] * hz
        with np.errstate(divide="ignore", invalid="ignore"):
            f = 1 / a
            sx, sy, sz = O[..., 0] - v0[None, :, 0], O[..., 1] - v0[None, :, 1], O[..., 2] - v0[None, :, 2]
            u = f * (sx * hx + sy * hy + sz * hz)
            qx = sy * e1[None, :, 2] - sz * e1[None, :, 1]
            qy = sz * e1[None, :, 0] - sx * e1[None, :, 2]
            qz = sx * e1[None, :, 1] - sy * e1[None, :, 0]
            v = f * (D[..., 0] * qx + D[..., 1] * qy + D[..., 2] * qz)
            t = f * (e2[None, :, 0] * qx + e2[None, :, 1] * qy + e2[None, :, 2] * qz)
        ok = ~(np.abs(a) < 0.0000001) & ~((u < 0) | (v < 0) | (u + v > 1)) & (t > 0) & (t < tmax)
        t = np.where(ok, t, np.inf)
        m = t.min(1)
        best[s:s + chunk] = m; prim[s:s + chunk] = t.argmin(1); count[s:s + chunk] = (t == m[:, None]).sum(1)
    return best, prim, count


@pytest.mark.parametrize("name", ["rotated_soup", "atrium_subset"])
def test_oracle_rule0_matches_brute_force(odbl, name):
    if name == "rotated_soup":
        verts = rotated_soup(20_000, seed=17)
        rays = random_rays_dbl(65536, (-12, -12, -12), (12, 12, 12), seed=5)
    else:
        verts = to_dbl(scenes.atrium(60_000, seed=1))[: 3 * 20_000]
        rays = random_rays_dbl(65536, (-30, 1, -12), (30, 25, 12), seed=6)
    h = tb.host_build_double(verts)
    got = odbl.intersect(h.nodes(), h.prim_idx(), verts, rays, rule=0)
    sample = np.arange(0, rays.shape[0], 8)   # brute force over every triangle for every 8th ray
    best, prim, count = brute_force(verts, rays[sample])
    hit = np.isfinite(best)
    assert hit.sum() > sample.size // 10
    g = got[sample]
    assert np.array_equal(g["t"] < 1e299, hit)
    uniq = hit & (count == 1)
    assert np.array_equal(g["t"][uniq].view(np.uint64), best[uniq].view(np.uint64))
    assert np.array_equal(g["prim"][uniq], prim[uniq].astype(np.uint64))
    assert (g["t"][hit & ~uniq] == best[hit & ~uniq]).all()   # exact ties: the same distance, either triangle
    # rule 1 differs from rule 0 only where distances tie exactly
    got1 = odbl.intersect(h.nodes(), h.prim_idx(), verts, rays, rule=1)
    assert np.array_equal(got1["t"], got["t"])
    occ0 = odbl.occluded(h.nodes(), h.prim_idx(), verts, rays, rule=0)
    assert np.array_equal(occ0.astype(bool), got["t"] < 1e299)


def test_tiny_hip_double_binding_compiles(tmp_path):
    syntax_check(tmp_path, '#include "tiny_bvh.h"\n#include "tiny_hip.h"\n'
                 "void f(tinybvh::BVH_Double& b, tinybvh::BVH_Double& tlas, tinybvh::RayEx* r, uint8_t* o) {\n"
                 "    tinyhip::Scene s(b); std::vector<tinyhip::Scene*> v{&s}; tinyhip::Scene t(tlas, v);\n"
                 "    s.Intersect(r, 4); s.IsOccluded(r, 4, o); t.Intersect(r, 4); t.IsOccluded(r, 4, o);\n}\n")
