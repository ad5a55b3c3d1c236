"""tbvh_scene_device_bytes is a function of what a scene holds when asked, not of the calls that led there (tinybvh_amd/csrc/capi_scene.hip: sceneBytesByWord;
the eight words of tbvh_debug_scene_bytes are include/tinybvh_amd_debug.h's).  Two routes to one state give one number, an update with a smaller blob gives the
number of that blob, an owner's number follows its copies as they are, and words 0 to 6 sum to the number after every step on every kind of scene.  Small
geometry only: the bookkeeping does not depend on the size (the copies that only a 48 MB blob grows are covered by construction: the owner asks the copy)."""
import os

import numpy as np
import pytest

import tinybvh_amd as tb
from tinybvh_amd import rays as R
from test_wide_copy_host import decode

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
UPLOADED, RELAYOUTS, COPIES, MAPS, MESH_INDICES, TLAS_PARTS, SCRATCH, UNCOUNTED = range(8)


@pytest.fixture(scope="module")
def soup():
    return np.load(os.path.join(GOLDEN, "soup_2k.npz"))


@pytest.fixture(scope="module")
def bunny():
    return np.load(os.path.join(GOLDEN, "mesh", "bunny_indexed.npz"))


def words(scene):
    """the breakdown, after checking that it is one of device_bytes"""
    w = scene.debug_bytes()
    assert sum(w[:7]) == scene.device_bytes, w
    return w


def maps_bytes(n_tris, N):
    """what tbvh_set_opacity_micromaps allocates (capi_scene.hip: allocOpacityMaps): the maps and the padding one row past the last map may read"""
    return (((N * N + 31) >> 5) * n_tris + (((N + 1) * (N + 1) + 63) >> 5)) * 4


def test_cwbvh_update_to_another_topology_keeps_maps_indices(ctx, bunny):
    """A BVH8_CWBVH scene from an indexed mesh with opacity maps, updated with a blob of another topology: the number is the new blob's, plus the maps and the
    held indices, which the update does not touch.  (Before the number was derived the update set it to blocks x 16 + maps: the 12 bytes per triangle of the
    held index buffer vanished — 34824 bytes here; recorded in profiles/scene_bytes.txt.)"""
    pos, idx = bunny["positions"], bunny["indices"]
    n_tris = idx.shape[0]
    blobs = []
    for leaf in (1, 3):   # the same triangles, two trees: one triangle per leaf makes more nodes
        h = tb.HostBVH(pos, tb.LAYOUT_BVH2_WALD, threads=1, max_leaf_tris=leaf, indices=idx)
        sc = tb.BVH8_CWBVH(ctx).ConvertFromBVH2(h.bvh2_nodes(), h.bvh2_prim_idx(), pos, indices=idx)
        blobs.append((sc, sc.download_blobs()))
    (sc, (nodes_a, tris_a)), (other, (nodes_b, tris_b)) = blobs
    other.free()
    assert nodes_b.shape[0] < nodes_a.shape[0] and tris_b.shape[0] <= tris_a.shape[0]   # (the update goes in place only if it fits)
    N = 4
    sc.SetOpacityMicroMaps(np.full((n_tris, 1), 0xFFFF, np.uint32), N)
    before = words(sc)
    assert before[UPLOADED] == (nodes_a.shape[0] + tris_a.shape[0]) * 16
    assert before[MAPS] == maps_bytes(n_tris, N) and before[MESH_INDICES] == 12 * n_tris
    sc.Update(nodes_b, tris_b)
    after = words(sc)
    print("device_bytes after the update", sc.device_bytes, "words", after)
    assert sc.device_bytes == (nodes_b.shape[0] + tris_b.shape[0]) * 16 + maps_bytes(n_tris, N) + 12 * n_tris
    assert after[MAPS] == before[MAPS] and after[MESH_INDICES] == before[MESH_INDICES]
    sc.Update(nodes_a, tris_a)
    assert words(sc)[:7] == before[:7]
    sc.free()


@pytest.mark.parametrize("layout", [tb.LAYOUT_BVH_GPU, tb.LAYOUT_BVH4_GPU])
def test_update_with_a_smaller_blob_reports_that_blob(ctx, soup, layout):
    verts = soup["verts"]
    cls = tb.LAYOUT_CLASSES[layout]

    def args(h):
        return (h.blob(0, np.uint32, 16), h.blob(1, np.uint32, 1).reshape(-1), verts) if layout == tb.LAYOUT_BVH_GPU else (h.blob(0, np.uint32, 4),)

    big, small = tb.HostBVH(verts, layout, threads=1, max_leaf_tris=1), tb.HostBVH(verts, layout, threads=1)
    assert small.blob(0, np.uint32, 4).shape[0] < big.blob(0, np.uint32, 4).shape[0]
    fresh = cls(ctx).Upload(*args(small))
    sc = cls(ctx).Upload(*args(big))
    first = words(sc)
    sc.Update(*args(small))
    assert sc.device_bytes == fresh.device_bytes and words(sc)[:7] == words(fresh)[:7]
    blob = args(small)
    assert sc.device_bytes == blob[0].nbytes + (48 * blob[1].size if layout == tb.LAYOUT_BVH_GPU else 0)   # 64 bytes per node and 48 per gathered triangle, or the stream
    sc.Update(*args(big))
    assert words(sc)[:7] == first[:7]
    sc.free(); fresh.free()


def test_set_hybrid_twice_is_set_hybrid_once(ctx, soup):
    nodes, tris = soup["cwbvh_nodes_0"], soup["cwbvh_tris_0"]
    n_nodes, n_recs = nodes.shape[0] // 5, tris.shape[0] // 3
    k1, k2 = 8, (n_nodes - 1) & ~7   # multiples of 8 below the node count: the smallest and the largest
    assert 0 < k1 < k2 < n_nodes
    plain = (nodes.shape[0] + tris.shape[0]) * 16
    a, b = tb.BVH8_CWBVH(ctx).Upload(nodes, tris), tb.BVH8_CWBVH(ctx).Upload(nodes, tris)
    assert a.device_bytes == plain
    a.set_hybrid(k1); a.set_hybrid(k2)
    b.set_hybrid(k2)
    assert words(a) == words(b)
    assert a.device_bytes == plain + (k2 * 5 + (n_nodes - k2) * 8) * 16 + n_recs * 64   # the hybrid nodes (cwbvh_node.h: kNodeHybrid) and the 64-byte records
    a.set_hybrid(-1)
    w = words(a)
    assert a.device_bytes == plain + n_recs * 64 and w[RELAYOUTS] == n_recs * 64   # the padded records are still held
    assert w[UNCOUNTED] == n_nodes * 4                                           # ... and so is the hybrid copy's numbering, which is not counted
    a.set_hybrid(k2)
    assert words(a) == words(b)
    a.free(); b.free()


def identical_cwbvh(ctx, blocks16):
    """the tree a BVH4_GPU scene's 8-wide copy is, made directly: the BVH2 and the triangle records the library derives on the host from the stream
    (tbvh_debug_wide_copy_bvh2), through the public device conversion.  (The vertices are rebuilt from the records {v0, e1, e2}; the collapse reads the BVH2's
    boxes and leaf sizes only, so the tree has the copy's node and record counts.)"""
    n2, recs = decode(8, blocks16)
    v = np.zeros((recs.shape[0], 3, 4), np.float32)
    v[:, 0, :3] = recs[:, 0, :3]; v[:, 1, :3] = recs[:, 0, :3] + recs[:, 1, :3]; v[:, 2, :3] = recs[:, 0, :3] + recs[:, 2, :3]
    return tb.BVH8_CWBVH(ctx).ConvertFromBVH2(n2.view(np.uint32), np.arange(recs.shape[0], dtype=np.uint32), v.reshape(-1, 4))


def test_an_owner_reports_its_copy_as_the_copy_is(ctx, soup, monkeypatch):
    monkeypatch.setenv("TBVH_WIDE_COPY_MIN", "64")
    blocks, verts = soup["bvh4_0"], soup["verts"]
    lo, hi = verts[:, :3].min(0), verts[:, :3].max(0)
    n = 4096
    d = ctx.malloc(n * 64)
    ctx.to_device(d, R.random_rays(n, lo, hi, seed=5))
    sc = tb.BVH4_GPU(ctx).Upload(blocks)
    plain = blocks.shape[0] * 16
    assert words(sc) == [plain, 0, 0, 0, 0, 0, 0, 0]

    def ask():
        sc.intersect_device(d, n)
        ctx.synchronize()

    ask()
    first = words(sc)
    assert first[UPLOADED] == plain and first[COPIES] > 0 and sc.device_bytes == plain + first[COPIES]
    twin = identical_cwbvh(ctx, blocks)
    assert first[COPIES] == twin.device_bytes
    twin.free()
    sc.Update(blocks)
    assert words(sc) == [plain, 0, 0, 0, 0, 0, 0, 0]   # plain, exactly
    for k in range(3):   # (copy_policy.h: the copy comes back with the fourth query after an update)
        ask()
        assert sc.device_bytes == plain, k
    ask()
    assert words(sc)[:7] == first[:7]
    ctx.free(d); sc.free()


def instances(n, extent):
    t = np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))
    t[:, 0, 3] = np.arange(n, dtype=np.float32) * 1.5 * extent
    return tb.make_instances(t, np.arange(n, dtype=np.uint32) % 3)


def test_a_tlas_and_its_blases_follow_the_copies_the_tlas_asks_for(ctx, soup):
    verts = soup["verts"]
    lo, hi = verts[:, :3].min(0), verts[:, :3].max(0)
    ext = float(hi[0] - lo[0])
    blas = [tb.BVH_GPU(ctx).Build(verts, threads=1), tb.BVH4_GPU(ctx).Build(verts, threads=1), tb.BVH8_CWBVH(ctx).Build(verts, threads=1)]
    alone = [words(b) for b in blas]
    assert all(w[COPIES] == 0 for w in alone)
    tl = tb.TLAS(ctx).Build(instances(8, ext), blas)
    under = [words(b) for b in blas]
    # closest-hit queries enter BVH_GPU and BVH8_CWBVH BLASes through 4-wide copies, made when the TLAS is uploaded; a BVH4_GPU BLAS is entered as it is
    assert under[0][COPIES] > 0 and under[1][COPIES] == 0 and under[2][COPIES] > 0
    t0 = words(tl)
    n = 4096
    d, d_occ = ctx.malloc(n * 64), ctx.malloc(n)
    ctx.to_device(d, R.random_rays(n, lo, hi + np.array([8 * 1.5 * ext, 0, 0], np.float32), seed=5))
    tl.intersect_device(d, n)
    ctx.synchronize()
    assert [words(b)[:7] for b in blas] == [w[:7] for w in under] and words(tl)[:7] == t0[:7]   # a TLAS that only answers Intersect pays for nothing more
    tl.occluded_device(d, n, d_occ)
    ctx.synchronize()
    after = [words(b) for b in blas]
    t1 = words(tl)
    print("BLAS words", after, "TLAS words", t0, t1)
    # the first any-hit query makes the 8-wide copies of the BVH_GPU and BVH4_GPU BLASes (a BVH8_CWBVH BLAS has none to make) and the TLAS's second wide tree
    assert after[0][COPIES] > under[0][COPIES] and after[1][COPIES] > under[1][COPIES] and after[2][COPIES] == under[2][COPIES]
    assert t1[TLAS_PARTS] > t0[TLAS_PARTS] and t1[UPLOADED] == t0[UPLOADED]
    for k in range(3):
        assert after[k][UPLOADED] == alone[k][UPLOADED] and blas[k].device_bytes == alone[k][UPLOADED] + after[k][COPIES]
    ctx.free(d); ctx.free(d_occ)
    tl.free()
    for b in blas:
        b.free()


def test_the_words_sum_to_the_number_after_every_step(soup, monkeypatch):
    """the cycle of tests/test_device_memory.py — every kind of scene, every place a scene owns device memory — with the sum checked on every scene after every step"""
    verts = soup["verts"]
    lo, hi = verts[:, :3].min(0), verts[:, :3].max(0)
    pos, inv = np.unique(verts, axis=0, return_inverse=True)
    pos = np.ascontiguousarray(pos, np.float32); idx = np.ascontiguousarray(inv.reshape(-1, 3).astype(np.uint32))
    ctx = tb.Context(0)
    scenes = []

    def step():
        for s in scenes:
            words(s)

    blas = [tb.BVH_GPU(ctx).Build(pos, indices=idx, threads=1), tb.BVH4_GPU(ctx).Build(verts, threads=1), tb.BVH8_CWBVH(ctx).Build(verts, threads=1)]
    assert words(blas[0])[MESH_INDICES] == 12 * idx.shape[0]
    rng = np.random.default_rng(3)
    sph = np.concatenate([rng.uniform(lo, hi, (200, 3)), rng.uniform(0.01, 0.05, (200, 1))], axis=1).astype(np.float32)
    spheres = tb.SphereBVH(ctx).Build(sph)
    moving = tb.SphereBVH(ctx).BuildOnDevice(sph)
    voxels = tb.VoxelSet(ctx).Build(tb.load_voxel_file(os.path.join(GOLDEN, "voxels", "rock.bin")))
    dverts = verts[:, :3].astype(np.float64)
    dbl = tb.BVH_Double(ctx).Build(dverts)
    inst_ex = tb.make_instances_ex(np.tile(np.eye(4), (2, 1, 1)), np.zeros(2, np.uint64))
    tdbl = tb.TLAS_Double(ctx).Build(inst_ex, [dbl])
    scenes += blas + [spheres, moving, voxels, dbl, tdbl]
    step()
    rex = tb.make_rays_ex(rng.uniform(lo, hi, (256, 3)), rng.normal(size=(256, 3)))
    tdbl.Intersect(rex.copy()); tdbl.IsOccluded(rex)
    r256 = R.random_rays(256, lo, hi, seed=2)
    spheres.Intersect(r256.copy()); voxels.IsOccluded(R.random_rays(256, (0, 0, 0), (1, 1, 1), seed=2))
    step()
    moving.RebuildOnDevice(sph); step()
    moving.Refit(sph); step()
    assert words(moving)[SCRATCH] > 0 and words(moving)[UNCOUNTED] == 0   # a sphere scene counts its scratch and staging
    dbl.Refit(dverts); step()
    assert words(dbl)[SCRATCH] > 0 and words(dbl)[UNCOUNTED] == 0         # ... and so does an fp64 one
    tdbl.RebuildOnDevice(np.tile(np.eye(4).reshape(16), (2, 1))); step()
    assert words(tdbl)[UPLOADED] == 0 and words(tdbl)[TLAS_PARTS] > 0 and words(tdbl)[SCRATCH] > 0

    ext = float(hi[0] - lo[0])
    tl = tb.TLAS(ctx).Build(instances(8, ext), blas)
    scenes.append(tl); step()
    n = 4096
    rays = R.random_rays(n, lo, hi + np.array([8 * 1.5 * ext, 0, 0], np.float32), seed=5)
    d_rays, d_occ = ctx.malloc(n * 64), ctx.malloc(n)
    ctx.to_device(d_rays, rays)
    tl.intersect_device(d_rays, n); ctx.synchronize(); step()
    tl.occluded_device(d_rays, n, d_occ); ctx.synchronize(); step()
    tl.Build(instances(40, ext), blas); step()                     # (an update: the TLAS arrays grow)
    tl.RebuildOnDevice(np.tile(np.eye(4, dtype=np.float32).reshape(16), (40, 1))); step()
    tl.RebuildOnDevice(builder="sah"); step()
    assert words(tl)[SCRATCH] > 0                                  # (the SAH builder's scratch is the TLAS's own and counted)
    tl.occluded_device(d_rays, n, d_occ); ctx.synchronize(); step()

    n_tris = verts.shape[0] // 3
    blas[2].SetOpacityMicroMaps(np.full((n_tris, 1), 0xFFFF, np.uint32), 4); step()
    assert words(blas[2])[MAPS] == maps_bytes(n_tris, 4)
    blas[2].SetOpacityMicroMaps(None, 0); step()
    assert words(blas[2])[MAPS] == 0
    blas[1].Refit(verts); step()
    assert words(blas[1])[UNCOUNTED] > 0 and words(blas[1])[SCRATCH] == 0   # a triangle scene's refit scratch and staging are held, not counted
    blas[0].intersect_spheres(sph, pos, indices=idx); step()

    monkeypatch.setenv("TBVH_WIDE_COPY_MIN", "64")
    solo = tb.BVH4_GPU(ctx).Upload(soup["bvh4_0"])
    scenes.append(solo); step()
    solo.intersect_device(d_rays, n); ctx.synchronize(); step()
    solo.Update(soup["bvh4_0"]); step()
    monkeypatch.delenv("TBVH_WIDE_COPY_MIN")

    ctx.free(d_rays); ctx.free(d_occ)
    blas[0].free()   # still under the TLAS: it goes with the TLAS
    tl.free()
    for s in (blas[1], blas[2], solo, spheres, moving, voxels, tdbl, dbl):
        s.free()
    ctx.close()
