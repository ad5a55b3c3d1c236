"""The wave-packet kernel after its scalar diet (kernels_cwbvh_packet.hip: the branch-free triangle test tri_test_flat, the survivor loop with its first two
children peeled, the traversal compiled once per kind of chunk, hit flags carried as wave masks; variant 92 forces the kernel whatever the batch) against the
strict per-lane kernel (variant 72) on the same scene: hit records byte for byte, occlusion flags equal.  None of the changes touches which nodes a wave
visits, which triangles it tests, their order or the arithmetic of a test, so the records must be the bytes they were.

The shapes are the smallest at which each changed piece can go wrong: batches of 1, 63, 64, 65 and 4 097 rays (lanes without a ray, a last partial chunk); a
chunk of mixed octants and a chunk with a non-finite origin (both turn the filter off: the other two copies of the traversal); a node all of whose children
are leaves, leaf slots of 3 triangles and four children that survive the filter (the peeled loop's remainder); for the flat triangle test an edge-on
triangle, rays through the vertices and along the edges (u = 0, v = 0, u + v = 1 exactly), t equal to the ray's tmax and t < 0; a launch that is not fresh,
with stored hits closer than any triangle.  Every case was run on the parent commit first, where variants 92 and 72 agree on all of them.  Two inputs on which the
parent's two kernels ALREADY differ are not here (profiles/packet_scalar.txt): a triangle with a NaN vertex — its NaN reaches the root's box, and the per-lane and
the packet kernel's box tests treat a NaN plane differently, 66 of 96 records —, which tests/test_tri_flat_host.py covers for the triangle test itself; and the
vertex rays under TIGHT leaf boxes (see edge_bvh2)."""
import numpy as np
import pytest

import tinybvh_amd as tb
from tinybvh_amd import rays as R
from tinybvh_amd import scenes

SOUP_CAM = ((-3.0, 5.0, -4.0), (0.6, -0.2, 0.75))


def both(sc, rays, but=()):
    """-> the records of variant 72 (strict per-lane); asserts variant 92's are the same bytes and the occlusion flags agree (rays `but` left out)"""
    sc.set_variant(72)
    want = sc.Intersect(rays.copy())
    occ_want = sc.IsOccluded(rays.copy())
    sc.set_variant(92)
    got = sc.Intersect(rays.copy())
    occ = sc.IsOccluded(rays.copy())
    diff = np.flatnonzero((got.view(np.uint8).reshape(-1, 64) != want.view(np.uint8).reshape(-1, 64)).any(1))
    diff = diff[~np.isin(diff, but)]
    occ[list(but)] = occ_want[list(but)]
    assert diff.size == 0, (diff.size, diff[:8], got[diff[:2]], want[diff[:2]])
    assert np.array_equal(occ, occ_want), np.flatnonzero(occ != occ_want)[:8]
    return want


@pytest.fixture(scope="module")
def soup(ctx):
    sc = tb.BVH8_CWBVH(ctx).Build(scenes.soup(3_000, seed=5))
    yield sc
    sc.free()


@pytest.fixture(scope="module")
def soup_rays():
    return R.primary(R.camera(*SOUP_CAM, 128, 128, 1, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_batch_sizes_around_a_chunk(soup, soup_rays, n):
    first = 64 * 40                                                            # (chunks in the middle of the image: they hit the soup)
    got = both(soup, soup_rays[first:first + n].copy())
    if n >= 63:
        assert int((got["t"] < 1e30).sum()) > 0


@pytest.mark.gpu
def test_a_chunk_of_mixed_octants_and_one_with_a_non_finite_origin(soup, soup_rays):
    def one_octant(c):
        return len({tuple(x) for x in (soup_rays["rD"][64 * c:64 * c + 64] < 0).tolist()}) == 1
    c0 = next(c for c in range(40, 200) if one_octant(c) and one_octant(c + 1) and one_octant(c + 2))
    base = soup_rays[64 * c0:64 * (c0 + 3)].copy()                             # three chunks, each of one octant
    # chunk 0: every other lane looks the other way along x and y: the lanes differ in octant
    D = base["D"].copy()
    D[1:64:2, 0] *= -1; D[1:64:2, 1] *= -1
    rays = R.make_rays(base["O"], D, normalize=False)
    assert len({tuple(x) for x in (rays["rD"][:64] < 0).tolist()}) > 1
    got = both(soup, rays)
    assert int((got["t"] < 1e30).sum()) > 0
    # chunk 1: one lane's origin is not finite: the filter is off for the chunk, the other 63 rays and the other chunks take their usual way.  The ray itself is
    # left out: every comparison with a NaN is false, so it "hits" whatever triangle it is shown, the packet kernel shows it the wave's and the per-lane kernel
    # its own — the two differ for that one ray on the parent commit as well (+inf: ray 81 of 192), and for no other.
    for bad in (np.inf, -np.inf, np.nan):
        rays = base.copy()
        rays["O"][64 + 17, 1] = bad
        both(soup, rays, but=(64 + 17,))


def layered_bvh2():
    """A BVH2 by hand (BVH::BVHNode layout): root -> two interior nodes -> four leaves of THREE triangles each, the leaves stacked in z, every leaf's box spanning the
    same square in x and y.  Collapsed 8-wide: one node, all four children leaves with three triangles, and every ray that looks down -z enters all four boxes."""
    tris, boxes = [], []
    for layer in range(4):
        z = 1.0 + layer
        # three triangles per layer, each over a third of the square [0, 6] x [0, 6] in x (so a ray meets one triangle per layer at most, or none near the rims)
        for k in range(3):
            x0 = 2.0 * k + 0.25 * layer
            tris.append([[x0, 0.0, z], [x0 + 1.5, 0.0, z + 0.125 * k], [x0, 6.0, z]])
        boxes.append(([0.0, 0.0, z], [6.75, 6.0, z + 0.25]))
    verts = np.zeros((36, 4), np.float32)
    verts[:, :3] = np.asarray(tris, np.float32).reshape(-1, 3)
    nodes = np.zeros((8, 8), np.float32)
    u = nodes.view(np.uint32)

    def put(i, lo, hi, left_first, count):
        nodes[i, 0:3] = lo; nodes[i, 4:7] = hi
        u[i, 3] = left_first; u[i, 7] = count

    for leaf in range(4):
        put(4 + leaf, boxes[leaf][0], boxes[leaf][1], 3 * leaf, 3)
    put(2, boxes[0][0], boxes[1][1], 4, 0)
    put(3, boxes[2][0], boxes[3][1], 6, 0)
    put(0, boxes[0][0], boxes[3][1], 2, 0)
    return nodes, np.arange(12, dtype=np.uint32), verts


@pytest.mark.gpu
def test_all_leaf_node_with_three_triangle_slots_and_four_survivors(ctx):
    n2, pi, verts = layered_bvh2()
    sc = tb.BVH8_CWBVH(ctx).ConvertFromBVH2(n2, pi, verts)
    # 16 x 20 parallel rays down -z over the whole square: a 64-ray chunk spans all of x, so the wave's origin box meets every child's box
    xs, ys = np.meshgrid(np.linspace(0.05, 6.7, 16, dtype=np.float32), np.linspace(0.1, 5.9, 20, dtype=np.float32))
    O = np.stack([xs.reshape(-1), ys.reshape(-1), np.full(xs.size, 9.0, np.float32)], 1)
    D = np.broadcast_to(np.asarray([0.0, 0.0, -1.0], np.float32), O.shape)
    got = both(sc, tb.make_rays(O, D))
    hit = got["t"] < 1e30
    layers = set((got["prim"][hit] // 3).tolist())
    assert len(layers) >= 3 and int(hit.sum()) > 100, (layers, int(hit.sum()))       # closest hits in three leaves or more: those children were entered
    # the same from below (+z): the near / far order of the other octant
    O2 = O.copy(); O2[:, 2] = -3.0
    both(sc, tb.make_rays(O2, -D))
    sc.free()


TRI = ((0.0, 0.0, 2.0), (1.0, 0.0, 2.0), (0.0, 1.0, 2.0))       # in the plane z = 2: u along x, v along y, exact in fp32


def edge_bvh2():
    """Four triangles under a BVH2 by hand: root -> two leaves of two triangles, the leaf boxes PADDED well beyond their triangles.  Rays through a vertex or along
    an edge of TRI travel along +z in the faces of TRI's own bounding box: with tight boxes they sit on the knife edge of the BOX tests, where the per-lane and the
    packet kernel may part ways (on the parent commit they do, for the vertices (1, 0) and (0, 1)); padded, only the triangle test sees the edge."""
    tris = [TRI,
            ((0.25, 0.0, 3.0), (0.25, 1.0, 3.0), (0.25, 0.0, 4.0)),           # in the plane x = 0.25: edge-on for the rays below that travel along +z at x = 0.25
            ((0.0, 0.0, 6.0), (2.0, 0.0, 6.0), (0.0, 2.0, 6.0)),              # a backstop behind both
            ((3.0, 3.0, 2.0), (4.0, 3.0, 2.0), (3.0, 4.0, 2.0))]              # off to the side
    verts = np.zeros((12, 4), np.float32)
    verts[:, :3] = np.asarray(tris, np.float32).reshape(-1, 3)
    nodes = np.zeros((4, 8), np.float32)
    u = nodes.view(np.uint32)
    for i, lo, hi, left_first, count in ((2, (-1.0, -1.0, 1.5), (2.0, 2.0, 4.5), 0, 2), (3, (-1.0, -1.0, 1.5), (5.0, 5.0, 6.5), 2, 2),
                                         (0, (-1.0, -1.0, 1.5), (5.0, 5.0, 6.5), 2, 0)):
        nodes[i, 0:3] = lo; nodes[i, 4:7] = hi
        u[i, 3] = left_first; u[i, 7] = count
    return nodes, np.arange(4, dtype=np.uint32), verts


def edge_rays():
    step = 2.0 ** -20
    pts = [(0.25, 0.25), (0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (0.5, 0.0), (0.0, 0.5), (0.5, 0.5), (0.25, 0.75),      # inside; the vertices; v = 0, u = 0, u + v = 1
           (-step, 0.5), (0.5, -step), (0.5 + step, 0.5), (0.25, 0.5), (3.25, 3.25), (5.2, 5.2), (1.5, 1.5)]
    O = [(x, y, 0.0) for x, y in pts]
    D = [(0.0, 0.0, 1.0)] * len(pts)
    O += [(x, y, 8.0) for x, y in pts]; D += [(0.0, 0.0, 1.0)] * len(pts)           # every triangle behind the origin: t < 0
    O += [(-1.0, 0.25, 2.0), (-1.0, 0.25, 2.0)]; D += [(1.0, 0.0, 0.0), (1.0, 0.0, 5e-7)]      # in the plane of TRI, and nearly: |a| < 1e-6
    O = np.asarray(O, np.float32); D = np.asarray(D, np.float32)
    reps = 3                                                                          # 96 rays: one full chunk and a partial one
    return np.tile(O, (reps, 1)), np.tile(D, (reps, 1))


@pytest.mark.gpu
def test_flat_triangle_test_edge_cases(ctx):
    sc = tb.BVH8_CWBVH(ctx).ConvertFromBVH2(*edge_bvh2())
    O, D = edge_rays()
    fresh = both(sc, tb.make_rays(O, D, normalize=False))
    assert fresh["t"][0] == np.float32(2.0) and all(fresh["t"][k] == np.float32(2.0) for k in range(1, 8)), fresh["t"][:8]      # vertices and edges are hits
    assert fresh["t"][8] != np.float32(2.0) and fresh["t"][9] != np.float32(2.0) and fresh["t"][10] != np.float32(2.0)          # one step outside is not
    # one octant per chunk here; the same rays with every other one looking down from z = 8 instead: mixed chunks
    O2, D2 = O.copy(), D.copy()
    O2[1::2, 2] = 8.0; D2[1::2] = (0.0, 0.0, -1.0)
    both(sc, tb.make_rays(O2, D2, normalize=False))
    # not fresh: t stored in the ray equal to the true distance (inclusive: still a hit), one ulp short of it, and closer than any triangle
    for tmax in (np.float32(2.0), np.nextafter(np.float32(2.0), np.float32(0.0)), np.float32(0.5)):
        pre = both(sc, tb.make_rays(O, D, tmax=tmax, normalize=False))
        if tmax == np.float32(2.0):
            assert pre["prim"][0] == fresh["prim"][0] and pre["t"][0] == np.float32(2.0)
        else:
            assert np.all(pre["t"][:12] == tmax)                                       # nothing closer: the records keep what they came with
    sc.free()


@pytest.mark.gpu
def test_not_fresh_launch_with_stored_hits_closer_than_any_triangle(soup, soup_rays):
    rays = soup_rays[64 * 40:64 * 40 + 64 * 9 + 7].copy()
    soup.set_variant(72)
    first = soup.Intersect(rays.copy())
    hit = first["t"] < 1e30
    assert int(hit.sum()) > 50
    pre = rays.copy()
    pre["t"] = np.where(hit, first["t"] * np.float32(0.25), np.float32(1e-3)).astype(np.float32)       # in front of everything
    got = both(soup, pre)
    assert np.array_equal(got["t"], pre["t"])
    pre["t"] = np.where(hit, first["t"], np.float32(1e30)).astype(np.float32)                           # exactly at the true hit: found again (inclusive)
    got = both(soup, pre)
    assert np.array_equal(got["t"][hit], first["t"][hit]) and np.array_equal(got["prim"][hit], first["prim"][hit])
