"""The two device LBVH builders that test_double_anim_gpu.py::test_tree_validity does not reach, held byte for byte to the numpy restatement
(tests/lbvh_ref.py): TLAS.RebuildOnDevice with its default builder (30-bit keys, Karras ids kept, Aila-Laine records) and
SphereBVH.BuildOnDevice(builder="lbvh") (63-bit keys, BVH2 numbering, ranges of at most max_leaf spheres collapsed to a leaf), which shares
its key, topology and bottom-up kernels with the triangle build.  Centres and quantisation are computed in numpy float32, as the kernels do."""
import numpy as np
import pytest

import lbvh_ref
import tinybvh_amd as tb
from tinybvh_amd import scenes
from test_tlas import grid_instances

pytestmark = pytest.mark.gpu

HALF = np.float32(0.5)


@pytest.fixture(scope="module")
def blas(ctx):
    return [tb.BVH_GPU(ctx).Build(scenes.soup(100, seed=2))]


@pytest.fixture(scope="module")
def grid1000():
    inst = grid_instances(10, 0.5, 4)
    inst.flags.writeable = False
    return inst


def tlas_cases():
    return [(str(n), n, False) for n in (1, 2, 3, 64, 65, 1000)] + [("27 in equal pairs", 27, True)]


@pytest.mark.parametrize("case", tlas_cases(), ids=[c[0] for c in tlas_cases()])
def test_tlas_rebuild_is_the_reference_tree(ctx, blas, grid1000, case):
    _, n, dup = case
    inst = grid1000[:n].copy()
    if dup:
        inst["transform"][1::2] = inst["transform"][0:26:2]   # the odd instances copy the even ones: equal boxes, equal keys
    tlas = tb.TLAS(ctx).Build(inst, blas)
    tlas.RebuildOnDevice()
    nodes, idx, got = tlas.Download()
    lo, hi = got["aabbMin"], got["aabbMax"]
    assert lo.dtype == np.float32 and np.isfinite(lo).all() and np.isfinite(hi).all()
    if dup:
        assert np.array_equal(lo[1::2], lo[0:26:2]) and np.array_equal(hi[1::2], hi[0:26:2])
    want_nodes, want_idx = lbvh_ref.tlas_nodes(HALF * (lo + hi), lo, hi)
    assert np.array_equal(idx, want_idx)
    assert nodes.shape == want_nodes.shape and nodes.tobytes() == want_nodes.tobytes(), np.nonzero((nodes != want_nodes).any(1))[0][:8].tolist()
    tlas.free()


def sphere_sets():
    rng = np.random.default_rng(11)
    for n in (1, 2, 3, 4, 5, 63, 64, 65, 257):
        s = np.empty((n, 4), np.float32)
        s[:, :3] = rng.uniform(-10, 10, (n, 3)); s[:, 3] = rng.uniform(0.05, 0.6, n)
        yield str(n), s
    yield "700 identical", np.tile(np.array([[1.5, -2.25, 3.0, 0.5]], np.float32), (700, 1))
    two = np.empty((200, 4), np.float32)
    two[:, :3] = rng.uniform(-1, 1, (200, 3)); two[100:, :3] += np.float32(1e6); two[:, 3] = 0.25
    yield "two clusters 1e6 apart", two


SPHERES = dict(sphere_sets())


@pytest.mark.parametrize("max_leaf", [1, 4])
@pytest.mark.parametrize("name", list(SPHERES))
def test_sphere_lbvh_is_the_reference_tree(ctx, name, max_leaf):
    s = SPHERES[name]
    sc = tb.SphereBVH(ctx).BuildOnDevice(s, builder="lbvh", max_leaf=max_leaf)
    nodes, idx, _ = sc.Download()
    lo, hi = s[:, :3] - s[:, 3:4], s[:, :3] + s[:, 3:4]   # (sah_split.h: sphere_box)
    assert lo.dtype == np.float32
    want, want_idx = lbvh_ref.bvh2_nodes(HALF * (lo + hi), lo, hi, max_leaf)
    assert np.array_equal(idx, want_idx)
    assert max(want) < nodes.shape[0]
    for slot, rec in want.items():   # every node the root reaches (what lies under a collapsed range is written but never read)
        assert np.array_equal(nodes[slot], rec), (slot, nodes[slot].tolist(), rec.tolist())
    if s.shape[0] > max_leaf:
        assert any(rec[7] == 0 for rec in want.values())
    sc.free()
