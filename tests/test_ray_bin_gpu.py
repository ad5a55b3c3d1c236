"""tbvh_bin_rays_device (k_bin_count, a hipcub scan, k_bin_scatter: a counting sort of 64-byte ray records by origin cell and direction
octant) held to the key function of raygen_ref.py.  Every input record carries its own index in `prim` and `inst` and a `t` of its
own, so a lost, duplicated, torn or mixed record shows; the output must be the input permuted (bytewise `in[perm]`, or the same
multiset of rows without `perm`), in non-decreasing order of the HOST's key, with the host's count per key.  A device key that
differs from the host's for any ray breaks the order or the counts."""
import ctypes as C
import os

import numpy as np
import pytest

import raygen_ref as G
import tinybvh_amd as tb
from tinybvh_amd import rays as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F = np.float32
POISON = 0xA5
INVALID = -1   # TBVH_E_INVALID
UNIT8 = (0.0, 0.0, 0.0, 8.0, 8.0, 8.0)     # 2^b cells of a power-of-two size for b <= 3: cell boundaries are exact


def tagged(rays):
    n = rays.shape[0]
    rays["prim"] = np.arange(n, dtype=np.uint32)
    rays["inst"] = np.arange(n, dtype=np.uint32) ^ np.uint32(0xA0000000)
    rays["t"] = (np.arange(n, dtype=np.float64) * 0.5 + 1.0).astype(F)       # exact and distinct up to 2^23 rays
    rays["u"] = F(0.25); rays["v"] = F(0.5)
    return rays


def batch(n, seed, lo=(-1.0, -1.0, -1.0), hi=(9.0, 9.0, 9.0)):
    """random origins in a box a little larger than UNIT8 (so some lie outside), directions in all octants"""
    return tagged(R.random_rays(n, lo, hi, seed=seed))


def bin_on_device(ctx, rays, bounds, cell_bits, flags, with_perm=True):
    n = rays.shape[0]
    out = np.full((n + 1) * 64, POISON, np.uint8)
    perm = np.full(n + 1, 0xA5A5A5A5, np.uint32)
    d_in, d_out, d_perm = ctx.malloc(max(n, 1) * 64), ctx.malloc(out.nbytes), ctx.malloc(perm.nbytes)
    try:
        if n:
            ctx.to_device(d_in, rays)
        ctx.to_device(d_out, out); ctx.to_device(d_perm, perm)
        ctx.bin_rays(d_in, d_out, n, bounds, cell_bits, flags, d_perm if with_perm else 0)
        ctx.synchronize()
        ctx.from_device(out, d_out); ctx.from_device(perm, d_perm)
    finally:
        for p in (d_in, d_out, d_perm):
            ctx.free(p)
    assert (out[n * 64:] == POISON).all() and perm[n] == 0xA5A5A5A5, "wrote past the batch"
    if not with_perm:
        assert (perm == 0xA5A5A5A5).all()
    return out[:n * 64].copy().view(tb.RAY_DTYPE), (perm[:n].copy() if with_perm else None)


def check_binned(rays, out, perm, bounds, cell_bits, flags):
    n = rays.shape[0]
    if perm is not None:
        assert np.array_equal(np.sort(perm), np.arange(n, dtype=np.uint32)), "perm is not a permutation"
        assert out.tobytes() == rays[perm].tobytes(), "out is not in[perm]"
    else:
        assert np.array_equal(np.sort(out["prim"]), np.arange(n, dtype=np.uint32)), "a record was lost or duplicated"
        assert out[np.argsort(out["prim"], kind="stable")].tobytes() == rays.tobytes(), "a record was torn or mixed"
    bins = G.bin_count(cell_bits, flags)
    k_in, k_out = G.bin_keys(rays, bounds, cell_bits, flags), G.bin_keys(out, bounds, cell_bits, flags)
    assert int(k_in.max(initial=0)) < bins
    assert (np.diff(k_out.astype(np.int64)) >= 0).all(), "keys of out are not non-decreasing"
    assert np.array_equal(np.bincount(k_out, minlength=bins), np.bincount(k_in, minlength=bins))


def run(ctx, rays, bounds, cell_bits, flags):
    for with_perm in (True, False):
        out, perm = bin_on_device(ctx, rays, bounds, cell_bits, flags, with_perm)
        check_binned(rays, out, perm, bounds, cell_bits, flags)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 100_003])
def test_batch_sizes(ctx, n):
    run(ctx, batch(n, seed=n), UNIT8, 4, 1)


@pytest.mark.parametrize("flags", [0, 1, 2])
@pytest.mark.parametrize("cell_bits", [0, 1, 3, 6])
def test_key_forms(ctx, cell_bits, flags):
    """cell_bits 6, flags 1: 2^21 bins for 5000 rays; cell_bits 0, flags 0: one bin, a plain copy"""
    rays = batch(5000, seed=10 * cell_bits + flags)
    run(ctx, rays, UNIT8, cell_bits, flags)


def test_all_rays_in_one_bin(ctx):
    """the heaviest contention on the two atomics: 50 000 rays, one cell, one octant"""
    rays = tagged(R.random_rays(50_000, (2.51, 3.51, 4.51), (2.62, 3.62, 4.62), seed=3))
    rays["D"] = np.abs(rays["D"]) * np.array([1, -1, 1], F)
    for cell_bits, flags in ((3, 1), (6, 2)):
        assert len(np.unique(G.bin_keys(rays, UNIT8, cell_bits, flags))) == 1
        run(ctx, rays, UNIT8, cell_bits, flags)


def edge_rays():
    """Origins outside the bounds on each side, on lo, on hi and on interior cell boundaries of UNIT8, one coordinate each of NaN, +inf
    and -inf, directions with -0.0 components (not negative) — each among 300 ordinary rays."""
    inf, nan = np.inf, np.nan
    O = [[-1, 4, 4], [9, 4, 4], [4, -1, 4], [4, 9, 4], [4, 4, -1], [4, 4, 9], [-1e30, 1e30, 4],
         [0, 0, 0], [0, 5, 5], [5, 0, 5], [5, 5, 0], [8, 8, 8], [8, 3, 3], [3, 8, 3], [3, 3, 8],
         [1, 2, 3], [4, 4, 4], [7, 1, 4], [np.nextafter(F(4), F(0)), 4, np.nextafter(F(4), F(8))], [np.nextafter(F(8), F(0)), 0.5, 2],
         [nan, 4, 4], [4, nan, 4], [4, 4, nan], [inf, 4, 4], [4, inf, 4], [4, 4, inf], [-inf, 4, 4], [4, -inf, 4], [4, 4, -inf]]
    O = np.array(O, F)
    D = np.tile(np.array([[-0.0, 1.0, -1.0], [1.0, -0.0, -0.0], [-0.0, -0.0, -0.0], [-1.0, -1.0, 0.0]], F), (len(O), 1))[:len(O)]
    special = tb.make_rays(O, D, normalize=False)
    rays = np.concatenate([batch(150, seed=21), special, batch(150, seed=22)])
    return tagged(rays), slice(150, 150 + len(O))


@pytest.mark.parametrize("cell_bits,flags", [(1, 0), (3, 1), (3, 2), (6, 1)])
def test_origins_on_and_outside_the_bounds_nan_inf_and_negative_zero(ctx, cell_bits, flags):
    rays, sp = edge_rays()
    with np.errstate(invalid="ignore"):
        cells = G.bin_cells(rays["O"][sp], UNIT8, 3)
    # the host key puts them where the header says: clamped to the first / last cell, a boundary in the upper cell, NaN and -inf in cell 0, +inf in the last
    assert cells[:6].tolist() == [[0, 4, 4], [7, 4, 4], [4, 0, 4], [4, 7, 4], [4, 4, 0], [4, 4, 7]] and cells[11].tolist() == [7, 7, 7]
    assert cells[15:19].tolist() == [[1, 2, 3], [4, 4, 4], [7, 1, 4], [3, 4, 4]]
    assert cells[20:29].tolist() == [[0, 4, 4], [4, 0, 4], [4, 4, 0], [7, 4, 4], [4, 7, 4], [4, 4, 7], [0, 4, 4], [4, 0, 4], [4, 4, 0]]
    octants = G.bin_keys(rays[sp], UNIT8, 0, 1)
    assert octants[:4].tolist() == [1, 0, 0, 6]            # -0.0 counts as not negative
    run(ctx, rays, UNIT8, cell_bits, flags)


@pytest.mark.parametrize("bounds", [(0.0, 2.5, 0.0, 8.0, 2.5, 8.0), (0.0, 8.0, 0.0, 8.0, 0.0, 8.0), (3.0, 3.0, 3.0, 3.0, 3.0, 3.0)],
                         ids=["zero_extent_y", "reversed_y", "a_point"])
def test_degenerate_bounds(ctx, bounds):
    rays, _ = edge_rays()
    with np.errstate(invalid="ignore"):
        assert (G.bin_cells(rays["O"], bounds, 3)[:, 1] == 0).all()
    for flags in (0, 1):
        run(ctx, rays, bounds, 3, flags)


def test_scratch_reuse_on_one_context():
    """2^21 bins, then one bin, then 2^21 again (the histogram of the wide call must not shine through), and n growing from 1000 to
    100 003 (the key array in front of the histogram grows and moves it): a context of its own, so that the scratch starts empty."""
    ctx = tb.Context(0)
    try:
        small, big = batch(1000, seed=31), batch(100_003, seed=32)
        for rays, cell_bits, flags in ((small, 6, 1), (small, 0, 0), (small, 6, 1), (small, 3, 2), (big, 3, 2), (big, 6, 1), (small, 0, 0), (big, 5, 0)):
            run(ctx, rays, UNIT8, cell_bits, flags)
    finally:
        ctx.close()


def test_binned_batch_traces_to_the_same_hits(ctx):
    """bin -> intersect_device on the stream with no synchronisation in between; bytes 44..63 gathered back through perm are the bytes
    of the unbinned batch's trace (the library's tie rule does not depend on the order of the rays)."""
    verts = np.ascontiguousarray(np.load(os.path.join(GOLDEN, "soup_2k.npz"))["verts"], F)
    lo, hi = verts[:, :3].min(0), verts[:, :3].max(0)
    n = 20_000
    rays = R.random_rays(n, lo - 1, hi + 1, seed=41)
    sc = tb.BVH8_CWBVH(ctx).Build(verts, threads=1)
    d_in, d_out, d_perm = ctx.malloc(n * 64), ctx.malloc(n * 64), ctx.malloc(n * 4)
    try:
        ctx.to_device(d_in, rays)
        ctx.bin_rays(d_in, d_out, n, np.concatenate([lo, hi]), 4, 1, d_perm)
        sc.intersect_device(d_out, n)
        sc.intersect_device(d_in, n)
        ctx.synchronize()
        plain, binned, perm = np.zeros(n, tb.RAY_DTYPE), np.zeros(n, tb.RAY_DTYPE), np.zeros(n, np.uint32)
        ctx.from_device(plain, d_in); ctx.from_device(binned, d_out); ctx.from_device(perm, d_perm)
    finally:
        for p in (d_in, d_out, d_perm):
            ctx.free(p)
        sc.free()
    assert np.array_equal(np.sort(perm), np.arange(n, dtype=np.uint32))
    hits = (plain["t"] < G.FAR).mean()
    assert 0.1 < hits < 0.95, hits
    pb, bb = plain.view(np.uint8).reshape(n, 64), binned.view(np.uint8).reshape(n, 64)
    assert np.array_equal(bb[:, :44], rays.view(np.uint8).reshape(n, 64)[perm][:, :44])
    back = np.empty((n, 20), np.uint8)
    back[perm] = bb[:, 44:]
    assert np.array_equal(back, pb[:, 44:])


def test_refusals(ctx):
    rays = batch(256, seed=51)
    n = rays.shape[0]
    out = np.full(n * 64, POISON, np.uint8)
    d_in, d_out = ctx.malloc(n * 64), ctx.malloc(n * 64)
    try:
        ctx.to_device(d_in, rays); ctx.to_device(d_out, out)
        for args in ((d_in, d_in, n, UNIT8, 3, 1), (d_in, d_out, n, UNIT8, 7, 1), (d_in, d_out, n, UNIT8, 3, 3), (d_in, d_out, n, UNIT8, 3, 4)):
            with pytest.raises(tb.TbvhError) as e:
                ctx.bin_rays(*args)
            assert e.value.code == INVALID
        assert tb.lib.tbvh_bin_rays_device(ctx._h, C.c_void_p(d_in), C.c_void_p(d_out), n, None, 3, 1, None) == INVALID     # null bounds
        ctx.bin_rays(d_in, d_out, 0, UNIT8, 3, 1)          # n == 0: returns 0 and touches nothing
        ctx.synchronize()
        back = np.zeros_like(out); same = np.zeros(n, tb.RAY_DTYPE)
        ctx.from_device(back, d_out); ctx.from_device(same, d_in)
        assert (back == POISON).all() and same.tobytes() == rays.tobytes()
    finally:
        ctx.free(d_in); ctx.free(d_out)
    run(ctx, rays, UNIT8, 3, 1)      # the context still works
