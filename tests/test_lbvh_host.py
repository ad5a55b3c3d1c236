"""The LBVH core the device builders share (tinybvh_amd/csrc/lbvh.h), run on the host through the debug entries: the Karras range search
against a top-down definition of the same tree that is written without the search, the ordered float encoding, and the scratch carving."""
import numpy as np
import pytest

import lbvh_ref
from tinybvh_amd import lib

SIZES = (2, 3, 4, 5, 63, 64, 65, 257, 700)
# kind -> n unsorted keys: one value (all ties), three values, n values, and the whole 30-, 63- and 64-bit ranges
KINDS = {
    "1 value": lambda rng, n: np.full(n, 5, np.uint64),
    "3 values": lambda rng, n: rng.integers(0, 3, n, dtype=np.uint64),
    "n values": lambda rng, n: rng.integers(0, n, n, dtype=np.uint64),
    "30 bits": lambda rng, n: rng.integers(0, 1 << 30, n, dtype=np.uint64),
    "63 bits": lambda rng, n: rng.integers(0, 1 << 63, n, dtype=np.uint64),
    "64 bits": lambda rng, n: rng.integers(0, 1 << 64, n, dtype=np.uint64, endpoint=False),
}


def device_topology(keys: np.ndarray, key_bits: int) -> np.ndarray:
    keys = np.ascontiguousarray(keys, np.uint64)
    out = np.zeros((keys.size - 1, 4), np.uint32)
    assert lib.tbvh_debug_lbvh_topology(keys.ctypes.data, keys.size, key_bits, out.ctypes.data) == 0, lib.tbvh_last_error().decode()
    return out


def top_down(keys) -> np.ndarray:
    """The tree by its definition: every sorted key is followed by its position, (key << 32) | position; a range [lo, hi] splits at the highest
    bit in which its first and last such keys differ, gamma being the last position that agrees with lo in that bit.  The root is node 0 over
    [0, n - 1]; a part of one position g is leaf g (id n - 1 + g), a longer left part is interior node gamma, a longer right part gamma + 1."""
    n = len(keys)
    aug = [(int(k) << 32) | p for p, k in enumerate(keys)]
    out = np.zeros((n - 1, 4), np.uint32)
    stack = [(0, 0, n - 1)]
    while stack:
        node, lo, hi = stack.pop()
        bit = (aug[lo] ^ aug[hi]).bit_length() - 1
        gamma = max(p for p in range(lo, hi) if (aug[p] ^ aug[lo]) >> bit == 0)
        left = n - 1 + gamma if lo == gamma else gamma
        right = n + gamma if hi == gamma + 1 else gamma + 1
        out[node] = (left, right, lo, hi)
        if lo != gamma:
            stack.append((gamma, lo, gamma))
        if hi != gamma + 1:
            stack.append((gamma + 1, gamma + 1, hi))
    return out


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("n", SIZES)
def test_topology_is_the_top_down_tree(n, kind, seed):
    keys = np.sort(KINDS[kind](np.random.default_rng(1000 * seed + n), n))
    widths = (32, 64) if kind in ("1 value", "3 values", "n values", "30 bits") else (64,)
    want = top_down(keys)
    for key_bits in widths:
        got = device_topology(keys, key_bits)
        assert np.array_equal(got, want), (key_bits, np.nonzero((got != want).any(1))[0][:8].tolist())
    ref = np.array(lbvh_ref.karras([int(k) for k in keys], 64), np.uint32)   # the tests' own restatement of the search agrees too
    assert np.array_equal(ref, want)


@pytest.mark.parametrize("key_bits", [32, 64])
def test_two_equal_keys(key_bits):
    assert device_topology(np.array([9, 9], np.uint64), key_bits).tolist() == [[1, 2, 0, 1]]


def test_low_words_are_the_32_bit_keys():
    keys = np.sort(np.random.default_rng(3).integers(0, 1 << 30, 100, dtype=np.uint64))
    junk = keys | (np.random.default_rng(4).integers(1, 1 << 31, 100, dtype=np.uint64) << np.uint64(32))
    assert np.array_equal(device_topology(junk, 32), device_topology(keys, 32))


def test_topology_refusals():
    out = np.zeros(4, np.uint32); k = np.zeros(2, np.uint64)
    assert lib.tbvh_debug_lbvh_topology(k.ctypes.data, 1, 64, out.ctypes.data) != 0
    assert lib.tbvh_debug_lbvh_topology(k.ctypes.data, 2, 48, out.ctypes.data) != 0
    assert lib.tbvh_debug_lbvh_topology(None, 2, 64, out.ctypes.data) != 0


@pytest.mark.parametrize("bits", [32, 64])
def test_ordered_encoding(bits):
    tiny = [1e-45, 1e-39] if bits == 32 else [5e-324, 1e-310]   # denormals of the format
    pos = [0.0] + tiny + [1e-30, 1.0, 1.5, 1e30, np.inf]
    v = np.array([-x for x in reversed(pos)] + pos, np.float64)
    assert np.signbit(v[len(pos) - 1]) and not np.signbit(v[len(pos)])   # ... -0, +0 ...
    enc = np.zeros(v.size, np.uint64); dec = np.zeros(v.size, np.float64)
    assert lib.tbvh_debug_lbvh_ordered(v.ctypes.data, v.size, bits, enc.ctypes.data, dec.ctypes.data) == 0
    assert (enc[1:] > enc[:-1]).all(), enc.tolist()                    # monotone, -0 below +0
    if bits == 32:
        assert (enc < (1 << 32)).all()
        assert np.array_equal(dec.astype(np.float32).view(np.uint32), v.astype(np.float32).view(np.uint32))
    else:
        assert np.array_equal(dec.view(np.uint64), v.view(np.uint64))
    # the bounds as reset_centre_bounds leaves them decode to "no centre yet": every encoded minimum is below, every maximum above
    assert enc.max() < (1 << bits) - 1 and enc.min() > 0


def scratch(n, sort_temp, scan_temp):
    out = np.zeros(6, np.uint64)
    assert lib.tbvh_debug_build_scratch_bytes(n, sort_temp, scan_temp, out.ctypes.data) == 0
    return out


def test_scratch_totals():
    sizes = [1, 2, 63, 64, 65, 1000, 4096, 4097, 100_000, 3_000_000]
    totals = np.stack([scratch(n, 4096, 1024) for n in sizes])
    assert (totals % 256 == 0).all() and (totals[0] >= 1024).all()
    assert (totals[1:] >= totals[:-1]).all()                      # monotone in n
    assert (totals[-1] > totals[0]).all() and (totals[5] > totals[0]).all()
    more = np.stack([scratch(n, 8192, 1024) for n in sizes])      # hipcub's temporary bytes are a part like the others
    assert (more >= totals).all() and (more[:, :5] == totals[:, :5] + 4096).all() and (more[:, 5] == totals[:, 5]).all()
    # the fp64 TLAS: keys 8 + 8, values 4 + 4, parent and slot 8 + 8, flags 4, transforms 128 bytes per instance, 64 bytes of bounds
    n = 4096
    assert scratch(n, 0, 0)[3] == n * (8 + 8 + 4 + 4 + 8 + 8 + 4 + 128) + 256
