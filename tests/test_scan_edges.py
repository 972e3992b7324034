"""The device-wide exclusive scan at its edges (mtb_scan_u32: the scan alone, host arrays).

A tile is 4096 elements. Full tiles are read and written as 16-B vectors, four stretches of 256
quads per tile; the last, partial tile takes the guarded element-wise path, so the sizes below put
the seam between the two paths at every place it can fall: no tile, one element, a tile less one,
exactly one tile, a tile and one, two tiles and one, three tiles and one. Both output widths run
every case: 64 bits (every per-read offset array) and 32 bits (the radix sort's tile offsets, whose
totals stay below 2^32). The reference is numpy's cumsum in 64 bits.
"""
import numpy as np
import pytest

from metabuli_work_amd._lib import check, lib

pytestmark = pytest.mark.gpu

TILE = 4096
SIZES = [0, 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 3 * TILE + 1]


def scan(x, bits):
    x = np.ascontiguousarray(x, np.uint32)
    out = np.full(len(x) + 1, 0xA5A5A5A5, np.uint64 if bits == 64 else np.uint32)
    check(lib().mtb_scan_u32(0, x.ctypes.data if len(x) else None, len(x), bits, out.ctypes.data), "mtb_scan_u32")
    return out


def expect(x):
    e = np.zeros(len(x) + 1, np.uint64)
    np.cumsum(x.astype(np.uint64), out=e[1:])
    return e


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n", SIZES)
def test_sizes(n, bits):
    rng = np.random.default_rng(n + bits)
    x = rng.integers(0, 1 << 16, n, dtype=np.uint32)  # totals below 2^32 for every size here
    e = expect(x)
    assert int(e[-1]) < 1 << 32
    assert np.array_equal(scan(x, bits).astype(np.uint64), e)


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n", [1, TILE, 3 * TILE + 1])
def test_all_zero(n, bits):
    assert not scan(np.zeros(n, np.uint32), bits).any()


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("at", [0, 255 * 4 + 3, TILE - 1, TILE, 2 * TILE + 1023, 3 * TILE])
def test_one_huge_element(at, bits):
    """One element of 2^32 - 1 among zeros: first and last of a tile, last of a stretch's first wave
    quad row, and in the partial tile; every later offset is that value, every earlier one zero."""
    x = np.zeros(3 * TILE + 1, np.uint32)
    x[at] = 0xFFFFFFFF
    got = scan(x, bits).astype(np.uint64)
    assert np.array_equal(got, expect(x))
    assert got[at] == 0 and got[at + 1] == 0xFFFFFFFF


def test_sums_past_32_bits():
    """64-bit outputs: every element 2^32 - 1, so the sums pass 2^32 inside the first tile's first
    stretch and the tile carries are past it from the second tile on."""
    x = np.full(3 * TILE + 1, 0xFFFFFFFF, np.uint32)
    got = scan(x, 64)
    assert np.array_equal(got, expect(x))
    assert int(got[-1]) == (3 * TILE + 1) * 0xFFFFFFFF


@pytest.mark.parametrize("n", [TILE, 3 * TILE + 1])
def test_total_just_below_32_bits(n):
    """32-bit outputs with a total of exactly 2^32 - 1, the largest the sort may hand it."""
    rng = np.random.default_rng(n)
    x = rng.integers(0, (1 << 32) // n - 1, n, dtype=np.uint32)
    x[n // 2] += np.uint32(0xFFFFFFFF - int(x.astype(np.uint64).sum()))
    e = expect(x)
    assert int(e[-1]) == 0xFFFFFFFF
    assert np.array_equal(scan(x, 32).astype(np.uint64), e)
    assert np.array_equal(scan(x, 64), e)


def test_bad_arguments():
    out = np.zeros(2, np.uint64)
    x = np.ones(1, np.uint32)
    assert lib().mtb_scan_u32(0, x.ctypes.data, 1, 16, out.ctypes.data) < 0
    assert lib().mtb_scan_u32(0, None, 1, 64, out.ctypes.data) < 0
    assert lib().mtb_scan_u32(0, x.ctypes.data, 1, 64, None) < 0
