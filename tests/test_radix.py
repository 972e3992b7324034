"""K2's LSD radix sort is stable: the lane-mask ranking relies on one wave's LDS operations
completing in program order, and every pass after the first must keep equal digits in input order for
the 24-bit prefix order to come out right. Checked directly through mtb_sort_pairs: keys over many
tiles with few distinct sort prefixes (long runs of equal digits in every tile), distinct values = the
input positions, so the output values must be numpy's stable argsort of the prefix exactly. Both tile
sizes (MTB_RADIX_TILE), both rankings (MTB_RADIX_ORRANK), partial last tiles.

The 64-bit-value instantiation (mtb_sort_pairs64: the DB builder's two sorts and K6's work lists) is
held to the contract written at the entry (mtb_api.hip):
  * sort key = bits [lo, min(64, lo + 8 * ceil((hi - lo) / 8))) — whole 8-bit digits from lo;
  * stable;
  * filter drops exactly the pairs whose whole key is ~0, in the first pass;
  * gen_vals makes the values the input positions (never together with filter: no 64-bit call
    site does that, and the entry refuses it).
Expected output everywhere: numpy's stable argsort of that bit field over the kept pairs."""
import numpy as np
import pytest

from metabuli_work_amd._lib import lib

LO, HI = 36, 60  # the query sort's prefix (kQuerySortLo / kQuerySortHi)


def sort_pairs(keys, lo=LO, hi=HI):
    n = len(keys)
    vals = np.arange(n, dtype=np.uint32)
    ko = np.zeros(n, np.uint64)
    vo = np.zeros(n, np.uint32)
    rc = lib().mtb_sort_pairs(0, keys.ctypes.data, vals.ctypes.data, n, lo, hi, ko.ctypes.data, vo.ctypes.data)
    assert rc == 0, lib().mtb_last_error().decode()
    return ko, vo


@pytest.mark.gpu
@pytest.mark.parametrize("env", ["", "MTB_RADIX_TILE=4096", "MTB_RADIX_ORRANK=0", "MTB_RADIX_FULLTILE=0"])
@pytest.mark.parametrize("n,distinct", [(8192 * 12 + 77, 5), (100_003, 300), (8191, 2), (4096 * 3, 1)])
def test_radix_sort_stable(monkeypatch, env, n, distinct):
    if env:
        k, v = env.split("=")
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(n + distinct)
    prefixes = rng.integers(0, 1 << (HI - LO), distinct, dtype=np.uint64)
    keys = (prefixes[rng.integers(0, distinct, n)] << np.uint64(LO)) | rng.integers(0, 1 << LO, n, dtype=np.uint64)
    keys |= rng.integers(0, 16, n, dtype=np.uint64) << np.uint64(HI)  # bits above the range: ignored
    ko, vo = sort_pairs(keys)
    order = np.argsort((keys >> np.uint64(LO)) & np.uint64((1 << (HI - LO)) - 1), kind="stable")
    assert np.array_equal(vo, order.astype(np.uint32))
    assert np.array_equal(ko, keys[order])


# ---- the 64-bit-value sort ------------------------------------------------------------------------
SENTINEL = np.uint64(0xFFFFFFFFFFFFFFFF)
SIZES = [0, 1, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193, 3 * 8192, 5 * 8192 + 77]
# the builder's species sorts (32, 40 / 48 / 56 / 64) and its value sort (0, 64); K6's (32, 40); the query
# prefix; the lowest and the highest digit alone; two ranges whose width is no multiple of 8: (0, 20)
# sorts on bits [0, 24) (K6's longest_first passes an arbitrary bit count), (54, 64) has a second digit
# that starts at bit 62 and is zero-extended past bit 63
RANGES = [(0, 64), (32, 40), (32, 48), (32, 56), (32, 64), (0, 8), (56, 64), (36, 60), (0, 20), (54, 64)]
KNOBS = ["", "MTB_RADIX_TILE=4096", "MTB_RADIX_ORRANK=0", "MTB_RADIX_FULLTILE=0"]
POPULATIONS = ["equal", 2, 5, 300, "uniform"]


def sort_field(keys, lo, hi):
    """The bits the passes of [lo, hi) sort on: whole 8-bit digits from lo, cut at bit 64."""
    top = min(64, lo + 8 * ((hi - lo + 7) // 8))
    f = keys >> np.uint64(lo)
    if top - lo < 64:
        f = f & np.uint64((1 << (top - lo)) - 1)
    return f


def position_values(n):
    """A distinct 64-bit value per input position whose two 32-bit words differ (an odd multiplier is a
    bijection mod 2^64), so a truncated, half-swapped or misplaced value shows."""
    with np.errstate(over="ignore"):
        v = (np.arange(n, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
    assert n == 0 or ((v >> np.uint64(32)) != (v & np.uint64(0xFFFFFFFF))).all()
    return v


def make_keys(rng, n, lo, hi, population):
    """Keys whose sort field takes `population` distinct values (or is uniform), with random bits outside
    the field, which the sort must ignore."""
    top = min(64, lo + 8 * ((hi - lo + 7) // 8))
    width = top - lo
    full = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    if population == "uniform":
        return full
    k = 1 if population == "equal" else population
    fields = rng.integers(0, 1 << width, k, dtype=np.uint64) if width < 64 else rng.integers(0, 1 << 64, k, dtype=np.uint64)
    f = fields[rng.integers(0, k, n)]
    mask = np.uint64(((1 << width) - 1) << lo)
    return (full & ~mask) | ((f << np.uint64(lo)) & mask)


def sort_pairs64(keys, vals, lo, hi, filt=False, gen=False):
    n = len(keys)
    keys = np.ascontiguousarray(keys, np.uint64)
    ko = np.full(n, 0x5A5A5A5A5A5A5A5A, np.uint64)
    vo = np.full(n, 0xA5A5A5A5A5A5A5A5, np.uint64)
    kept = np.zeros(1, np.uint64)
    vp = None if gen else np.ascontiguousarray(vals, np.uint64).ctypes.data
    rc = lib().mtb_sort_pairs64(0, keys.ctypes.data, vp, n, lo, hi, int(filt), int(gen), ko.ctypes.data,
                                vo.ctypes.data, kept.ctypes.data)
    assert rc == 0, lib().mtb_last_error().decode()
    k = int(kept[0])
    assert k <= n
    # nothing is written past the kept pairs
    assert (ko[k:] == np.uint64(0x5A5A5A5A5A5A5A5A)).all() and (vo[k:] == np.uint64(0xA5A5A5A5A5A5A5A5)).all()
    return ko[:k], vo[:k]


def check_sort64(keys, lo, hi, filt=False, gen=False):
    n = len(keys)
    vals = np.arange(n, dtype=np.uint64) if gen else position_values(n)
    ko, vo = sort_pairs64(keys, vals, lo, hi, filt, gen)
    keep = np.flatnonzero(keys != SENTINEL) if filt else np.arange(n)
    order = keep[np.argsort(sort_field(keys[keep], lo, hi), kind="stable")]
    assert len(ko) == len(order), (len(ko), len(order))
    assert np.array_equal(ko, keys[order])
    assert np.array_equal(vo, vals[order])


def set_knob(monkeypatch, env):
    if env:
        k, v = env.split("=")
        monkeypatch.setenv(k, v)


@pytest.mark.gpu
@pytest.mark.parametrize("lo,hi", RANGES)
@pytest.mark.parametrize("n", SIZES)
def test_sort64_sizes_ranges_populations(n, lo, hi):
    """Every size (partial and full last tiles at both tile sizes) at every range, for every key
    population; 64-bit values carried through all passes."""
    rng = np.random.default_rng(1000 * n + 64 * lo + hi)
    for pop in POPULATIONS:
        check_sort64(make_keys(rng, n, lo, hi, pop), lo, hi)


@pytest.mark.gpu
@pytest.mark.parametrize("env", KNOBS)
@pytest.mark.parametrize("n", [257, 4095, 4097, 8192, 8193, 5 * 8192 + 77])
def test_sort64_knobs(monkeypatch, env, n):
    """The knob sets of test_radix_sort_stable on a reduced cross product: the builder's two ranges and
    a rounded one, few and many distinct fields, plain / filter / gen_vals."""
    set_knob(monkeypatch, env)
    rng = np.random.default_rng(7 * n + len(env))
    for lo, hi in [(0, 64), (32, 48), (0, 20)]:
        for pop in (2, 300, "uniform"):
            keys = make_keys(rng, n, lo, hi, pop)
            check_sort64(keys, lo, hi)
            check_sort64(keys, lo, hi, gen=True)
            keys[rng.random(n) < 0.3] = SENTINEL
            check_sort64(keys, lo, hi, filt=True)


def sentinel_patterns(rng, n, tile):
    """(name, mask of sentinel positions) for a sort of n keys in tiles of `tile`."""
    n_tiles = (n + tile - 1) // tile
    none = np.zeros(n, bool)
    out = [("none", none), ("all", np.ones(n, bool))]
    first = none.copy()
    first[:tile] = True
    out.append(("first_tile", first))
    last = none.copy()
    last[(n_tiles - 1) * tile:] = True
    out.append(("last_tile", last))
    mid = none.copy()
    m = n_tiles // 2
    mid[m * tile:(m + 1) * tile] = True
    span = np.flatnonzero(mid)
    mid[span[int(rng.integers(0, len(span)))]] = False  # all but one element of a middle tile
    out.append(("middle_tile_but_one", mid))
    out.append(("random_30", rng.random(n) < 0.3))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("env", ["", "MTB_RADIX_TILE=4096"])
@pytest.mark.parametrize("n", [1, 255, 257, 4095, 4096, 4097, 8191, 8192, 8193, 3 * 8192, 5 * 8192 + 77])
def test_sort64_filter(monkeypatch, env, n):
    """filter as the builder (32 .. 32 + 8k) and K6 (32 .. 40) run it: exactly the keys equal to ~0 are
    dropped, the kept pairs stay stable. Keys that only look like the sentinel inside the range (field
    all ones, or one bit short of ~0) are kept."""
    set_knob(monkeypatch, env)
    tile = 4096 if env else 8192
    rng = np.random.default_rng(31 * n + len(env))
    for lo, hi in [(32, 40), (32, 48), (32, 56), (32, 64), (0, 64)]:
        for name, mask in sentinel_patterns(rng, n, tile):
            keys = make_keys(rng, n, lo, hi, 5 if name != "random_30" else "uniform")
            near = rng.random(n) < 0.05
            keys[near] |= np.uint64(0xFFFFFFFF00000000)  # the whole high word ones, the low word not
            if n > 3:
                keys[int(rng.integers(0, n))] = np.uint64(0xFFFFFFFFFFFFFFFE)
                keys[int(rng.integers(0, n))] = np.uint64(0x7FFFFFFFFFFFFFFF)
            keys[mask] = SENTINEL
            check_sort64(keys, lo, hi, filt=True)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_sort64_gen_vals(n):
    """gen_vals as K6's longest_first runs it (bits [0, bits), no filter): the values are the input
    positions, so the output values are the stable argsort itself. The input value array is not read."""
    rng = np.random.default_rng(77 + n)
    for lo, hi in [(0, 8), (0, 20), (0, 24), (0, 32), (0, 64), (32, 40)]:
        for pop in ("equal", 5, 300, "uniform"):
            check_sort64(make_keys(rng, n, lo, hi, pop), lo, hi, gen=True)


@pytest.mark.gpu
def test_sort64_refuses_filter_with_gen_vals():
    keys = np.arange(16, dtype=np.uint64)
    out = np.zeros(16, np.uint64)
    kept = np.zeros(1, np.uint64)
    rc = lib().mtb_sort_pairs64(0, keys.ctypes.data, None, 16, 0, 8, 1, 1, out.ctypes.data, out.ctypes.data,
                                kept.ctypes.data)
    assert rc < 0


def test_sort_field_contract():
    """The expectation's own bit field (CPU): widths round up to whole digits from lo and stop at bit 64."""
    k = np.array([0xFEDCBA9876543210], np.uint64)
    assert int(sort_field(k, 0, 20)[0]) == 0x543210
    assert int(sort_field(k, 0, 24)[0]) == 0x543210
    assert int(sort_field(k, 32, 40)[0]) == 0x98
    assert int(sort_field(k, 54, 64)[0]) == 0xFEDCBA9876543210 >> 54
    assert int(sort_field(k, 0, 64)[0]) == 0xFEDCBA9876543210
    assert int(sort_field(k, 36, 60)[0]) == (0xFEDCBA9876543210 >> 36) & 0xFFFFFF
