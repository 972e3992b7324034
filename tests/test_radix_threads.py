"""K2's scatter in its two forms: 256 threads with 32 keys per lane, and 512 threads with 16 (the same
8192-key tile; MTB_RADIX_THREADS, read per sort). Wave w ranks the tile's keys [w * slice, (w + 1) * slice)
in input order and the waves are placed in w order in both, so the two must return the same arrays: numpy's
stable argsort of the bit field, the values being the input positions. The 512-thread form keeps its wave
histograms in 16 bits; a wave's digit count reaches 1024 and a tile position 8191 when one digit takes a
whole tile.

The digit side arrays (a pass's scatter writes the next pass's digit of every key) are not reachable from
mtb_sort_pairs: one paired batch with more than two tiles of kept query k-mers is classified under each
value of the knob and compared with the oracle at every stage."""
import numpy as np
import pytest

from metabuli_work_amd import synth
from metabuli_work_amd._lib import lib
from tests.test_radix import sort_field

SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193, 16384, 3 * 8192 + 511]
RANGES = [(36, 60), (0, 8)]  # the query sort's three passes; one pass on the lowest digit
POPULATIONS = ["equal", "alternating", "descending", "all_digits", "duplicates"]
FORMS = ("256", "512")


def make_keys(rng, n, lo, hi, population):
    """Keys whose bits [lo, hi) follow `population`; the bits outside are random and must be ignored."""
    width = hi - lo
    i = np.arange(n, dtype=np.uint64)
    if population == "equal":
        f = np.full(n, 0xA5C3E1 & ((1 << width) - 1), np.uint64)
    elif population == "alternating":  # two values that differ in every digit, lane by lane
        f = np.where(i & np.uint64(1), np.uint64(0xFEFDFC), np.uint64(0x010203))
    elif population == "descending":
        f = np.uint64(n - 1) - i
    elif population == "all_digits":  # every byte of the field is a bijection of i mod 256: 32 of each per tile
        d = i & np.uint64(0xFF)
        f = d | (((d * np.uint64(7) + np.uint64(3)) & np.uint64(0xFF)) << np.uint64(8)) | ((np.uint64(255) - d) << np.uint64(16))
    else:
        f = rng.integers(0, 1 << width, 300, dtype=np.uint64)[rng.integers(0, 300, n)]
    mask = np.uint64(((1 << width) - 1) << lo)
    return (rng.integers(0, 1 << 64, n, dtype=np.uint64) & ~mask) | ((f.astype(np.uint64) << np.uint64(lo)) & mask)


def sort_pairs(keys, lo, hi):
    n = len(keys)
    vals = np.arange(n, dtype=np.uint32)
    ko = np.full(n, 0x5A5A5A5A5A5A5A5A, np.uint64)
    vo = np.full(n, 0xA5A5A5A5, np.uint32)
    rc = lib().mtb_sort_pairs(0, keys.ctypes.data, vals.ctypes.data, n, lo, hi, ko.ctypes.data, vo.ctypes.data)
    assert rc == 0, lib().mtb_last_error().decode()
    return ko, vo


def test_populations_are_what_they_claim():
    """CPU: one digit takes the whole tile; 256 digits, 32 times each per tile, in every pass's byte."""
    rng = np.random.default_rng(1)
    assert len(np.unique(sort_field(make_keys(rng, 8192, 36, 60, "equal"), 36, 60))) == 1
    f = sort_field(make_keys(rng, 8192, 36, 60, "all_digits"), 36, 60)
    for b in range(3):
        assert (np.bincount(((f >> np.uint64(8 * b)) & np.uint64(0xFF)).astype(np.int64), minlength=256) == 32).all()
    f = sort_field(make_keys(rng, 8192, 36, 60, "alternating"), 36, 60)
    assert set(f[:4].tolist()) == {0x010203, 0xFEFDFC} and f[0] != f[1]
    f = sort_field(make_keys(rng, 8193, 0, 8, "descending"), 0, 8).astype(np.int64)
    assert ((f[:-1] - f[1:]) % 256 == 1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("lo,hi", RANGES)
@pytest.mark.parametrize("n", SIZES)
def test_both_forms_sort_stably(monkeypatch, n, lo, hi):
    rng = np.random.default_rng(100 * n + lo)
    for pop in POPULATIONS:
        keys = make_keys(rng, n, lo, hi, pop)
        order = np.argsort(sort_field(keys, lo, hi), kind="stable")
        got = {}
        for form in FORMS:
            monkeypatch.setenv("MTB_RADIX_THREADS", form)
            ko, vo = sort_pairs(keys, lo, hi)
            assert np.array_equal(vo, order.astype(np.uint32)), f"{pop}, {form} threads: values"
            assert np.array_equal(ko, keys[order]), f"{pop}, {form} threads: keys"
            got[form] = (ko, vo)
        assert np.array_equal(got["256"][0], got["512"][0]) and np.array_equal(got["256"][1], got["512"][1])


@pytest.fixture(scope="module")
def paired_batch(make_db):
    """1200 pairs of 150 bases from the fmt2 genomes, their oracle stages computed once for both forms."""
    from tests import oracle_ctypes as oc
    from tests.test_batch_shapes import Case, _oracle_stages
    from tests.test_gpu_parity import _params
    db_dir, taxo, gen = make_db("fmt2")
    reads = synth.make_reads(gen, 1200, seed=19)
    par = _params(db_dir, 2)
    odb = oc.OracleDb(db_dir)
    o = _oracle_stages(odb, par, reads)
    odb.close()
    return db_dir, par, Case("k2_forms", reads), o


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_digit_arrays_both_forms_against_oracle(paired_batch, monkeypatch, form):
    """The query sort as a batch runs it (histograms from the digit side arrays, each scatter writing
    the next pass's digits) over more than two full tiles and a partial one."""
    from metabuli_work_amd.classifier import Classifier
    from tests.test_batch_shapes import _compare
    monkeypatch.setenv("MTB_RADIX_THREADS", form)
    db_dir, par, case, o = paired_batch
    r = case.reads
    with Classifier(par, db_dir=db_dir) as clf:
        br = clf.classify_batch(r.seq1, r.off1, r.seq2, r.off2, keep_stages=True)
        kept = clf.stats()["query_kmers"]
        assert kept > 2 * 8192 and kept % 8192 != 0, kept
        assert int(o[2]["is_classified"].sum()) > 600
        bad = _compare(clf, case, br, par, db_dir, o, {})
    assert not bad, "\n".join(bad)
