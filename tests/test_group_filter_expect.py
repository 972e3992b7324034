"""The common-k-mer filter's fixture (tests/golden/ref_group_filter.npz, from the reference's own
filterCommonKmers) against the filter's predicate in plain numpy (tests/group_filter_cases.py): each
guards the other. No GPU."""
import numpy as np
import pytest

from tests import group_filter_cases as gc

CASES = [(cfg, db) for cfg, _, _ in gc.CONFIGS for db in gc.DBS]


@pytest.fixture(scope="module")
def fx():
    return gc.load()


@pytest.mark.parametrize("cfg,db", CASES)
def test_fixture_obeys_the_predicate(fx, cfg, db):
    v, s, p, _ = gc.extraction(fx, cfg)
    dbv = gc.db_values(fx, cfg, db)
    keep_ref, hit_pairs, kept = gc.reference_result(fx, cfg, db)
    hit, keep = gc.predicate(dbv, v, s, p)
    # the hit set is exactly the instances whose value is in the DB
    want_pairs = np.unique(np.stack([s[hit], p[hit]], 1), axis=0) if hit.any() else np.zeros((0, 2), np.uint32)
    assert np.array_equal(want_pairs, hit_pairs)
    # the kept set is exactly the instances with no hit within one nucleotide in the same read
    assert np.array_equal(gc.multiset(v[keep], s[keep], p[keep]), gc.multiset(v[keep_ref], s[keep_ref], p[keep_ref]))
    assert int(keep.sum()) == kept == int(keep_ref.sum())


def test_fixture_covers_its_cases(fx):
    v, s, p, f = gc.extraction(fx, "fmt3")
    assert (v == 0).any(), "a 12-mer of value 0"
    assert (p == 0).any()
    lens = np.array([len(a) for a in fx["seq1"]])
    assert (lens >= 6000).any() and (np.array([len(b) for b in fx["seq2"]]) == 75).any()
    for cfg, _, _ in gc.CONFIGS:
        cv, cs, cp, _ = gc.extraction(fx, cfg)
        dbv = gc.db_values(fx, cfg, "fifth")
        assert len(dbv) > max(gc.SPLITS) and (np.diff(dbv.astype(np.int64)) == 0).any()  # duplicates
        assert cv.min() in dbv and cv.max() in dbv
        hit, keep = gc.predicate(dbv, cv, cs, cp)
        assert 0.15 < hit.mean() < 0.35
        assert (hit & (cp == 0)).any() or cfg != "fmt3"  # a hit at pos 0
        # the last k-mer of the last-but-one read and the first of the last read are hits
        a, b = cs.max() - 1, cs.max()
        assert hit[cs == a][np.argmax(cp[cs == a])] and hit[cs == b][np.argmin(cp[cs == b])]
        keep_all = gc.reference_result(fx, cfg, "all")
        keep_none = gc.reference_result(fx, cfg, "none")
        assert keep_all[2] == 0 and keep_none[2] == len(cv)


def test_encoder_round_trips():
    rng = np.random.default_rng(5)
    vals = np.sort(np.concatenate([[0, 0, 1, 0x7FFF, 0x8000, (1 << 30) - 1, 1 << 30, (1 << 60) - 1],
                                   rng.integers(0, 1 << 60, 500, dtype=np.uint64)]).astype(np.uint64))
    words = gc.encode_diffidx(vals)
    assert words.dtype == np.uint16 and (words[-1] & 0x8000)
    assert np.array_equal(gc.decode_diffidx(words), vals)
    assert np.array_equal(gc.encode_diffidx([0, 0]), np.array([0x8000, 0x8000], np.uint16))
    assert np.array_equal(gc.encode_diffidx([0x8000]), np.array([1, 0x8000], np.uint16))
    assert len(gc.encode_diffidx([])) == 0


def test_split_table_names_kmers_of_the_db():
    vals = gc.db_values(gc.load(), "fmt5_s5", "fifth")
    words = gc.encode_diffidx(vals)
    term = np.nonzero(words & 0x8000)[0]
    for n in gc.SPLITS:
        sp = gc.split_table(vals, n)
        assert sp[0].tolist() == (0, 0, 0)
        used = sp[1:][sp["ADkmer"][1:] != 0]
        assert len(used) >= 1
        for e in used:  # the entry's k-mer is the infoIdxOffset-th, and diffIdxOffset words precede the next
            k = int(e["infoIdxOffset"]) - 1
            assert vals[k] == e["ADkmer"] and term[k] + 1 == e["diffIdxOffset"]
            assert k == 0 or (vals[k - 1] >> np.uint64(24)) != (vals[k] >> np.uint64(24))
