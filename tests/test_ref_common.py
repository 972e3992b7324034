"""tests/common_expect.py held byte for byte to the reference's own output (tests/golden/ref_common.npz, made
by tests/golden/make_ref_common.py from extractKmer_dna2aa and mergeTargetFiles<COMMON_KMER> as written):
the six-frame AA 12-mers of the fixture's genomes, and the diffIdx / info / split of its flush-file cases.
CPU only."""
import functools
import pathlib
import types

import numpy as np
import pytest

from tests import common_expect as ce
from tests.dbref import Tree, decode_diff

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "ref_common.npz"
CONFIGS = [("fmt3", 0, 5), ("fmt5_s5", 1, 5), ("fmt5_s6", 1, 6)]


@functools.lru_cache(maxsize=None)
def fixture():
    return np.load(GOLDEN)


@functools.lru_cache(maxsize=None)
def tree():
    fx = fixture()
    return Tree(types.SimpleNamespace(taxid=fx["tax_id"], parent=fx["tax_parent"], rank=fx["tax_rank"].tolist()))


def case_names():
    return fixture()["cases"].tolist()


def case_pairs(fx, name):
    """The case's flush files as distinct (value, species) pairs, and the k-mers before the merge (the files'
    entries, IndexCreator.h:343)."""
    vs, ss, n_before = [], [], 0
    for i in range(int(fx[f"{name}_n_in"])):
        v = decode_diff(fx[f"{name}_in{i}_diffIdx"])
        t = fx[f"{name}_in{i}_info"].astype(np.int64)
        assert len(v) == len(t)
        sp = tree().sp[t]
        assert (sp > 0).all()
        vs.append(v)
        ss.append(sp)
        n_before += len(v)
    v, s = np.concatenate(vs), np.concatenate(ss)
    o = np.lexsort((s, v))
    v, s = v[o], s[o]
    head = np.ones(len(v), bool)
    head[1:] = (v[1:] != v[:-1]) | (s[1:] != s[:-1])
    return v[head], s[head], n_before


@pytest.mark.parametrize("cfg", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_six_frame_kmers_equal_the_reference(cfg):
    name, syncmer, smer = cfg
    fx = fixture()
    ref_v, ref_g = fx[f"{name}_value"], fx[f"{name}_genome"]
    for g, seq in enumerate(fx["genomes"].tolist()):
        got = ce.genome_kmers(seq.encode(), syncmer, smer)
        assert got.tobytes() == ref_v[ref_g == g].tobytes(), f"genome {g} ({len(seq)} bases)"


def test_first_windows_appear_with_the_length():
    """35 .. 39 bases: 12 codons need 36 bases from the frame's begin; the reverse frames lose frame % 3 bases
    at the right end. 39 bases hold 13 codons in frames 0 and 3: two windows each."""
    fx = fixture()
    lens = [len(s) for s in fx["genomes"].tolist()]
    for n, want in ((35, 0), (36, 2), (37, 4), (38, 6), (39, 8)):
        g = lens.index(n)
        assert int((fx["fmt3_genome"] == g).sum()) == want


@pytest.mark.parametrize("name", case_names())
def test_common_rule_equals_the_reference(name):
    fx = fixture()
    v, s, n_before = case_pairs(fx, name)
    split_num = int(fx[f"{name}_split_num"])
    diff, info, split, values = ce.expected_from_pairs(tree(), v, s, n_before, split_num)
    assert diff.tobytes() == fx[f"{name}_diffIdx"].tobytes()
    assert info.tobytes() == fx[f"{name}_info"].tobytes()
    assert split.tobytes() == fx[f"{name}_split"].tobytes()


def test_cases_hold_what_they_were_designed_for():
    fx = fixture()
    t = tree()
    seen_root = seen_genus = seen_far = False
    n_ins, splits = set(), set()
    first_last = set()
    for name in case_names():
        if name == "from_genomes":
            continue
        v, s, _ = case_pairs(fx, name)
        values, info = ce.common_rule(t, v, s)
        n_ins.add(int(fx[f"{name}_n_in"]))
        splits.add(int(fx[f"{name}_split_num"]))
        first_last.add((bool(values[0] == v[0]), bool(values[-1] == v[-1])))
        ranks = {t.rank[int(x)] for x in info.tolist()}
        seen_root |= 1 in info.tolist()
        seen_genus |= "genus" in ranks
        seen_far |= bool(ranks - {"genus", "no rank"})
        single = np.setdiff1d(v, values)
        assert len(single) and len(values)
    assert n_ins == {2, 3, 8} and splits == {4, 16, 4096}
    assert first_last == {(True, False), (False, True), (True, True), (False, False)}
    assert seen_root and seen_genus and seen_far


def test_one_flush_quirk_is_recorded_not_expected():
    """numOfFlush == 1 (IndexCreator.cpp:296-299): the reference leaves its single flush file as the DB; the
    COMMON_KMER rule over that file keeps only the values of two species."""
    fx = fixture()
    left = decode_diff(fx["one_flush_in0_diffIdx"])
    ruled = decode_diff(fx["one_flush_diffIdx"])
    assert 0 < len(ruled) < len(np.unique(left)) and np.isin(ruled, left).all()
    assert len(left) > len(np.unique(left))  # a value under two species: two entries of the file
