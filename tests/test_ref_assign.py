"""The per-read scoring path pinned to the reference's own Taxonomer code (round 8).

tests/golden/ref_assign.npz (tests/golden/make_ref_assign.py) holds, for fmt2, fmt1, fmt2_syncmer and
fmt2_acc, match lists in compareMatches order and what the reference's own chooseBestTaxon
(getBestSpeciesMatches, getMatchPaths, combineMatchPaths, filterRedundantMatches,
lowerRankClassification / getSpeciesCladeCounts / BFS, Taxonomer.cpp:130-648) returned for them under
four parameter sets, over the taxonomy make_db builds; and for compareDna (KmerMatcher.cpp:1117-1146)
the selected candidates of 720 candidate lists. The oracle's restatements are compared with it
exactly (scores bitwise), and so is the device's K5 / K6 (both entry points, default and general
paths), directly against the fixture, not the oracle; under the em parameter sets also the mappings
(species2Score lists) of both.

`fmt2_acc_blank` is the fmt2_acc taxonomy with the strains' rank strings emptied (the leaf removal of
rank "" at accessionLevel 2); make_db builds no such taxonomy, so oracle and device run over a copy
of make_db's fmt2_acc with a rewritten nodes.dmp. `wide` is a DB of its own, built here at test time
(tests/ref_assign_fixture.py): species that sit under Eukaryota, and a species with 322 strains, for
reads whose taxCnt overflows K6's LDS hashes (65 and 257 distinct taxa).

compareDna on the device: no test here. The device's selection in K4 stays covered by
test_gpu_parity.test_stage_parity, now against a pinned oracle.

Still unpinned: MMseqs2's taxonomy services (LCA, IsAncestor, rank lookup), which the fixture's generator
replaces with plain parent walks. The matchKmers merge loop is pinned in test_ref_match.py.
"""
import ctypes
import os
import pathlib
import shutil

import numpy as np
import pytest

from metabuli_work_amd._abi import info_pos, info_seq
from tests import oracle_ctypes as oc

from tests.ref_assign_fixture import (BLANK, DBS, EXPECTED_SHAPES, GOLDEN, WIDE, _offsets, build_wide_db, c_params,
                                      coverage_table, fl, golden, matches_of, params_of, wide_taxonomy_and_genomes)


def test_golden_covers_branches():
    g = golden()
    table = coverage_table(g)
    for k in EXPECTED_SHAPES:
        print(f"{k:44s} {table.get(k, 0)}")
    missing = [k for k in EXPECTED_SHAPES if table.get(k, 0) < 1]
    assert not missing, missing
    assert sum(len(g[f"{db}_m_ham"]) for db in DBS) <= 60000
    for db in DBS + [BLANK, WIDE]:  # every pos inside filterRedundantMatches' arrays
        m = matches_of(g, db)
        ql = (g[f"{db}_ql1"].astype(np.int64) + g[f"{db}_ql2"])[info_seq(m["qinfo"]).astype(np.int64) - 1]
        ds = 3 * (8 - params_of(g, db)[0]["smerLen"]) if params_of(g, db)[0]["syncmer"] else 3
        assert np.all(info_pos(m["qinfo"]).astype(np.int64) // ds <= (ql + 3) // ds)
        assert np.all(m["target_id"] != 0) and np.all(m["species_id"] != 0)


# ---------------------------------------------------------------------------------------------------
def test_taxonomy_matches_fixture(make_db):
    g = golden()
    for db in DBS + [BLANK, WIDE]:
        taxo = wide_taxonomy_and_genomes()[0] if db == WIDE else make_db("fmt2_acc" if db == BLANK else db)[1]
        assert np.array_equal(taxo.taxid, g[f"{db}_tax_id"]), db
        assert np.array_equal(taxo.parent, g[f"{db}_tax_parent"]), db
        ranks = [g["rank_names"][i] for i in g[f"{db}_tax_rank"]]
        want = ["" if db == BLANK and r == "no rank" and t != 1 else r for t, r in zip(taxo.taxid.tolist(), taxo.rank)]
        assert ranks == want, db
        assert int(g[f"{db}_euk"]) == taxo.taxid[taxo.name.index("Eukaryota")], db


def _fixture_results(g, db, k):
    return {x: g[f"{db}_p{k}_{x}"] for x in ("is_classified", "classification", "score_bits", "hamming_dist", "tc_len", "tc")}


def compare_to_fixture(res, tc, want, ql, hamming=True):
    """The fields and strictness of test_gpu_parity.compare_results, against the fixture."""
    assert len(res) == len(ql)
    np.testing.assert_array_equal(res["is_classified"], want["is_classified"])
    np.testing.assert_array_equal(res["classification"], want["classification"])
    np.testing.assert_array_equal(res["query_length"], ql)
    bad = np.flatnonzero(res["score"].view(np.uint32) != want["score_bits"])
    assert len(bad) == 0, f"scores not bit-identical at reads {bad[:10]}"
    if hamming:
        np.testing.assert_array_equal(res["hamming_dist"], want["hamming_dist"])
    np.testing.assert_array_equal(res["taxcnt_len"], want["tc_len"])
    off = _offsets(want["tc_len"])
    for i in np.flatnonzero(want["tc_len"]):
        a = tc[res["taxcnt_offset"][i]:res["taxcnt_offset"][i] + res["taxcnt_len"][i]]
        b = want["tc"][off[i]:off[i + 1]]
        assert np.array_equal(a["tax_id"], b[:, 0]) and np.array_equal(a["count"], b[:, 1].astype(np.uint32)), \
            f"read {i}: taxcnt {a} != {b}"


def _compare_em_lists(maps, g, db, k, want):
    """The device's --em mappings against the reference's species2Score lists, with the three
    equalities test_oracle_assign_pinned holds the oracle to (classified reads only: writeMappings)."""
    ln, lst = g[f"{db}_p{k}_s2_len"], g[f"{db}_p{k}_s2"]
    keep = np.repeat(want["is_classified"].astype(bool), ln)
    assert np.array_equal(maps["query_id"], np.repeat(np.arange(len(ln)), ln)[keep])
    assert np.array_equal(maps["species_id"], lst[keep, 0])
    assert np.array_equal(maps["score"].view(np.uint32), lst[keep, 1].astype(np.uint32))
    assert ln[want["is_classified"].astype(bool)].sum() > 0 and _offsets(ln)[-1] == len(lst)


def _blank_db(src, dst):
    shutil.copytree(src, dst)
    nodes = os.path.join(dst, "taxonomy", "nodes.dmp")
    lines = open(nodes).read().split("\n")
    with open(nodes, "w") as f:
        f.write("\n".join(ln.replace("\t|\tno rank\t|\t", "\t|\t\t|\t") if not ln.startswith("1\t") else ln
                          for ln in lines))
    assert not os.path.exists(os.path.join(dst, "taxonomyDB"))


@pytest.fixture(scope="module")
def db_dir_of(make_db, tmp_path_factory):
    """The DB directory of a fixture DB: make_db's, the blank-rank copy of fmt2_acc, or `wide`."""
    made = {}

    def get(db):
        if db not in made:
            if db == BLANK:
                made[db] = str(tmp_path_factory.mktemp("ref_assign") / "blank")
                _blank_db(make_db("fmt2_acc")[0], made[db])
            elif db == WIDE:
                made[db] = str(tmp_path_factory.mktemp("ref_assign") / "wide")
                build_wide_db(made[db])
            else:
                made[db] = make_db(db)[0]
        return made[db]
    return get


@pytest.mark.parametrize("db", DBS + [BLANK, WIDE])
def test_oracle_assign_pinned(db_dir_of, db):
    g = golden()
    db_dir = db_dir_of(db)
    odb = oc.OracleDb(db_dir)
    m = matches_of(g, db)
    ql1, ql2 = np.ascontiguousarray(g[f"{db}_ql1"]), np.ascontiguousarray(g[f"{db}_ql2"])
    for k, p in enumerate(params_of(g, db)):
        res, tc = oc.assign(odb, c_params(p), m, ql1, ql2)
        compare_to_fixture(res, tc, _fixture_results(g, db, k), ql1 + ql2)
        if p["em"]:
            maps = oc.last_em_maps()
            ln, lst = g[f"{db}_p{k}_s2_len"], g[f"{db}_p{k}_s2"]
            off = _offsets(ln)
            keep = np.repeat(res["is_classified"].astype(bool), ln)  # writeMappings: classified reads only
            assert np.array_equal(maps["query_id"], np.repeat(np.arange(len(ln)), ln)[keep])
            assert np.array_equal(maps["species_id"], lst[keep, 0])
            assert np.array_equal(maps["score"].view(np.uint32), lst[keep, 1].astype(np.uint32))
            assert ln[res["is_classified"].astype(bool)].sum() > 0 and off[-1] == len(lst)
    odb.close()


def test_oracle_compare_dna_pinned():
    g = golden()
    L = oc.lib()
    off = _offsets(g["dna_n"])
    koff = _offsets(g["dna_k"])
    for i in range(len(g["dna_n"])):
        tg = np.ascontiguousarray(g["dna_targets"][off[i]:off[i + 1]])
        n = len(tg)
        sel, ssum, sham = np.zeros(n, np.uint64), np.zeros(n, np.uint8), np.zeros(n, np.uint16)
        k = ctypes.c_uint64(0)
        assert L.orc_pin_compare_dna(int(g["dna_query"][i]), tg.ctypes.data, n, int(g["dna_frame"][i]),
                                     int(g["dna_fmt"][i]), sel.ctypes.data, ssum.ctypes.data, sham.ctypes.data,
                                     ctypes.byref(k)) == 0
        want = g["dna_sel"][koff[i]:koff[i + 1]]
        assert k.value == len(want), i
        got = np.stack([sel[:k.value], ssum[:k.value], sham[:k.value]], axis=1).astype(np.uint32)
        assert np.array_equal(got, want), i


# ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("db", DBS + [BLANK, WIDE])
def test_device_assign_pinned(db_dir_of, db):
    """K5 / K6 against the fixture: assign_chunks (the pruning K5 and the live pack) and assign_matches
    on a shuffled copy (the kept stages), at default and on the general paths."""
    from metabuli_work_amd.classifier import Classifier, LocalParameters
    g = golden()
    db_dir = db_dir_of(db)
    m = np.ascontiguousarray(matches_of(g, db))
    ql = (g[f"{db}_ql1"] + g[f"{db}_ql2"]).astype(np.uint32)
    n = len(ql)
    counts = np.bincount(info_seq(m["qinfo"]).astype(np.int64) - 1, minlength=n).astype(np.uint32)
    shuffled = m[np.random.default_rng(0).permutation(len(m))]
    old = os.environ.get("MTB_FORCE_GENERIC")
    try:
        for k, p in enumerate(params_of(g, db)):
            want = _fixture_results(g, db, k)
            for generic in ("0", "1"):
                os.environ["MTB_FORCE_GENERIC"] = generic  # read when the context opens
                par = LocalParameters(seqMode=p["seqMode"], minScore=fl(p["minScoreBits"]),
                                      minSpScore=fl(p["minSpScoreBits"]), accessionLevel=int(p["accessionLevel"] == 1),
                                      em=p["em"])
                with Classifier(par, db_dir=db_dir) as clf:
                    assert clf.par.accessionLevel == p["accessionLevel"] and clf.par.kmerFormat == p["kmerFormat"]
                    ar = clf.assign_chunks(m, len(m), counts, 1, ql, n)
                    compare_to_fixture(ar.results, ar.taxcnt, want, ql, hamming=False)
                    if p["em"]:
                        _compare_em_lists(clf.em_mappings(), g, db, k, want)
                    br = clf.assign_matches(shuffled, ql)
                    compare_to_fixture(br.results, br.taxcnt, want, ql, hamming=False)
                    if p["em"]:
                        _compare_em_lists(clf.em_mappings(), g, db, k, want)
    finally:
        if old is None:
            os.environ.pop("MTB_FORCE_GENERIC", None)
        else:
            os.environ["MTB_FORCE_GENERIC"] = old
