"""The k-mer join pinned to the reference's own merge loop: tests/golden/ref_match.npz holds what
KmerMatcher::matchKmers (KmerMatcher.cpp:123-481, cut out whole and compiled beside declaration-only
stand-ins by tests/golden/make_ref_match.py) returns for designed DBs and reads, the same under 1, 2, 7
and 16 threads and under split counts 4 and 4096. Until now the loop was restated twice
(oracle/orc_match.cpp and the K3 / K4 kernels) and every join test compared the two restatements.

The DBs are made of families (one AA 8-mer as N synonymous variants under different taxa), so that AA
runs of 1, 2, 3, 47, 48, 49, 63, 64, 65, 128 and 300 records exist (kLongRun is 48), one of them the
DB's first records and one its last (the last DB k-mer is never a candidate), values repeat across
species (a diff of 0), and bit 31 is set on a share of the info words (masked off with
skipRedundancy 0). The reads copy family members with 0 to 3 synonymous changes on both strands, repeat
windows within and across strands (the identical-query reuse with equal and unequal frame/3), and hold
N, IUPAC codes and lower case. test_fixture_covers_shapes counts all of that from the file.

CPU: the oracle's matchKmers, extraction and DB writer against the fixture. GPU: every join form
test_match_window_paths names that reaches different code, on a uniform batch (the short single-end
reads), a non-uniform one (with the 400-bp read) and the paired set, element for element in
compareMatches order."""
import ctypes

import numpy as np
import pytest

from metabuli_work_amd._abi import default_params, info_seq
from tests import oracle_ctypes as oc
from tests import ref_match_fixture as fx

MAIN = ["fmt2", "fmt1"]
SEQ_MODE = {"short": 1, "long": 3, "paired": 2}


@pytest.fixture(scope="module")
def g():
    return fx.golden()


@pytest.fixture(scope="module")
def db_dir(g, tmp_path_factory):
    root, made = tmp_path_factory.mktemp("ref_match"), {}

    def get(db, split_num=4096, skip=0):
        key = (db, split_num, skip)
        if key not in made:
            made[key] = fx.write_db(g, db, split_num, skip, str(root / f"{db}_{split_num}_{skip}"))
        return made[key]
    return get


# ---------------------------------------------------------------------------------------------------
# the fixture holds what it claims
def test_fixture_covers_shapes(g):
    c = fx.coverage_table(g)
    assert sorted(g["dbs"].tolist()) == sorted(MAIN + ["fmt2_syncmer"])
    for db in MAIN:
        need = [f"queries of a run of {n}" for n in fx.RUN_LENGTHS] + [
            "queries of a run above 256", "queries of the DB's first run", "queries with the last k-mer's AA",
            "queries above every DB k-mer", "queries below every DB k-mer", "queries between two present AA 8-mers",
            "identical queries, equal frame/3", "identical queries, unequal frame/3",
            "AA-equal, DNA-different neighbours", "equal consecutive DB values", "matched records with bit 31 set",
            "split 4: offsets inside an AA run", "split 4096: offsets inside an AA run", "split 4096: filtered entries",
            "matches of the long read", "matches of the paired reads", "matches with a non-zero hamming"]
        for k in need:
            assert c[f"{db}: {k}"] >= 1, (db, k)
        assert c[f"{db}: length of the DB's first run"] >= 2 and c[f"{db}: length of the DB's last run"] >= 2
        assert c[f"{db}: matches naming the DB's last k-mer"] == 0
        assert len(fx.kmer_list(g, db)[0]) <= 20000
    for k in ("queries of a run of 49", "queries of a run of 65", "identical queries, unequal frame/3",
              "matched records with bit 31 set"):
        assert c[f"fmt2_syncmer: {k}"] >= 1
    # the reads: single-end 60-150 bp, the long one (>= 400 bp) last of them, then the paired set
    for db in g["dbs"].tolist():
        s1, s2 = g[f"{db}_seq1"].tolist(), g[f"{db}_seq2"].tolist()
        ns = int(g[f"{db}_n_single"])
        assert all(60 <= len(s) <= 150 and not t for s, t in zip(s1[:ns], s2[:ns]))
        assert len(s1[ns]) >= 400 and not s2[ns] and all(s2[ns + 1:])
        text = "".join(s1 + s2)
        assert "N" in text and any(ch in text for ch in "RYKMSWBDHV") and any(ch in text for ch in "acgt")


def test_fixture_order_is_compare_matches(g):
    """The stored order is compareMatches' (sequenceID, speciesId, frame, pos, hamming, dnaEncoding), total
    on these matches: orc_sort_matches leaves it unchanged."""
    for db in g["dbs"].tolist():
        m = fx.matches_of(g, db)
        again = m.copy()
        oc.lib().orc_sort_matches(again.ctypes.data, len(again))
        assert np.array_equal(again, m)


# ---------------------------------------------------------------------------------------------------
# the oracle against the reference's own code
@pytest.mark.parametrize("threads", [1, 16])
@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("split_num", [4, 4096])
@pytest.mark.parametrize("db", MAIN + ["fmt2_syncmer"])
def test_oracle_match_pinned(g, db_dir, db, split_num, skip, threads):
    d = db_dir(db, split_num, skip)
    par = oc.load_db_parameters(d, default_params(seq_mode=1, threads=threads))
    assert par.skip_redundancy == skip
    odb = oc.OracleDb(d)
    before = oc.lib().orc_threads()
    oc.lib().orc_set_threads(threads)
    try:
        got = oc.match(odb, par, fx.query_of(g, db))
    finally:
        oc.lib().orc_set_threads(before)
        odb.close()
    want = fx.matches_of(g, db)
    assert len(got) == len(want)
    assert np.array_equal(got, want)


def _canon(k):
    return np.sort(k, order=["value", "info"])


@pytest.mark.parametrize("db", MAIN + ["fmt2_syncmer"])
def test_oracle_extract_pinned(g, db_dir, db):
    """oc.extract on the reads gives the fixture's query buffer (the reference's scanners and
    fillQueryKmerBuffer; its reserved-but-unfilled slots are not in the fixture). The order among equal
    (value, sequenceID) keys is the sort's own choice, so both sides are ordered on (value, info)."""
    d = db_dir(db)
    q = fx.query_of(g, db)
    qs = info_seq(q["info"]).astype(np.int64)
    for kind in ("long", "paired"):
        reads, first = fx.reads_of(g, db, kind)
        par = oc.load_db_parameters(d, default_params(seq_mode=SEQ_MODE[kind]))
        got, _, _ = oc.extract(par, reads)
        got = got[info_seq(got["info"]) != 0]
        want = q[(qs >= first) & (qs < first + reads.n)].copy()
        want["info"] -= np.uint64(first - 1) << np.uint64(32)
        assert len(got) == len(want)
        assert np.array_equal(_canon(got), _canon(want))
    assert int(g[f"{db}_query_kmer_number"]) == len(q)


@pytest.mark.parametrize("split_num", [4, 4096])
@pytest.mark.parametrize("db", MAIN + ["fmt2_syncmer"])
def test_oracle_writer_reproduces_files(g, db, split_num):
    """orc_pin_write_db on the decoded k-mer list (with the info words as stored, bit 31 included) writes
    the three files the reference's writer wrote."""
    v = fx.decode(g[f"{db}_diffIdx"])
    ids = np.ascontiguousarray(g[f"{db}_info"])
    n = len(v)
    diff = np.zeros(5 * n + 5, np.uint16)
    nd = ctypes.c_uint64(0)
    info = np.zeros(n, np.uint32)
    split = np.zeros(3 * split_num, np.uint64)
    rc = oc.lib().orc_pin_write_db(v.ctypes.data, ids.ctypes.data, n, split_num, diff.ctypes.data, ctypes.byref(nd),
                                   info.ctypes.data, split.ctypes.data)
    assert rc == 0
    assert np.array_equal(diff[:nd.value], g[f"{db}_diffIdx"])
    assert np.array_equal(info, g[f"{db}_info"])
    assert np.array_equal(split, g[f"{db}_s{split_num}_split"])


# ---------------------------------------------------------------------------------------------------
# the GPU join against the reference's own code
FORMS = ["default", "nofast", "gallop", "staged", "spill", "retry", "ext", "6144", "nofilter", "sweep"]
# the forms that keep a long run on its query's lane (wave_long_run takes the direct join's only: "staged"
# writes staged output, "retry" reruns the batch staged); every other form sends each query whose run holds
# more than kLongRun = 48 candidates to k_match_long
LANE_ONLY_FORMS = ("staged", "retry")


def _set_form(monkeypatch, form):
    """test_match_window_paths' settings for the form (tests/test_gpu_parity.py), and MTB_JOIN for the sweep."""
    window = "6144" if form == "6144" else "0"
    monkeypatch.setenv("MTB_SORT_LO_FINE", "36")
    monkeypatch.setenv("MTB_MATCH_WINDOW", window)
    monkeypatch.setenv("MTB_RUN_INDEX", "0" if form == "gallop" else "1")
    monkeypatch.setenv("MTB_DIRECT", {"staged": "0", "retry": "2", "spill": "3"}.get(form, "1"))
    monkeypatch.setenv("MTB_FUSE_FILTER", "1")
    monkeypatch.setenv("MTB_FILTER", "0" if form == "nofilter" else "1")
    monkeypatch.setenv("MTB_JOIN_FAST", "0" if form == "nofast" else "1")
    monkeypatch.setenv("MTB_LINE_EXT", "1" if form == "ext" else "0")
    if form == "sweep":
        monkeypatch.setenv("MTB_JOIN", "sweep")
    else:
        monkeypatch.delenv("MTB_JOIN", raising=False)


def _check_batches(g, db, d, kinds, lane_only=False):
    from metabuli_work_amd.classifier import Classifier, LocalParameters
    for kind in kinds:
        reads, first = fx.reads_of(g, db, kind)
        want, n_query = fx.subset(g, db, first, reads.n)
        par = LocalParameters(seqMode=SEQ_MODE[kind])
        with Classifier(par, db_dir=d) as clf:
            br = clf.classify_batch(reads.seq1, reads.off1, reads.seq2, reads.off2, keep_stages=True)
            gm = clf.matches()
            st = clf.stats()
        print(f"{db} {kind}: {len(gm)} matches, {br.query_kmers} query k-mers, long_run_queries "
              f"{st['long_run_queries']}, uniform_units {st['uniform_units']}, join_path {st['join_path']}")
        assert br.query_kmers == n_query
        assert len(gm) == len(want) == br.matches
        assert np.array_equal(gm, want)
        n_long = fx.long_run_queries(g, db, first, reads.n)
        assert n_long >= 1
        assert st["long_run_queries"] == (0 if lane_only else n_long)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("db", MAIN)
def test_gpu_join_pinned(g, db_dir, db, form, monkeypatch):
    """Every join form on the uniform and the non-uniform batch, info words with bit 31 (skipRedundancy 0)."""
    _set_form(monkeypatch, form)
    _check_batches(g, db, db_dir(db, 4096, 0), ("short", "long"), form in LANE_ONLY_FORMS)


@pytest.mark.gpu
@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("split_num", [4, 4096])
@pytest.mark.parametrize("db", MAIN + ["fmt2_syncmer"])
def test_gpu_join_pinned_db_variants(g, db_dir, db, split_num, skip, monkeypatch):
    """The default form on every DB variant (split count, skipRedundancy), the paired set included."""
    _set_form(monkeypatch, "default")
    _check_batches(g, db, db_dir(db, split_num, skip), ("short", "long", "paired"))
