"""chooseBestTaxon's tie set and the top-ten cut under --em, on designed matches.

Under --em the reference sorts sp2score by score, descending, before the loop that collects the tie set
and adds up its scores in float (Taxonomer.cpp:377-394); without --em the loop runs in species order.
From three unequal scores on the two sums can round differently, so the score of a read classified at
the LCA of its tie set depends on em. The three taxon-choice kernels (k_choose_taxon_group, the
default; k_choose_taxon_wave, MTB_WAVE_TAXON=1; k_choose_taxon, MTB_WAVE_TAXON=0 or
MTB_FORCE_GENERIC=1) are held here to the oracle's assign under em=0 and em=1, scores bitwise and
taxID:count lists as tests/test_gpu_parity.compare_results does, and the device's em_mappings() to the
oracle's last_em_maps() in query id, species and score bits.

The reads are built as tests/test_choose_group_edges.py builds its tie sets: the 12-match chain of
the fixture's `taxa64` read (the `wide` DB) copied under k species. A copy's score is set by the
right_end_hamming of its last match: 0, 1, 2 and 3 give 0.185, 0.18, 0.17833 and 0.17667. Those are
all the levels there are inside the tie window (0.95 of the best): the next mismatch costs 3 score
units of the 55.5 and falls outside. So every set of more than four species holds equal scores among
unequal ones; the sets of 3 come all-unequal and with a pair of equal scores. A shorter copy (8, 6 or
4 matches: 0.145, 0.13, 0.11) scores outside the tie window, and the 4-match copy below the
minScore of 0.12 every context here runs with, so its run has spKeep = 0.

  * tie sets of 3, 5, 16, 17 and 20 species with scores ascending, descending and mixed in species
    order, the triple (2, 2, 0) among them (em=0 0x3E38E38D, em=1 0x3E38E38F on the oracle). The
    oracle must report every one as a tie set (classified, at a taxon that is none of the species),
    and its em=0 and em=1 score bits must differ for at least a third of the cases: asserted on the
    CPU, so the device test cannot pass on inputs where the order does not matter;
  * batches of 1, 16 and 17 reads, the tie reads among ordinary, matchless and all-dead reads;
  * mappings: reads with 1, 9, 10, 11, 16, 17 and 20 scored species, with equal and with unequal
    scores. 17 and 20 equal scores leave libstdc++'s introsort (metabuli_work_amd/csrc/mtb_stdsort.h
    on the device) to decide which ten survive: the oracle's ten are not the first ten in species
    order (asserted on the CPU), so a stable sort would fail. Also a read whose species outside the
    tie window make up its list, one with a species below minScore in the middle of its runs, and
    unclassified reads, which get no mappings.
"""
import os

import numpy as np
import pytest

from metabuli_work_amd.classifier import Classifier, LocalParameters
from tests import oracle_ctypes as oc
from tests.ref_assign_fixture import WIDE, build_wide_db, golden
from tests.test_choose_group_edges import SEQ_MASK, Shapes

MIN_SCORE = 0.12
# reh of the copy's last match per species, in species order
TRIPLES = [(2, 2, 0), (0, 2, 2), (2, 0, 2), (3, 1, 0), (0, 1, 3), (1, 3, 0), (3, 2, 1), (1, 2, 3), (0, 3, 3), (3, 3, 1)]
MODES = {"group": {}, "wave": {"MTB_WAVE_TAXON": "1"}, "serial": {"MTB_WAVE_TAXON": "0"},
         "generic": {"MTB_FORCE_GENERIC": "1"}}
MAP_COUNTS = (1, 9, 10, 11, 16, 17, 20)


def _orders(k):
    """Scores ascending, descending and three mixed orders over k species (reh 3, 2, 1, 0: ascending)."""
    asc = sorted((3 - (i * 4) // k for i in range(k)), reverse=True)
    out = [("asc", asc), ("desc", asc[::-1])]
    rng = np.random.default_rng(100 + k)
    for j in range(3):
        out.append((f"mixed{j}", rng.permutation(asc).tolist()))
    return out


class Reads:
    """The designed reads over the `wide` DB."""

    def __init__(self):
        s = Shapes()
        g = golden()
        m, self.a, self.b = s.taxa64
        self.chain = m[:12]
        tax_id, rank = g[f"{WIDE}_tax_id"].tolist(), [g["rank_names"][i] for i in g[f"{WIDE}_tax_rank"]]
        species = sorted(t for t, r in zip(tax_id, rank) if r == "species")
        sp0 = int(m["species_id"][0])
        strains = sorted(t for t, p in zip(tax_id, g[f"{WIDE}_tax_parent"].tolist()) if p == sp0 and t != sp0)
        self.taxa = species + strains[:4]  # as Shapes.tie: 20 "species" in ascending order
        self.fill = [s.empty, s.taxa1, s.dead, s.two_species, s.taxa63]
        self.ties = {}  # name -> read
        for rehs in TRIPLES:
            self.ties["3_" + "".join(map(str, rehs))] = self.read(rehs)
        for k in (5, 16, 17, 20):
            for name, rehs in _orders(k):
                self.ties[f"{k}_{name}"] = self.read(rehs)
        self.equal = {k: self.read([0] * k) for k in MAP_COUNTS}
        self.unequal = {k: self.read([(5 * i + k) % 4 for i in range(k)]) for k in MAP_COUNTS}
        # one best species and others outside the tie window; the 4-match copy is below minScore
        self.window = self.read([0, 0, 0, 0], lens=[8, 12, 6, 8])
        self.below = self.read([0, 0, 1, 0, 0], lens=[12, 4, 12, 4, 8])
        self.unclassified = self.read([0, 0], lens=[4, 4])

    def read(self, rehs, lens=None):
        out = []
        for i, r in enumerate(rehs):
            c = self.chain[:lens[i] if lens else 12].copy()
            c["species_id"] = self.taxa[i]
            c["target_id"] = self.taxa[i]
            c["right_end_hamming"][-1] = r
            out.append(c)
        return np.concatenate(out), self.a, self.b


def _batch(items):
    ms = []
    for j, (m, _, _) in enumerate(items):
        m = m.copy()
        m["qinfo"] = (m["qinfo"] & ~SEQ_MASK) | (np.uint64(j + 1) << np.uint64(32))
        ms.append(m)
    matches = np.ascontiguousarray(np.concatenate(ms))
    oc.lib().orc_sort_matches(matches.ctypes.data, len(matches))
    ql1 = np.array([a for _, a, _ in items], np.uint32)
    ql2 = np.array([b for _, _, b in items], np.uint32)
    return ms, matches, ql1, ql2


def oracle_run(odb, opar, items):
    """The oracle's (results, taxcnt, mappings or None) for the reads."""
    _, matches, ql1, ql2 = _batch(items)
    ores, otc = oc.assign(odb, opar, matches, ql1, ql2)
    return ores, otc, (oc.last_em_maps() if opar.em else None)


def device_run(clf, odb, opar, items):
    """assign_chunks on the reads (each read's matches shuffled), compared with the oracle's assign;
    under em the mappings too. Returns the oracle's results and mappings."""
    from tests.test_gpu_parity import compare_results
    ms, _, ql1, ql2 = _batch(items)
    ores, otc, omaps = oracle_run(odb, opar, items)
    n = len(items)
    assert sum(len(m) for m in ms) <= 256 * n, "the batch would take the wave kernel by default"
    counts = np.array([len(m) for m in ms], np.uint32)
    rng = np.random.default_rng(3)
    shuffled = np.ascontiguousarray(np.concatenate([m[rng.permutation(len(m))] for m in ms]))
    ar = clf.assign_chunks(shuffled, len(shuffled), counts, 1, (ql1 + ql2).astype(np.uint32), n)
    compare_results(ar.results, ar.taxcnt, ores, otc)
    if opar.em:
        gm = clf.em_mappings()
        assert np.array_equal(gm["query_id"], omaps["query_id"])
        assert np.array_equal(gm["species_id"], omaps["species_id"])
        assert np.array_equal(gm["score"].view(np.uint32), omaps["score"].view(np.uint32))
    return ores, omaps


def _par(db_dir, em):
    par = LocalParameters(seqMode=2, em=em, minScore=MIN_SCORE)
    par.load_db_parameters(db_dir)
    return par


@pytest.fixture(scope="module")
def wide(tmp_path_factory):
    """(reads, oracle DB, DB directory, classifier(mode, em)): one context per kernel and em, opened
    with the kernel's knob set (the knobs are read when a context opens)."""
    d = str(tmp_path_factory.mktemp("em_assign") / "wide")
    build_wide_db(d)
    odb = oc.OracleDb(d)
    open_ctx = {}

    def classifier(mode, em):
        if (mode, em) not in open_ctx:
            old = {k: os.environ.get(k) for k in ("MTB_WAVE_TAXON", "MTB_FORCE_GENERIC")}
            try:
                for k in old:
                    os.environ.pop(k, None)
                os.environ.update(MODES[mode])
                open_ctx[(mode, em)] = Classifier(_par(d, em), db_dir=d)
            finally:
                for k, v in old.items():
                    os.environ.pop(k, None)
                    if v is not None:
                        os.environ[k] = v
        return open_ctx[(mode, em)]
    yield Reads(), odb, d, classifier
    for c in open_ctx.values():
        c.close()
    odb.close()


def _tie_batches(r, n):
    """Every tie read in batches of n reads. n = 1: alone (a selection); else among ordinary, matchless
    and all-dead reads, the first and last read of a batch without live matches."""
    names = list(r.ties)
    if n == 1:
        return [[("3_220", r.ties["3_220"])]] + [[(k, r.ties[k])] for k in ("3_310", "5_mixed0", "16_asc", "17_desc",
                                                                           "20_mixed1")]
    fill = [("fill", f) for f in r.fill]
    batches, per = [], n - 6
    for a in range(0, len(names), per):
        part = [(k, r.ties[k]) for k in names[a:a + per]]
        part += [(k, r.ties[k]) for k in names[:per - len(part)]]  # the last batch filled up from the front
        items = [fill[0]] + part[:per // 2] + [fill[1], fill[2], fill[0], fill[3]] + part[per // 2:] + [fill[2]]
        assert len(items) == n
        batches.append(items)
    return batches


def test_oracle_tie_sets_depend_on_em(wide):
    """CPU. Every designed tie read is a tie set for the reference's code (classified, at the LCA, no
    taxCnt), and the order of the sum shows: the em=0 and em=1 score bits differ for at least a third."""
    r, odb, d, _ = wide
    p0, p1 = _par(d, 0).to_c(), _par(d, 1).to_c()
    items = list(r.ties.values())
    o0, _, _ = oracle_run(odb, p0, items)
    o1, _, m1 = oracle_run(odb, p1, items)
    for o in (o0, o1):
        assert o["is_classified"].all() and (o["taxcnt_len"] == 0).all()
        assert not set(o["classification"].tolist()) & set(r.taxa)
    assert np.array_equal(o0["classification"], o1["classification"])
    differ = o0["score"].view(np.uint32) != o1["score"].view(np.uint32)
    print(f"em=0 and em=1 score bits differ for {int(differ.sum())} of {len(items)} tie reads")
    assert 3 * int(differ.sum()) >= len(items)
    i = list(r.ties).index("3_220")
    assert (int(o0["score"].view(np.uint32)[i]), int(o1["score"].view(np.uint32)[i])) == (0x3E38E38D, 0x3E38E38F)
    for k in ("3_310", "3_321"):  # three unequal scores
        j = list(r.ties).index(k)
        assert len(set(m1["score"][m1["query_id"] == j].tolist())) == 3
    assert np.bincount(m1["query_id"]).max() == 10


def test_oracle_mapping_reads(wide):
    """CPU. What the mapping reads are for: the list lengths, the cut at ten, an introsort order that
    is not the stable one, a species dropped by minScore inside the runs, reads without mappings."""
    r, odb, d, _ = wide
    p1 = _par(d, 1).to_c()
    items = [r.equal[k] for k in MAP_COUNTS] + [r.unequal[k] for k in MAP_COUNTS] + [r.window, r.below, r.unclassified]
    o, _, m = oracle_run(odb, p1, items)
    n = len(MAP_COUNTS)
    lens = np.bincount(m["query_id"], minlength=len(items))
    assert lens[:n].tolist() == [min(k, 10) for k in MAP_COUNTS] and lens[n:2 * n].tolist() == lens[:n].tolist()
    for j, k in enumerate(MAP_COUNTS):
        kept = m["species_id"][m["query_id"] == j].tolist()
        assert len(set(m["score"][m["query_id"] == j].tolist())) == 1
        if k in (17, 20):
            assert kept != r.taxa[:10], "the equal-score read does not tell the introsort from a stable sort"
        if k > 1:
            sc = m["score"][m["query_id"] == n + j]
            assert len(set(sc.tolist())) > 1 and np.all(sc[:-1] >= sc[1:])
    w, b, u = 2 * n, 2 * n + 1, 2 * n + 2
    assert o["is_classified"][w] and o["classification"][w] == r.taxa[1] and lens[w] == 4
    assert o["is_classified"][b] and lens[b] == 3  # five species with matches, two of them below minScore
    assert set(m["species_id"][m["query_id"] == b].tolist()) == {r.taxa[0], r.taxa[2], r.taxa[4]}
    assert not o["is_classified"][u] and lens[u] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 16, 17])
@pytest.mark.parametrize("em", [0, 1])
@pytest.mark.parametrize("mode", list(MODES))
def test_tie_sum_order(wide, mode, em, n):
    r, odb, d, classifier = wide
    clf, opar = classifier(mode, em), _par(d, em).to_c()
    for items in _tie_batches(r, n):
        ores, _ = device_run(clf, odb, opar, [it for _, it in items])
        tie = np.array([k != "fill" for k, _ in items])
        assert ores["is_classified"][tie].all() and (ores["taxcnt_len"][tie] == 0).all()
        if n > 1:
            assert not ores["is_classified"][[0, n - 1]].any()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
def test_em_mappings_cut(wide, mode):
    """1 to 20 scored species per read, equal and unequal scores: the ten kept and their order."""
    r, odb, d, classifier = wide
    clf, opar = classifier(mode, 1), _par(d, 1).to_c()
    items = []
    for k in MAP_COUNTS:
        items += [r.equal[k], r.fill[0], r.unequal[k]]
    items += [r.window, r.fill[2], r.below, r.unclassified, r.fill[1]]
    ores, omaps = device_run(clf, odb, opar, items)
    lens = np.bincount(omaps["query_id"], minlength=len(items))
    assert lens.max() == 10 and (lens[~ores["is_classified"].astype(bool)] == 0).all()
    assert (lens[ores["is_classified"].astype(bool)] > 0).all()
    device_run(clf, odb, opar, [r.equal[20]])  # a batch of one
