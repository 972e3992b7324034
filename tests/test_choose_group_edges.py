"""chooseBestTaxon for short reads (k_choose_taxon_group: a 16-lane group per read, 16 reads per block)
at the edges of its groups, blocks and LDS tables.

A group's LDS tables are its own, and its phases are ordered inside its wave only, so the 16 reads of a
block run through their phases independently: a batch here mixes reads whose phases differ as much as
they can (no match, no live match, one taxon, a full taxon hash, the serial filter, a tie set that
skips the filter) in every block, at 1, 15, 16, 17 and 33 reads per batch (one group, a block less
one, a block, a block and one, two blocks and one), with matchless and all-dead reads first, last
and three in a row.

The reads come from tests/golden/ref_assign.npz (the `wide` DB: one species with 322 strains; fmt2
for the minSpScore case), cut or combined where the fixture has no read of the shape:
  * the best species' taxCnt with 1, 63, 64 and 65 distinct taxa (kGroupHash is 64: 65 takes the
    serial filter), the list in ascending taxon order whatever order the hash held it in;
  * (readLength + 3) / dnaShift of 126, 127 and 128 — 127, 128 and 129 quotients; kGroupQ is 128 and
    the last of the three takes the serial filter;
  * tie sets of 2, 16 and 20 species (the LCA path: no filter, no taxCnt), 20 spanning two 16-lane
    rounds of the species scan;
  * reads classified at the species' parent (score below minSpScore).
The reference is the oracle's assign on the same matches, compared as tests/test_k6_handoff.py does:
scores bitwise, taxID:count lists element by element. Every batch averages at most 256 matches per
read, so the group kernel is the one that runs.
"""
import numpy as np
import pytest

from metabuli_work_amd._abi import info_seq
from metabuli_work_amd.classifier import Classifier, LocalParameters
from tests import oracle_ctypes as oc
from tests.ref_assign_fixture import WIDE, build_wide_db, c_params, fl, golden, matches_of, params_of

pytestmark = pytest.mark.gpu

PM = 4
SEQ_MASK = np.uint64(0x1FFFFFFF << 32)
BATCH_SIZES = [1, 15, 16, 17, 33]


def fixture_reads(db):
    """(matches, ql1, ql2) per read of the fixture's batch for db, and the reads' tags."""
    g = golden()
    m = matches_of(g, db)
    seq = info_seq(m["qinfo"]).astype(np.int64)
    tag = g[f"{db}_tag"].tolist()
    return [(m[seq == r + 1], int(g[f"{db}_ql1"][r]), int(g[f"{db}_ql2"][r])) for r in range(len(tag))], tag


def first(tag, name):
    return tag.index(name)


class Shapes:
    """The reads of the `wide` DB this file combines."""

    def __init__(self):
        reads, tag = fixture_reads(WIDE)
        g = golden()
        self.empty = reads[first(tag, "empty")]
        self.taxa64 = reads[first(tag, "taxa64")]
        self.taxa65 = reads[first(tag, "taxa65")]
        self.taxa1 = reads[first(tag, "euk_depth9")]
        self.two_species = reads[first(tag, "euk_and_bacteria")]
        m, a, b = self.taxa64
        assert len(m) == 64 and a + b == 300
        self.taxa63 = (m[:-1], a, b)
        self.dead = (m[:PM - 1], a, b)  # one group of pm - 1 matches: K5 prunes all of it
        # (readLength + 3) / 3 of 126, 127 and 128 with the same matches (every position stays inside the read)
        self.quot = {q: (m, a, 3 * q - 3 - a) for q in (126, 127, 128)}
        tax_id, rank = g[f"{WIDE}_tax_id"].tolist(), [g["rank_names"][i] for i in g[f"{WIDE}_tax_rank"]]
        species = sorted(t for t, r in zip(tax_id, rank) if r == "species")
        sp0 = int(m["species_id"][0])
        strains = sorted(t for t, p in zip(tax_id, g[f"{WIDE}_tax_parent"].tolist()) if p == sp0 and t != sp0)
        assert len(species) == 16
        self.tie = {k: (self.tied(m[:12], (species + strains[:4])[:k]), a, b) for k in (2, 16, 20)}

    @staticmethod
    def tied(chain, taxa):
        """The same chain of matches under each of the taxa (as species and as target): equal scores."""
        out = []
        for t in taxa:
            c = chain.copy()
            c["species_id"] = t
            c["target_id"] = t
            out.append(c)
        return np.concatenate(out)


@pytest.fixture(scope="module")
def wide(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("choose_group") / "wide")
    build_wide_db(d)
    par = LocalParameters(seqMode=2)
    par.load_db_parameters(d)
    odb = oc.OracleDb(d)
    with Classifier(par, db_dir=d) as clf:
        yield Shapes(), clf, odb, par.to_c()
    odb.close()


def run_batch(clf, odb, opar, items):
    """items: (matches, ql1, ql2) per read. Returns the oracle's results after comparing the device's."""
    from tests.test_gpu_parity import compare_results
    n = len(items)
    ms = []
    for j, (m, _, _) in enumerate(items):
        m = m.copy()
        m["qinfo"] = (m["qinfo"] & ~SEQ_MASK) | (np.uint64(j + 1) << np.uint64(32))
        ms.append(m)
    matches = np.ascontiguousarray(np.concatenate(ms))
    assert len(matches) <= 256 * n, "the batch would take the wave kernel"
    oc.lib().orc_sort_matches(matches.ctypes.data, len(matches))
    ql1 = np.array([a for _, a, _ in items], np.uint32)
    ql2 = np.array([b for _, _, b in items], np.uint32)
    ores, otc = oc.assign(odb, opar, matches, ql1, ql2)
    counts = np.array([len(m) for m in ms], np.uint32)
    rng = np.random.default_rng(3)
    shuffled = np.ascontiguousarray(np.concatenate([m[rng.permutation(len(m))] for m in ms]))
    ar = clf.assign_chunks(shuffled, len(shuffled), counts, 1, (ql1 + ql2).astype(np.uint32), n)
    compare_results(ar.results, ar.taxcnt, ores, otc)
    return ores


def mixed_items(s, n):
    """n reads cycling through every shape, with matchless and all-dead reads first, last and three in
    a row in the middle (from 7 reads on)."""
    cycle = [s.taxa64, s.taxa1, s.tie[16], s.taxa65, s.quot[128], s.two_species, s.taxa63, s.tie[2], s.quot[127],
             s.tie[20], s.quot[126]]
    items = [cycle[i % len(cycle)] for i in range(n)]
    if n >= 7:
        items[0], items[-1] = s.empty, s.dead
        items[n // 2 - 1:n // 2 + 2] = [s.dead, s.empty, s.dead]
    return items


@pytest.mark.parametrize("n", BATCH_SIZES)
def test_batch_sizes(wide, n):
    s, clf, odb, opar = wide
    ores = run_batch(clf, odb, opar, mixed_items(s, n))
    assert ores["is_classified"].any()
    if n >= 7:
        assert not ores["is_classified"][[0, n - 1, n // 2 - 1, n // 2, n // 2 + 1]].any()


@pytest.mark.parametrize("lone", ["empty", "dead"])
def test_one_read_without_live_matches(wide, lone):
    s, clf, odb, opar = wide
    ores = run_batch(clf, odb, opar, [getattr(s, lone)])
    assert not ores["is_classified"][0] and ores["taxcnt_len"][0] == 0


def test_taxon_counts(wide):
    """1, 63, 64 and 65 distinct taxa in the best species' taxCnt, each beside a matchless read."""
    s, clf, odb, opar = wide
    items = [s.taxa1, s.empty, s.taxa63, s.taxa64, s.empty, s.taxa65]
    ores = run_batch(clf, odb, opar, items)
    assert ores["taxcnt_len"].tolist() == [1, 0, 63, 64, 0, 65]


def test_quotient_counts(wide):
    """(readLength + 3) / dnaShift of 126, 127 (the LDS table's last) and 128 (the serial filter)."""
    s, clf, odb, opar = wide
    items = [s.quot[q] for q in (126, 127, 128)]
    assert [(a + b + 3) // 3 for _, a, b in items] == [126, 127, 128]
    ores = run_batch(clf, odb, opar, items)
    assert ores["is_classified"].all() and (ores["taxcnt_len"] == 64).all()


def test_tie_sets(wide):
    """Tie sets of 2, 16 and 20 species: classified at their LCA, without the filter's taxCnt."""
    s, clf, odb, opar = wide
    ores = run_batch(clf, odb, opar, [s.tie[2], s.tie[16], s.tie[20], s.taxa64])
    assert ores["is_classified"].all()
    assert ores["taxcnt_len"].tolist() == [0, 0, 0, 64]
    assert len(set(ores["classification"][:3].tolist()) & set(s.tie[20][0]["species_id"].tolist())) == 0


def test_species_parent(make_db):
    """Reads whose best species scores below minSpScore are classified at the species' parent (the
    fixture's minscore_edge reads under its third parameter set), in a batch of 17 with others."""
    reads, tag = fixture_reads("fmt2")
    g = golden()
    p = params_of(g, "fmt2")[2]
    assert p["minSpScoreBits"] != 0
    pick = [first(tag, t) for t in ("minscore_edge", "minscore_edge2", "minscore_below_above", "tie_outside", "twins",
                                    "empty", "minscore_only_below")]
    idx = [pick[i % len(pick)] for i in range(17)]
    db_dir = make_db("fmt2")[0]
    par = LocalParameters(seqMode=p["seqMode"], minScore=fl(p["minScoreBits"]), minSpScore=fl(p["minSpScoreBits"]))
    odb = oc.OracleDb(db_dir)
    try:
        with Classifier(par, db_dir=db_dir) as clf:
            ores = run_batch(clf, odb, c_params(p), [reads[r] for r in idx])
    finally:
        odb.close()
    want = g["fmt2_p2_classification"]
    assert ores["classification"].tolist() == [int(want[r]) for r in idx]
    for j in (0, 1):  # at the parent: not the best species itself, and with the filter's taxCnt
        assert ores["is_classified"][j] and ores["taxcnt_len"][j] > 0
        assert ores["classification"][j] not in set(reads[idx[j]][0]["species_id"].tolist())
