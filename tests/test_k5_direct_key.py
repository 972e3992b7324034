"""K5's pruned register sort on its two keys: the direct key and the species-rank key.

A segment of 65-512 matches is pruned, then its live matches are sorted on one 64-bit key per match.
When every species of the segment is below 2^24 and every position below 2^28 the key is
species:24 | frame:3 | pos:28 | record:9 (direct); any other segment ranks its live species first and
sorts on rank:9 | frame:3 | pos:29 | record:9 (rank). The branch is taken per segment, over all of its
matches, dead ones included. Both must give the oracle's order, so every case here is compared with
the oracle's assign on the same matches (scores bitwise, taxID:count lists element by element), as
tests/test_k6_handoff.py does.

The DB's taxonomy is synthetic with three species renumbered to 2^23, 2^24 - 1 and 2^24, so real
matches of reads from those species carry those ids. A case's reads are hand-made from such matches:
  * the live part: one species' matches of a source read, inflated with ties where more are needed
    (copies of a match that differ only in hamming, dna or target), cut to the wanted count;
  * the dead part: filler matches of other species with at most pm - 1 matches per (species, frame)
    pair, which the pruning drops;
  * a position offset for the whole segment (the read grows by as much, so every position stays
    inside the read as in real input).
Which branch a read takes follows from its matches alone (`branch`), and every case states it.

Sizes: 64, 65, 128, 129, 256, 257 and 512 matches per read (the register kernels' class edges; 64
sorts first and prunes after, with neither key), each with 0 live matches, a lone group of pm - 1
(dead), pm, 64, 65 and all of them live. Species 1 (the smallest id: the root, as a pathless group),
2^23, 2^24 - 1 (direct) and 2^24 (rank). Positions 0, 2^28 - 1 (direct), 2^28 and 2^29 - 1 (rank).
All six frames. Ties of 2, 3 and 5 on (species, frame, pos). A direct read next to a rank read.

The oracle's own order on these inputs is checked against a plain sort without a GPU
(`test_oracle_order_is_the_plain_sort`), so the reference is known to hold inside these cases.
"""
import numpy as np
import pytest

from metabuli_work_amd import synth
from metabuli_work_amd._abi import MATCH_DTYPE, default_params, info_frame, info_pos, info_seq
from metabuli_work_amd.classifier import Classifier, LocalParameters
from tests import oracle_ctypes as oc

PM = 4  # prune_min_matches(4, 9, 1): the fewest matches of a live (species, frame) pair on this DB
SP_BITS, POS_BITS = 24, 28
BIG_IDS = [1 << 23, (1 << 24) - 1, 1 << 24]
SIZES = [64, 65, 128, 129, 256, 257, 512]


def renumbered_taxonomy():
    """40 species of one strain each; the first three species become 2^23, 2^24 - 1 and 2^24."""
    t = synth.make_taxonomy(40, 1, seed=11)
    species = [int(x) for x, r in zip(t.taxid, t.rank) if r == "species"]
    ren = dict(zip(species[:3], BIG_IDS))
    f = np.vectorize(lambda x: ren.get(int(x), int(x)), otypes=[np.int32])
    return synth.Taxonomy(f(t.taxid), f(t.parent), t.rank, t.name)


class World:
    """The DB, the oracle's matches of a read set split by read, and the species at hand."""

    def __init__(self, root):
        self.db_dir = str(root / "k5key")
        taxo = renumbered_taxonomy()
        gen = synth.make_genomes(taxo, genome_len=8000, seed=12)
        oc.build_db(self.db_dir, default_params(kmer_format=2, syncmer=0, smer_len=5), taxo, gen)
        self.par = LocalParameters(seqMode=2)
        self.par.load_db_parameters(self.db_dir)
        self.opar = self.par.to_c()
        self.odb = oc.OracleDb(self.db_dir)
        reads = synth.make_reads(gen, 400, paired=True, seed=5)
        okmers, self.ql1, self.ql2 = oc.extract(self.opar, reads)
        om = oc.match(self.odb, self.opar, okmers)
        seq = info_seq(om["qinfo"]).astype(np.int64)
        self.reads = [om[seq == r + 1] for r in range(reads.n)]
        self.species = sorted(int(x) for x, r in zip(taxo.taxid, taxo.rank) if r == "species")
        self.leaf = {int(p): int(x) for x, p, r in zip(taxo.taxid, taxo.parent, taxo.rank) if r == "no rank" and x != p}

    def source(self, species):
        """(read, its matches of that species) for the read that holds the most of them."""
        best = max(range(len(self.reads)), key=lambda r: int((self.reads[r]["species_id"] == species).sum()))
        m = self.reads[best]
        m = m[m["species_id"] == species]
        assert len(m) >= 40, f"no read with enough matches of species {species}"
        return best, m

    def close(self):
        self.odb.close()


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    w = World(tmp_path_factory.mktemp("k5key"))
    yield w
    w.close()


def sort_key(m):
    """compareMatches' fields, most significant last (np.lexsort order)."""
    return (m["dna_encoding"], m["hamming"], info_pos(m["qinfo"]), info_frame(m["qinfo"]),
            m["species_id"].astype(np.int64), info_seq(m["qinfo"]))


def inflate(m, want, field):
    """At least `want` matches from m (one species, sorted): match i becomes a tie of k_i copies that
    differ only in `field`, k_i cycling through 2, 3 and 5 (longer by a constant where that is not
    enough, and 1 once enough are there)."""
    out, i = [], 0
    extra = want - len(m)
    longer = max(0, -(-want // len(m)) - 3)  # ties of 2, 3 and 5 hold 10 / 3 per match: longer ones past that
    for x in m:
        k = (2, 3, 5)[i % 3] + longer if extra > 0 else 1
        i += 1
        for j in range(k):
            y = x.copy()
            if field == "hamming":
                y["hamming"] = (int(x["hamming"]) + j) % 8
            elif field == "dna":
                y["dna_encoding"] = int(x["dna_encoding"]) ^ (j << 3)
            else:
                y["pad"] = j  # the copy's number: live_part gives copies their targets and clears it
            out.append(y)
        extra -= k - 1
    return np.array(out, MATCH_DTYPE)


def live_part(w, species, count, field="hamming"):
    """`count` matches of `species`, in its frames' order, the first group of at least pm when count
    allows; ties on (species, frame, pos) of 2, 3 and 5 where the source read alone is too short."""
    r, m = w.source(species)
    m = inflate(m, count, field)
    if field == "target":  # a tie's copies point at the species and its strain in turn
        alt = [species, w.leaf.get(species, species)]
        m["target_id"] = np.where(m["pad"] > 0, np.array(alt, np.uint32)[m["pad"] % 2], m["target_id"])
        m["pad"] = 0
    m = m[np.lexsort(sort_key(m))][:count]
    return r, m


def filler(w, count, avoid, rng, species=None):
    """`count` dead matches: at most pm - 1 per (species, frame) pair, species outside `avoid`."""
    pool = species if species is not None else [s for s in w.species if s not in avoid and s < (1 << SP_BITS)]
    m = np.zeros(count, MATCH_DTYPE)
    i = 0
    for j in range(PM - 1):
        for s in pool:
            for f in range(6):
                if i == count:
                    break
                m[i]["qinfo"] = (f << 61) | int(rng.integers(0, 280))
                m[i]["species_id"] = s
                m[i]["target_id"] = w.leaf.get(s, s)
                m[i]["dna_encoding"] = int(rng.integers(0, 1 << 24))
                m[i]["hamming"] = int(rng.integers(0, 4))
                m[i]["right_end_hamming"] = int(rng.integers(0, 1 << 16))
                i += 1
    assert i == count, "not enough dead (species, frame) pairs"
    return m


def pathless_live_group(species, frame, n, rng):
    """n >= pm matches of one (species, frame) pair too far apart to link: live for K5, score 0 in K6."""
    m = np.zeros(n, MATCH_DTYPE)
    for i in range(n):
        m[i]["qinfo"] = (frame << 61) | (30 * i)
        m[i]["species_id"] = species
        m[i]["target_id"] = species
        m[i]["dna_encoding"] = int(rng.integers(0, 1 << 24))
        m[i]["hamming"] = int(rng.integers(0, 4))
    return m


def live_count(m):
    key = m["species_id"].astype(np.int64) * 8 + info_frame(m["qinfo"]).astype(np.int64)
    pairs, cnt = np.unique(key, return_counts=True)
    live_species = np.unique(pairs[cnt >= PM] // 8)
    return int(np.isin(m["species_id"].astype(np.int64), live_species).sum())


def branch(m):
    """The key K5 sorts this segment's live matches on."""
    if len(m) <= 64:
        return "sort-then-prune"
    wide = (m["species_id"] >= (1 << SP_BITS)).any() or (info_pos(m["qinfo"]) >= (1 << POS_BITS)).any()
    return "rank" if wide else "direct"


def make_read(w, species, n, live, rng, field="hamming", max_pos=None, extra=None):
    """One read of n matches, `live` of them of `species` (fewer than pm: a dead lone group), the rest
    dead filler; max_pos: the whole segment is moved so that its last position is exactly that.
    Returns (source read, matches, length added to the read)."""
    r, lv = live_part(w, species, live, field)
    parts = [lv] + ([extra] if extra is not None else [])
    used = sum(len(p) for p in parts)
    parts.append(filler(w, n - used, {species}, rng))
    m = np.concatenate(parts)
    grow = 0
    if max_pos is not None:
        grow = max_pos - int(info_pos(m["qinfo"]).max())
        m["qinfo"] += np.uint64(grow)
    assert len(m) == n
    want_live = (live if live >= PM else 0) + (len(extra) if extra is not None else 0)
    assert live_count(m) == want_live, (live_count(m), want_live)
    return r, m, grow


class Batch:
    def __init__(self, w, reads):
        """reads: (source read, matches, grow) per batch read."""
        self.n = len(reads)
        ms = []
        for j, (_, m, _) in enumerate(reads):
            m = m.copy()
            m["qinfo"] = (m["qinfo"] & ~np.uint64(0x1FFFFFFF << 32)) | (np.uint64(j + 1) << np.uint64(32))
            ms.append(m)
        self.per_read = ms
        src = np.array([r for r, _, _ in reads], np.int64)
        grow = np.array([g for _, _, g in reads], np.uint32)
        self.ql1 = np.ascontiguousarray(w.ql1[src] + grow)
        self.ql2 = np.ascontiguousarray(w.ql2[src])
        self.counts = np.array([len(m) for m in ms], np.uint32)
        rng = np.random.default_rng(1)
        self.shuffled = np.ascontiguousarray(np.concatenate([m[rng.permutation(len(m))] for m in ms]))
        self.branches = [branch(m) for m in ms]

    def oracle_sorted(self):
        m = self.shuffled.copy()
        oc.lib().orc_sort_matches(m.ctypes.data, len(m))
        return m


def batch_sizes(w, species):
    rng = np.random.default_rng(7)
    reads, expect = [], []
    for n in SIZES:
        for live in (0, PM - 1, PM, 64, 65, n):
            if live <= n:
                reads.append(make_read(w, species, n, live, rng))
                wide = species >= 1 << SP_BITS and live > 0  # the segment holds the species at all
                expect.append("sort-then-prune" if n <= 64 else "rank" if wide else "direct")
    b = Batch(w, reads)
    assert b.branches == expect
    return b


def case_sizes_direct(w):
    """Every size and live count, the live species the smallest real one: direct above 64 matches."""
    b = batch_sizes(w, min(s for s in w.species if s not in BIG_IDS))
    assert set(b.branches) == {"sort-then-prune", "direct"}
    frames = np.unique(np.concatenate([info_frame(m["qinfo"]) for m in b.per_read]))
    assert len(frames) == 6
    assert any((info_pos(m["qinfo"]) == 0).any() for m in b.per_read)
    return b


def case_sizes_rank(w):
    """Every size and live count, the live species 2^24: rank above 64 matches wherever the segment
    holds a match of it (a lone group of pm - 1 included), direct where it is filler alone."""
    b = batch_sizes(w, 1 << 24)
    assert b.branches.count("rank") == 5 * (len(SIZES) - 1) and b.branches.count("direct") == len(SIZES) - 1
    return b


def case_species(w):
    """Live species 2^23 and 2^24 - 1 (direct) and 2^24 (rank); species 1 as a pathless live group and
    as dead filler beside a real species (direct)."""
    rng = np.random.default_rng(8)
    reads = [make_read(w, s, n, n // 2, rng) for s in BIG_IDS for n in (200, 400)]
    small = min(s for s in w.species if s not in BIG_IDS)
    reads.append(make_read(w, small, 200, 80, rng, extra=pathless_live_group(1, 2, PM + 1, rng)))
    r, m, g = make_read(w, small, 200, 80, rng)
    m[-3:] = filler(w, 3, set(), rng, species=[1])[:3]
    reads.append((r, m, g))
    b = Batch(w, reads)
    assert b.branches == ["direct"] * 4 + ["rank"] * 2 + ["direct"] * 2
    return b


def case_positions(w):
    """The segment's last position at 2^28 - 1 (direct), 2^28 and 2^29 - 1 (rank), and unmoved (from 0)."""
    rng = np.random.default_rng(9)
    small = min(s for s in w.species if s not in BIG_IDS)
    reads = [make_read(w, small, 200, 90, rng, max_pos=p) for p in ((1 << 28) - 1, 1 << 28, (1 << 29) - 1, None)]
    b = Batch(w, reads)
    assert b.branches == ["direct", "rank", "rank", "direct"]
    assert int(info_pos(b.per_read[0]["qinfo"]).max()) == (1 << 28) - 1
    assert int(info_pos(b.per_read[2]["qinfo"]).max()) == (1 << 29) - 1
    return b


def case_ties(w):
    """Ties of 2, 3 and 5 on (species, frame, pos) that differ only in hamming, dna or target, on both keys."""
    rng = np.random.default_rng(10)
    small = min(s for s in w.species if s not in BIG_IDS)
    reads = [make_read(w, s, 300, 130, rng, field=f) for s in (small, 1 << 24) for f in ("hamming", "dna", "target")]
    b = Batch(w, reads)
    assert b.branches == ["direct"] * 3 + ["rank"] * 3
    for m, f in zip(b.per_read, ("hamming", "dna", "target") * 2):
        lv = m[m["species_id"] == m["species_id"][0]]
        k = lv["species_id"].astype(np.uint64) << np.uint64(35) | info_frame(lv["qinfo"]) << np.uint64(32) | info_pos(lv["qinfo"])
        _, cnt = np.unique(k, return_counts=True)
        assert {2, 3, 5} <= set(cnt.tolist()), (f, sorted(set(cnt.tolist())))
    return b


def case_mixed(w):
    """Direct and rank reads alternate in one batch, with matchless reads between them."""
    rng = np.random.default_rng(11)
    small = min(s for s in w.species if s not in BIG_IDS)
    reads = []
    for i in range(6):
        reads.append(make_read(w, (small, 1 << 24)[i % 2], 129 + 60 * i, 100, rng))
        if i % 3 == 1:
            r, m, g = reads[-1]
            reads.append((r, m[:0], 0))
    b = Batch(w, reads)
    assert [x for x in b.branches if x != "sort-then-prune"] == ["direct", "rank"] * 3
    return b


CASES = [case_sizes_direct, case_sizes_rank, case_species, case_positions, case_ties, case_mixed]
_ids = [c.__name__[5:] for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_oracle_order_is_the_plain_sort(world, case):
    """The reference's order on these inputs is the plain lexicographic one on (read, species, frame,
    pos, hamming, dna): the oracle's sort against numpy's, key by key (target is not compared by the
    reference, and a tie on everything else holds equal keys either way)."""
    b = case(world)
    got = b.oracle_sorted()
    want = b.shuffled[np.lexsort(sort_key(b.shuffled))]
    for a, e in zip(sort_key(got), sort_key(want)):
        assert np.array_equal(a, e)
    full = lambda m: np.sort(m.view(np.dtype((np.void, MATCH_DTYPE.itemsize))))
    assert np.array_equal(full(got), full(b.shuffled))


@pytest.fixture(scope="module")
def clf(world):
    c = Classifier(world.par, db_dir=world.db_dir)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_pruned_sort_matches_oracle(world, clf, case):
    from tests.test_gpu_parity import compare_results
    b = case(world)
    ores, otc = oc.assign(world.odb, world.opar, b.oracle_sorted(), b.ql1, b.ql2)
    ql = (b.ql1 + b.ql2).astype(np.uint32)
    ar = clf.assign_chunks(b.shuffled, len(b.shuffled), b.counts, 1, ql, b.n)  # the pruning K5
    compare_results(ar.results, ar.taxcnt, ores, otc)
    if case is not case_mixed:
        assert ores["is_classified"].any()  # the case reaches the scoring, not only the empty paths
