"""CPU checks of the DB builder's expectations (tests/build_cases.py), independent of the device:

* the oracle's diffIdx (decoded) and info equal (value, info) lists computed in plain Python from
  pyscan.block_windows, a plain sort and the Tree LCA, so the device-against-oracle tests of
  tests/test_gpu_build.py never compare two copies of one mistake;
* the hand-made inputs really contain the shapes they are there for (in the manner of
  test_golden_covers_branches): recounted from the oracle's outputs, a fixture that stops holding its
  shape fails here."""
import numpy as np
import pytest

from tests import build_cases as bc
from tests import pyscan
from tests.dbref import decode_diff, diff_words

AA_SHIFT = np.uint64(24)


@pytest.mark.parametrize("fmt", bc.FORMATS, ids=lambda f: "f%ds%dm%d" % f)
@pytest.mark.parametrize("name", bc.PY_CHECKED)
def test_oracle_equals_plain_python(name, fmt):
    c = bc.get_case(name)
    db = bc.oracle_db(name, fmt)
    values, info = bc.expected_kmers(c, fmt)
    assert np.array_equal(decode_diff(db["diffIdx"]), values)
    assert np.array_equal(db["info"], info)
    assert np.array_equal(db["taxID_list"], np.unique(c.gen.taxid))
    assert len(db["split"]) == 3 * 4096


def _values(name, fmt, split_num=4096):
    return decode_diff(bc.oracle_db(name, fmt, split_num)["diffIdx"])


@pytest.mark.parametrize("fmt", bc.FORMATS, ids=lambda f: "f%ds%dm%d" % f)
def test_delta_widths_and_zero_deltas(fmt):
    """Every diffIdx width the format can have occurs somewhere in the cases: 1 to 5 words in format 2; 1
    to 4 in format 1, whose values stay below 21^8 * 2^24 < 2^60 (a fifth word needs a delta of 2^60). At
    least one zero delta (one value under two species)."""
    widths, zero = set(), 0
    for name in bc.ALL_CASES:
        v = _values(name, fmt)
        widths |= set(diff_words(v).tolist())
        zero += int((np.diff(v) == 0).sum()) if len(v) > 1 else 0
    assert widths == set(range(1, 6 if fmt[0] == 2 else 5)), widths
    assert zero > 0


def _groups(c, fmt):
    """(value, species) -> taxIDs of the group, from the plain-Python windows."""
    g = {}
    for gi, vals in zip(c.gen.blk_genome.tolist(), bc.block_kmers(c, fmt)):
        t = int(c.gen.taxid[gi])
        for v in vals:
            g.setdefault((v, c.tree.species_of(t)), []).append(t)
    return g


@pytest.mark.parametrize("fmt", bc.FORMATS, ids=lambda f: "f%ds%dm%d" % f)
def test_group_shapes(fmt):
    """Groups of 1, 2 and at least 4 k-mers; groups whose LCA is the species itself, above the strain and
    accession nodes that hold the genomes; a strain as the LCA of its accessions; a genome on a genus
    node kept apart from the species below it."""
    c = bc.get_case("groups")
    g = _groups(c, fmt)
    sizes = {len(t) for t in g.values()}
    assert 1 in sizes and 2 in sizes and max(sizes) >= 4, sizes
    db = bc.oracle_db("groups", fmt)
    info = set(db["info"].tolist())
    assert {20, 21} <= info      # species from two / five strains and from accessions of two strains
    assert {30, 38} <= info      # a strain from its accessions; an ancestor of the other member
    assert 10 in info and 22 in info  # the genus-node genome and the species-node genome
    unequal = [t for t in g.values() if len({c.tree.depth[x] for x in t}) > 1]
    assert unequal               # lca_node walks from unequal depths
    s = bc.get_case("groups_synth")
    gs = _groups(s, fmt)
    assert max(len(t) for t in gs.values()) >= 4
    rank = dict(zip(s.taxo.taxid.tolist(), s.taxo.rank))
    got = {rank[int(t)] for t in bc.oracle_db("groups_synth", fmt)["info"].tolist()}
    assert got == {"accession", "no rank", "species"}, got
    sn = bc.get_case("species_nodes")
    assert {rank2 for rank2 in (dict(zip(sn.taxo.taxid.tolist(), sn.taxo.rank))[int(t)]
                                for t in bc.oracle_db("species_nodes", fmt)["info"].tolist())} == {"species"}


@pytest.mark.parametrize("fmt", bc.FORMATS, ids=lambda f: "f%ds%dm%d" % f)
def test_block_and_alphabet_shapes(fmt):
    c = bc.get_case("block_edges")
    gen = c.gen
    tags = set(c.tags)
    assert {"at_start", "at_end", "inside", "whole_genome", "overlap", "duplicate", "mod3_0", "mod3_1", "mod3_2",
            "zero_window"} <= tags
    kmers = bc.block_kmers(c, fmt)
    glen = np.diff(gen.off.astype(np.int64))
    for strand in (1, -1):
        for tag in ("at_start", "at_end", "inside"):
            for ln in (21, 22, 23, 24, 25, 26, 27, 47, 48):
                hit = [b for b in range(len(c.tags)) if c.tags[b] == tag and gen.blk_strand[b] == strand and
                       gen.blk_end[b] - gen.blk_start[b] + 1 == ln and gen.blk_genome[b] == 1]
                assert hit, (tag, ln, strand)
                b = hit[0]
                if tag == "at_start":
                    assert gen.blk_start[b] == 0
                if tag == "at_end":
                    assert gen.blk_end[b] == glen[1] - 1
                if not fmt[1]:  # without the syncmer choice every window of clean ACGT is kept
                    assert len(kmers[b]) == max(0, ln // 3 - 7)
        assert any(kmers[b] for b in range(len(kmers)) if gen.blk_strand[b] == strand)  # both strands
    assert all(not k for k, t in zip(kmers, c.tags) if t == "zero_window")
    # the middle genome's neighbours in seq: a scan shifted by one base across either edge reads a base
    # that differs from the one inside, so it cannot give the same k-mers by accident
    whole, off = bytes(gen.seq), gen.off.astype(np.int64)
    for b in range(len(c.tags)):
        if gen.blk_genome[b] == 1 and c.tags[b] in ("at_start", "at_end") and kmers[b]:
            s, e = int(off[1] + gen.blk_start[b]), int(off[1] + gen.blk_end[b])
            for d in (-1, 1):
                moved = [v for v, _ in pyscan.block_windows(whole, s + d, e + d, gen.blk_strand[b] > -1, *fmt)]
                assert moved != kmers[b]
    a = bc.get_case("alphabet")
    ag = a.gen
    seqs = [bytes(ag.seq[int(ag.off[g]):int(ag.off[g + 1])]) for g in range(ag.n)]
    blank = {}
    for b, tag in enumerate(a.tags):
        cods = pyscan.block_codons(seqs[ag.blk_genome[b]], int(ag.blk_start[b]), int(ag.blk_end[b]),
                                   ag.blk_strand[b] > -1, fmt[0])
        blank.setdefault(tag, []).append(sum(1 for aa, _ in cods if aa < 0))
    assert all(n == 1 for n in blank["N"]) and len(blank["N"]) == 36
    # atcg reads an IUPAC letter as one of its bases (R as A, Y as T, ...); V alone has no base, like N
    iupac = {t: n for t, n in blank.items() if t.startswith("iupac_")}
    assert sum(len(n) for n in iupac.values()) == 36 and len(iupac) == 10
    assert all(n == 1 for n in iupac["iupac_V"]) and len(iupac["iupac_V"]) >= 3
    assert all(n == 0 for t, ns in iupac.items() if t != "iupac_V" for n in ns)
    assert all(n == 0 for n in blank["lower"]) and len(blank["lower"]) == 36  # a lower-case base is a base
    assert all(n == 20 for n in blank["all_N"])
    assert 0 not in set(ag.blk_genome.tolist())  # genome 0 owns no block
    ak = bc.block_kmers(a, fmt)
    assert all(not k for k, t in zip(ak, a.tags) if t == "all_N")
    if not fmt[1]:
        # one bad codon: a 24-base block loses its only window; a 48-base block keeps 8, 1 or 8 of its 9
        # (bad codon first, at index 7, last in scan order), on either strand
        got = sorted(len(k) for k, t, s, e in zip(ak, a.tags, ag.blk_start, ag.blk_end) if t == "N" and e - s == 47)
        assert got == [1] * 6 + [8] * 12, got
        for tag in ("N", "iupac_V"):
            assert all(not k for k, t, s, e in zip(ak, a.tags, ag.blk_start, ag.blk_end) if t == tag and e - s == 23)
            assert all(len(k) in (1, 8) for k, t, s, e in zip(ak, a.tags, ag.blk_start, ag.blk_end)
                       if t == tag and e - s == 47)
        assert all(len(k) == (e - s + 1) // 3 - 7 for k, t, s, e in zip(ak, a.tags, ag.blk_start, ag.blk_end)
                   if t == "lower" or (t.startswith("iupac_") and t != "iupac_V"))
    for name in ("all_blank", "no_blocks"):
        db = bc.oracle_db(name, fmt)
        assert len(db["diffIdx"]) == 0 and len(db["info"]) == 0 and not db["split"].any()
    ab = bc.get_case("all_blank").gen
    assert ((ab.blk_end - ab.blk_start + 1) // 3 >= 8).all()  # R > 0: every block has windows, all blank
    assert len(bc.get_case("no_blocks").gen.blk_genome) == 0
    assert len(bc.oracle_db("one_kmer", fmt)["info"]) == 1


@pytest.mark.parametrize("fmt", bc.FORMATS, ids=lambda f: "f%ds%dm%d" % f)
def test_taxid_width_shapes(fmt):
    """Each width case holds every value once per species, in species order, with the largest taxID the
    case is named for."""
    for m in bc.TAXID_WIDTHS:
        c = bc.get_case(f"taxid_width_{m}")
        assert int(c.taxo.taxid.max()) == m
        sp = sorted(set(c.gen.taxid.tolist()))
        db = bc.oracle_db(c.name, fmt)
        v = decode_diff(db["diffIdx"])
        shared = np.flatnonzero(np.bincount(np.unique(v, return_inverse=True)[1]) == len(sp))
        assert len(shared) > 50
        first = int(np.flatnonzero(v == np.unique(v)[shared[0]])[0])
        assert db["info"][first:first + len(sp)].tolist() == sp


def _boundaries(values, split_num):
    """Indices i = k * sizeOfSplit - 1 of the k-mers that close a split (IndexCreator.cpp:819-851)."""
    size = len(values) // (split_num - 1)
    return size, [k * size - 1 for k in range(1, split_num) if size]


@pytest.mark.parametrize("fmt", bc.FORMATS, ids=lambda f: "f%ds%dm%d" % f)
def test_split_shapes(fmt):
    v = _values("split_world", fmt)
    U = len(v)
    sn = bc.split_nums(U)
    # U is an exact multiple of split_num - 1 (the last boundary is the DB's end, cnt == U) with size1 and
    # two always, and with a sizeOfSplit in between where U has such a divisor
    assert U % (sn["size1"] - 1) == 0 and U % (sn["two"] - 1) == 0
    assert "exact" not in sn or (U % (sn["exact"] - 1) == 0 and U // (sn["exact"] - 1) > 2)
    assert not bc.oracle_db("split_world", fmt, sn["size0"])["split"].any()
    for label in sorted(set(sn) - {"size0"}):
        split = bc.oracle_db("split_world", fmt, sn[label])["split"].reshape(-1, 3)
        used = split[split[:, 2] > 0]
        assert len(used) <= sn[label] - 1
        assert (np.diff(used[:, 2].astype(np.int64)) > 0).all()
    # one boundary per k-mer: most boundaries fall in an AA part already closed by the one before
    size1 = bc.oracle_db("split_world", fmt, sn["size1"])["split"].reshape(-1, 3)
    assert 0 < int((size1[:, 2] > 0).sum()) < U - 1
    # the synonymous gene: several boundaries inside one AA part, and the last one inside the DB's last
    # AA part (no entry is written for it)
    sv = _values("synonymous", fmt)
    s_num = bc.synonymous_split_num(sv)
    size, bnd = _boundaries(sv, s_num)
    aa = (sv >> AA_SHIFT).tolist()
    per_run = {}
    for i in bnd:
        per_run[aa[i]] = per_run.get(aa[i], 0) + 1
    assert max(per_run.values()) >= 3
    assert any(aa[i] == aa[-1] and i < len(sv) - 1 for i in bnd)
    split = bc.oracle_db("synonymous", fmt, s_num)["split"].reshape(-1, 3)
    assert 0 < int((split[:, 2] > 0).sum()) < len(bnd) - 1

