"""Hand-made inputs of the DB builder's tests (tests/test_gpu_build.py on the GPU,
tests/test_build_expect.py on the CPU): small genomes, gene blocks and taxonomies that put the block
scanner, the (value, species) sort, the group LCA and the split table at their edges. Every case is
built by the oracle once per format (oracle_db); the expected (value, info) lists are also computed in
plain Python (expected_kmers) so that an agreement of the device with the oracle is never two copies of
one mistake."""
import dataclasses
import functools
import os
import tempfile

import numpy as np

from metabuli_work_amd import synth
from metabuli_work_amd._abi import default_params
from tests import oracle_ctypes as oc
from tests import pyscan
from tests.dbref import Tree, decode_diff

# (kmer_format, syncmer, smer_len)
FORMATS = [(2, 0, 5), (2, 1, 5), (2, 1, 6), (1, 0, 5)]
TAXID_WIDTHS = [255, 256, 65535, 65536, (1 << 24) + 1]
_TMP = tempfile.TemporaryDirectory(prefix="mtb_build_cases_")
_IUPAC = b"RYKMSWBDHV"


@dataclasses.dataclass
class Case:
    name: str
    taxo: synth.Taxonomy
    gen: synth.Genomes
    tree: Tree
    # per block: what the block is there for (the coverage test counts these)
    tags: list


def _taxonomy(rows):
    """rows: (taxID, parent, rank), root first."""
    return synth.Taxonomy(np.array([r[0] for r in rows], np.int32), np.array([r[1] for r in rows], np.int32),
                          [r[2] for r in rows], [f"{r[2]}_{r[0]}" for r in rows])


def _dna(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)]


def _case(name, taxo, seqs, taxids, blocks, tags=None):
    tree = Tree(taxo)
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    b = np.array(blocks, np.int32).reshape(-1, 4)
    for g, s, e, _ in b.tolist():  # every block lies inside its genome
        assert 0 <= s <= e < len(seqs[g]), (name, g, s, e)
    gen = synth.Genomes(np.ascontiguousarray(np.concatenate(seqs), np.uint8), off, np.array(taxids, np.int32),
                        np.array([tree.species_of(t) for t in taxids], np.int32), np.ascontiguousarray(b[:, 0]),
                        np.ascontiguousarray(b[:, 1]), np.ascontiguousarray(b[:, 2]), np.ascontiguousarray(b[:, 3]))
    return Case(name, taxo, gen, tree, list(tags) if tags is not None else [""] * len(b))


_SMALL_TREE = [(1, 1, "no rank"), (2, 1, "genus"), (3, 2, "species"), (4, 2, "species"), (5, 3, "no rank"),
               (6, 3, "no rank"), (7, 4, "no rank")]


def block_edges():
    """Blocks of 21..27, 47 and 48 bases on both strands at genome offset 0, on the genome's last base and
    in between, in three genomes (the middle one has a neighbour on either side in seq, whose random bases
    would change the k-mers if read); lengths 0, 1 and 2 modulo 3; whole-genome blocks; overlapping and
    exactly duplicated blocks; zero-window blocks scattered among them; > 256 blocks, no multiple of 256."""
    rng = np.random.default_rng(101)
    lens = [997, 1000, 1001]
    seqs = [_dna(rng, n) for n in lens]
    blocks, tags = [], []

    def add(g, s, e, strand, tag):
        blocks.append((g, s, e, strand))
        tags.append(tag)
    for g, L in enumerate(lens):
        for ln in (21, 22, 23, 24, 25, 26, 27, 47, 48):
            for strand in (1, -1):
                add(g, 0, ln - 1, strand, "at_start")
                add(g, L - ln, L - 1, strand, "at_end")
                add(g, 100 + 7 * ln, 100 + 8 * ln - 1, strand, "inside")
        for strand in (1, -1):
            add(g, 0, L - 1, strand, "whole_genome")
            add(g, 500, 640, strand, "overlap")
            add(g, 560, 700, strand, "overlap")
            add(g, 700, 820, strand, "duplicate")
            add(g, 700, 820, strand, "duplicate")
            for ln in (100, 101, 102):
                add(g, 830, 830 + ln - 1, strand, f"mod3_{ln % 3}")
    for _ in range(120):  # no window: fewer than 24 bases
        g = int(rng.integers(0, 3))
        ln = int(rng.integers(1, 24))
        s = int(rng.integers(0, lens[g] - ln + 1))
        add(g, s, s + ln - 1, 1 if rng.random() < 0.5 else -1, "zero_window")
    order = rng.permutation(len(blocks))
    blocks = [blocks[i] for i in order]
    tags = [tags[i] for i in order]
    assert len(blocks) > 256 and len(blocks) % 256 != 0
    return _case("block_edges", _taxonomy(_SMALL_TREE), seqs, [5, 6, 7], blocks, tags)


def alphabet():
    """N, IUPAC and lower-case letters at the first, a middle and the last codon of a window and at each
    of the three codon positions, both strands: in blocks of 24 bases (one window: codons 0, 4, 7) and of
    48 (nine windows: codons 0, 7, 15). A lower-case base is a base (atcg maps it like its capital) and so
    is every IUPAC letter but V (atcg maps R to A, Y to T, ...): those windows stay. An all-N block; a genome that owns no block before the one that owns them all."""
    rng = np.random.default_rng(102)
    g1 = _dna(rng, 60 * 112 + 200)
    blocks, tags = [], []
    i = 0
    for cls in ("N", "iupac", "lower"):
        for ln, codons in ((24, (0, 4, 7)), (48, (0, 7, 15))):
            for c in codons:
                for pos in range(3):
                    for strand in (1, -1):
                        s = 10 + 60 * i
                        at = s + 3 * c + pos
                        if cls == "N":
                            g1[at] = ord("N")
                        elif cls == "iupac":
                            g1[at] = _IUPAC[i % len(_IUPAC)]
                        else:
                            g1[at] = g1[at] + 32
                        blocks.append((1, s, s + ln - 1, strand))
                        tags.append(cls if cls != "iupac" else "iupac_" + chr(g1[at]))
                        i += 1
    s = 10 + 60 * i
    g1[s:s + 60] = ord("N")
    blocks += [(1, s, s + 59, 1), (1, s, s + 59, -1)]
    tags += ["all_N", "all_N"]
    s += 60
    blocks += [(1, s, s + 98, 1), (2, 0, 149, -1)]  # clean blocks
    tags += ["clean", "clean"]
    return _case("alphabet", _taxonomy(_SMALL_TREE), [_dna(rng, 300), g1, _dna(rng, 150)], [5, 6, 7], blocks, tags)


def all_blank():
    """Blocks with windows (R > 0) none of which survives: an N at least every 20 bases. The DB is empty."""
    rng = np.random.default_rng(103)
    seqs = [_dna(rng, 700), _dna(rng, 500)]
    for s in seqs:
        s[5::17] = ord("N")
    seqs[1][:] = ord("N")
    blocks = [(0, 0, 699, 1), (0, 0, 699, -1), (0, 33, 80, 1), (0, 100, 401, -1), (1, 0, 499, 1), (1, 7, 300, -1)]
    return _case("all_blank", _taxonomy(_SMALL_TREE), seqs, [5, 7], blocks)


def no_blocks():
    """n_blocks == 0: genomes and a taxonomy, no gene block at all."""
    rng = np.random.default_rng(104)
    return _case("no_blocks", _taxonomy(_SMALL_TREE), [_dna(rng, 200), _dna(rng, 100)], [5, 7], [])


def one_kmer():
    """One block of exactly one window, all valine: U == 1, and in format 2 a first delta of five words."""
    seq = np.frombuffer(b"GTGGTGGTAGTCGTGGTGGTGGTT", np.uint8).copy()
    return _case("one_kmer", _taxonomy(_SMALL_TREE), [seq], [5], [(0, 0, 23, 1)])


_GROUP_TREE = [(1, 1, "no rank"), (2, 1, "superkingdom"), (3, 2, "phylum"), (4, 3, "class"), (5, 4, "order"),
               (6, 5, "family"), (10, 6, "genus"), (11, 6, "genus"),
               (20, 10, "species"), (21, 10, "species"), (22, 10, "species"), (23, 11, "species"), (24, 11, "species"),
               (30, 20, "no rank"), (31, 20, "no rank"),
               (32, 21, "no rank"), (33, 21, "no rank"), (34, 21, "no rank"), (35, 21, "no rank"), (36, 21, "no rank"),
               (37, 23, "no rank"), (38, 24, "no rank"),
               (40, 30, "accession"), (41, 30, "accession"), (42, 31, "accession"), (43, 31, "accession"),
               (44, 38, "accession")]

# genome letter -> the taxa that hold an identical copy of it
GROUP_PLACEMENT = {
    "A": [30, 31],              # two strains of one species: the species
    "B": [37, 38],              # strains of two species of one genus: two entries, equal value, zero delta
    "C": [36, 32, 35, 33, 34],  # five strains: the species
    "D": [40, 41],              # two accessions of one strain: the strain
    "E": [43, 40],              # accessions of two strains: the species, from equal depths
    "F": [41, 31],              # an accession and a strain node: unequal depths
    "G": [44, 38],              # an accession and its own strain: the strain (an ancestor)
    "H": [22, 32],              # directly on a species node, and under another species
    "I": [10, 22, 10],          # on a genus node (its own "species", TaxonomyWrapper.cpp:479-498) and below it
    "J": [33],                  # alone
}


def groups():
    """Identical genomes under several taxa (GROUP_PLACEMENT) over a tree with accession leaves, a
    strainless species and a genome on a genus node: getTaxIdAtRank(genus, "species") is the genus
    itself (the walk starts above species level and stops at once), so that genome's k-mers form their
    own (value, species = genus) groups in the reference and here."""
    rng = np.random.default_rng(105)
    seqs, taxids, blocks = [], [], []
    for name, taxa in GROUP_PLACEMENT.items():
        s = _dna(rng, 400)
        for t in taxa:
            g = len(seqs)
            seqs.append(s.copy())
            taxids.append(t)
            blocks += [(g, 0, 399, 1), (g, 50, 349, -1), (g, 7, 200, 1)]
    return _case("groups", _taxonomy(_GROUP_TREE), seqs, taxids, blocks)


def groups_synth():
    """A make_taxonomy tree with accession leaves and one with strainless species, relabelled so that
    strains of one species and species of one genus share genomes."""
    rng = np.random.default_rng(106)
    taxo = synth.make_taxonomy(4, 2, seed=7, n_genera=2, accessions=2, block_species=4, block_size=2)
    rank = np.array(taxo.rank)
    acc = taxo.taxid[rank == "accession"].tolist()
    par = dict(zip(taxo.taxid.tolist(), taxo.parent.tolist()))
    seqs, taxids, blocks = [], [], []
    shared = [_dna(rng, 300) for _ in range(3)]
    for k, a in enumerate(acc):
        # the same genome on every accession (LCAs at strain, species level; one entry per species), one
        # per strain's accessions, and one of its own
        for s in (shared[0], shared[1 + (k // 2) % 2], _dna(rng, 300)):
            g = len(seqs)
            seqs.append(s.copy())
            taxids.append(a)
            blocks += [(g, 0, 299, 1), (g, 0, 299, -1)]
    assert len({par[a] for a in acc}) == 8
    return _case("groups_synth", taxo, seqs, taxids, blocks)


def species_nodes():
    """make_taxonomy(..., strains_per_species=0): every genome directly on a species node; sister
    species share one genome."""
    rng = np.random.default_rng(107)
    taxo = synth.make_taxonomy(4, 0, seed=8, n_genera=2, block_species=4, block_size=2)
    sp = taxo.taxid[np.array(taxo.rank) == "species"].tolist()
    shared = _dna(rng, 300)
    seqs, taxids, blocks = [], [], []
    for t in sp:
        for s in (shared, _dna(rng, 300)):
            g = len(seqs)
            seqs.append(s.copy())
            taxids.append(t)
            blocks += [(g, 0, 299, 1), (g, 3, 290, -1)]
    return _case("species_nodes", taxo, seqs, taxids, blocks)


_WIDTH_SPECIES = {
    255: [255, 127, 3],
    256: [256, 5, 255],
    65535: [65535, 0x12FF, 255, 0xFF00],
    65536: [65536, 7, 65535, 0x0100],
    (1 << 24) + 1: [(1 << 24) + 1, 9, 0x010001, 0x000101, 0x0FF0001],
}


def taxid_width(max_tax):
    """A tree whose largest taxID is max_tax, so the species digits take 1, 2, 2, 3 or 4 radix passes
    (255, 256, 65535, 65536, 2^24 + 1). One genome is copied onto every species, the largest first:
    species that differ only in the top used byte (or whose lower bytes order the other way) then hold
    every value, and a missing high pass mis-orders or splits the (value, species) groups."""
    rng = np.random.default_rng(108)
    sp = _WIDTH_SPECIES[max_tax]
    taxo = _taxonomy([(1, 1, "no rank"), (2, 1, "genus")] + [(t, 2, "species") for t in sp])
    assert int(taxo.taxid.max()) == max_tax
    shared = _dna(rng, 240)
    seqs, taxids, blocks = [], [], []
    for rep in range(2):  # twice over: a, b, .., a, b: a sort on too few digits leaves groups interleaved
        for t in sp:
            g = len(seqs)
            seqs.append(shared.copy())
            taxids.append(t)
            blocks += [(g, 0, 239, 1), (g, 0, 239, -1)]
    g = len(seqs)
    seqs.append(_dna(rng, 240))
    taxids.append(sp[0])
    blocks += [(g, 0, 239, 1)]
    return _case(f"taxid_width_{max_tax}", taxo, seqs, taxids, blocks)


def split_world():
    """The fixed small DB of the split-table tests (split_num is chosen from its unique count)."""
    taxo = synth.make_taxonomy(4, 2, seed=5)
    gen = synth.make_genomes(taxo, genome_len=2500, strain_div=0.02, seed=6, min_block=60, max_block=400)
    return Case("split_world", taxo, gen, Tree(taxo), [""] * len(gen.blk_genome))


def _codons_by_aa():
    by = {}
    for a in b"ACGT":
        for b in b"ACGT":
            for c in b"ACGT":
                key = tuple(pyscan.code(pyscan.ATCG[x]) for x in (a, b, c))
                by.setdefault(pyscan.AA[key], []).append(bytes([a, b, c]))
    return by


def synonymous():
    """Synonymous-codon variants of one gene: identical amino acids, differing DNA parts, so one AA part
    holds dozens of k-mers and spans several sizeOfSplit; some variants change one amino acid near the
    end, which gives AA parts that differ only in their low bits (three-word deltas)."""
    rng = np.random.default_rng(109)
    by = _codons_by_aa()
    aas = [a for a in by if 0 <= a < 20]
    # amino acids 10..19 in the first 18 places, 0..9 in the last 12 (and in the changed ones): the windows
    # a changed amino acid touches then sort below the others in either format, and the DB's last AA
    # part is one that every variant shares
    hi, lo = [a for a in aas if a >= 10], [a for a in aas if a < 10]
    gene = [hi[int(rng.integers(0, len(hi)))] for _ in range(18)] + [lo[int(rng.integers(0, len(lo)))] for _ in range(12)]
    seqs, blocks = [], []
    for v in range(56):
        prot = list(gene)
        if v >= 48:
            prot[int(rng.integers(25, 30))] = lo[int(rng.integers(0, len(lo)))]
        dna = b"".join(by[a][int(rng.integers(0, len(by[a])))] for a in prot)
        g = len(seqs)
        seqs.append(np.frombuffer(dna, np.uint8).copy())
        blocks.append((g, 0, len(dna) - 1, 1))
    return _case("synonymous", _taxonomy(_SMALL_TREE), seqs, [5 + (g % 2) for g in range(len(seqs))], blocks)


_BUILDERS = {"block_edges": block_edges, "alphabet": alphabet, "all_blank": all_blank, "no_blocks": no_blocks,
             "one_kmer": one_kmer, "groups": groups, "groups_synth": groups_synth, "species_nodes": species_nodes,
             "split_world": split_world, "synonymous": synonymous}
_BUILDERS.update({f"taxid_width_{m}": functools.partial(taxid_width, m) for m in TAXID_WIDTHS})

# the cases whose expected (value, info) lists are also computed in plain Python
PY_CHECKED = ["block_edges", "alphabet", "all_blank", "no_blocks", "one_kmer", "groups", "groups_synth",
              "species_nodes"] + [f"taxid_width_{m}" for m in TAXID_WIDTHS[:4]] + ["synonymous"]
# every case at the default split_num (the split-table cases add their own)
ALL_CASES = ["block_edges", "alphabet", "all_blank", "no_blocks", "one_kmer", "groups", "groups_synth",
             "species_nodes"] + [f"taxid_width_{m}" for m in TAXID_WIDTHS] + ["split_world", "synonymous"]


@functools.lru_cache(maxsize=None)
def get_case(name) -> Case:
    return _BUILDERS[name]()


def params(fmt):
    return default_params(kmer_format=fmt[0], syncmer=fmt[1], smer_len=fmt[2])


@functools.lru_cache(maxsize=None)
def oracle_db(name, fmt, split_num=4096):
    """The oracle's files for a case: {"diffIdx", "info", "split", "taxID_list"} as numpy arrays."""
    c = get_case(name)
    d = os.path.join(_TMP.name, f"{name}_f{fmt[0]}s{fmt[1]}m{fmt[2]}_{split_num}")
    oc.build_db(d, params(fmt), c.taxo, c.gen, split_num=split_num)
    out = {n: np.fromfile(os.path.join(d, n), dt) for n, dt in (("diffIdx", np.uint16), ("info", np.uint32),
                                                                ("split", np.uint64))}
    with open(os.path.join(d, "taxID_list")) as f:
        out["taxID_list"] = np.array([int(x) for x in f.read().split()], np.int32)
    for a in out.values():
        a.setflags(write=False)
    return out


def block_kmers(c: Case, fmt):
    """Per block, the scanner's windows in plain Python (pyscan.block_windows over the block's genome
    alone: nothing outside the genome can be read)."""
    gen = c.gen
    per_genome = [bytes(gen.seq[int(gen.off[g]):int(gen.off[g + 1])]) for g in range(gen.n)]
    return [[v for v, _ in pyscan.block_windows(per_genome[g], s, e, st > -1, fmt[0], fmt[1], fmt[2])]
            for g, s, e, st in zip(gen.blk_genome.tolist(), gen.blk_start.tolist(), gen.blk_end.tolist(),
                                   gen.blk_strand.tolist())]


def expected_kmers(c: Case, fmt):
    """(values, info) the DB must hold, independent of the oracle: every block's windows, a plain sort by
    (value, species, taxID), one entry per (value, species) with the LCA of the group's taxIDs by parent
    walks (filterKmers<DB_CREATION>, IndexCreator.h:475-617)."""
    rows = []
    for g, vals in zip(c.gen.blk_genome.tolist(), block_kmers(c, fmt)):
        t = int(c.gen.taxid[g])
        sp = c.tree.species_of(t)
        rows += [(v, sp, t) for v in vals]
    rows.sort()
    values, info = [], []
    i = 0
    while i < len(rows):
        j, red = i + 1, rows[i][2]
        while j < len(rows) and rows[j][:2] == rows[i][:2]:
            red = c.tree.lca(red, rows[j][2])
            j += 1
        values.append(rows[i][0])
        info.append(red)
        i = j
    return np.array(values, np.uint64), np.array(info, np.uint32)


def split_nums(n_unique):
    """{label: split_num} for a DB of n_unique k-mers: sizeOfSplit = U / (split_num - 1) of 0, 1 and 2, U
    an exact multiple of split_num - 1 with a larger sizeOfSplit, and the smallest tables."""
    U = n_unique
    assert U > 200
    d = next((k for k in range(7, 200) if U % k == 0), None)
    out = {"size0": U + 2, "size1": U + 1, "size2": U // 2 + 1, "two": 2, "three": 3}
    assert U // (out["size0"] - 1) == 0 and U // (out["size1"] - 1) == 1 and U // (out["size2"] - 1) == 2
    if d is not None:
        out["exact"] = d + 1  # sizeOfSplit = U / d exactly: the last boundary is the DB's end (cnt == U)
    return out


def synonymous_split_num(values):
    """The split_num for the synonymous DB (from the oracle's values): the smallest sizeOfSplit of 3 to 9
    k-mers, over AA parts of dozens, that puts a boundary strictly inside the DB's last AA part."""
    U = len(values)
    aa = (np.asarray(values, np.uint64) >> np.uint64(24)).tolist()
    for want in range(3, 10):
        split_num = U // want + 1
        size = U // (split_num - 1)
        if any(aa[k * size - 1] == aa[-1] and k * size - 1 < U - 1 for k in range(1, split_num)):
            return split_num
    raise AssertionError("no boundary falls inside the last AA part")
