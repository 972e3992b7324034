"""The common-k-mer DB built on the GPU (mtb_build_common_db, dbbuild.build_common_kmer_db) against
tests/common_expect.py (held to the reference's own output by tests/test_ref_common.py) and against the
reference fixture itself (tests/golden/ref_common.npz): diffIdx, info, split and taxID_list byte for byte.

What the device emits per genome is seen through the DB: a genome given twice, under strains of two
species, has every one of its k-mers kept, so the DB's values are the distinct values of the genome."""
import functools

import numpy as np
import pytest
import torch  # before the library is loaded, as in test_gpu_build.py: the device-resident inputs are tensors

from metabuli_work_amd import synth
from metabuli_work_amd._lib import MtbError, lib
from metabuli_work_amd.dbbuild import build_common_kmer_db, common_last_ms
from tests import common_expect as ce
from tests.dbref import Tree, decode_diff
from tests.test_ref_common import CONFIGS, fixture
from tests.test_ref_common import tree as fixture_tree

pytestmark = pytest.mark.gpu

CFG_IDS = [c[0] for c in CONFIGS]
ACGT = np.frombuffer(b"ACGT", np.uint8)


def dna(rng, n):
    return ACGT[rng.integers(0, 4, n)].tobytes()


def genomes_of(seqs, taxids):
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    seq = np.frombuffer(b"".join(seqs) or b"\0", np.uint8).copy()
    e = np.zeros(0, np.int32)
    return synth.Genomes(seq, off, np.asarray(taxids, np.int32), e, e, e, e, e)


def check_db(taxo, tree, seqs, taxids, syncmer=0, smer=5, split_num=16, device=False, expected=None):
    """Build on the device and compare every array with the expectation; returns the expected values."""
    gen = genomes_of(seqs, taxids)
    dev = None
    if device:
        dev = (torch.from_numpy(gen.seq).cuda(), torch.from_numpy(gen.off.astype(np.int64)).cuda())
    db = build_common_kmer_db(gen, taxo, None, syncmer=syncmer, smer_len=smer, split_num=split_num, device_seq=dev)
    diff, info, split, ids, values = expected or ce.expected_db(tree, seqs, taxids, syncmer, smer, split_num)
    assert db.info.tobytes() == info.tobytes()
    assert db.diff_idx.tobytes() == diff.tobytes()
    assert db.split.tobytes() == split.tobytes()
    assert db.taxid_list.tobytes() == ids.astype(np.int32).tobytes()
    return values


@functools.lru_cache(maxsize=None)
def world():
    """10 species in 3 genera (species s in genus s // 4), 2 strains each."""
    taxo = synth.make_taxonomy(10, 2, seed=7, n_genera=3, with_eukaryota=False, block_species=10, block_size=4)
    tree = Tree(taxo)
    par = dict(zip(taxo.taxid.tolist(), taxo.parent.tolist()))
    species = [int(t) for t, r in zip(taxo.taxid.tolist(), taxo.rank) if r == "species"]
    strains = {s: [t for t in par if par[t] == s] for s in species}
    genus = {s: par[s] for s in species}
    assert len(species) == 10 and len(set(genus.values())) == 3 and all(len(v) == 2 for v in strains.values())
    return taxo, tree, species, strains, genus


def two_species_strains():
    _, _, species, strains, _ = world()
    return strains[species[0]][0], strains[species[5]][1]


def twice(seqs):
    """Every genome under strains of two species: all its k-mers are kept."""
    a, b = two_species_strains()
    return [s for q in seqs for s in (q, q)], [t for _ in seqs for t in (a, b)]


# ---- extraction ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CONFIGS, ids=CFG_IDS)
def test_first_windows_of_each_frame(cfg):
    """35 .. 39 bases: the first window of each frame appears (36 bases from the frame's begin) and the reverse
    frames lose frame % 3 bases at the right end; 0 .. 2 bases hold no codon in some frames."""
    _, syncmer, smer = cfg
    taxo, tree, *_ = world()
    rng = np.random.default_rng(11)
    base = dna(rng, 39)
    for n in (35, 36, 37, 38, 39):
        seqs, taxids = twice([base[:n]])
        values = check_db(taxo, tree, seqs, taxids, syncmer, smer)
        assert values.tobytes() == np.unique(ce.genome_kmers(base[:n], syncmer, smer)).tobytes()
        if not syncmer:
            assert len(ce.genome_kmers(base[:n])) == {35: 0, 36: 2, 37: 4, 38: 6, 39: 8}[n]
    seqs, taxids = twice([base[:n] for n in (0, 1, 2, 35, 36, 37, 38, 39)])
    check_db(taxo, tree, seqs, taxids, syncmer, smer)


@pytest.mark.parametrize("cfg", CONFIGS, ids=CFG_IDS)
def test_unit_boundaries(cfg):
    """Genomes of unit - 1, unit and unit + 1 windows in frame 0 (and the bases that move the other frames
    across the same boundary), and of two units and one window."""
    _, syncmer, smer = cfg
    taxo, tree, *_ = world()
    unit = int(lib().mtb_common_unit_windows())
    assert unit == 32
    rng = np.random.default_rng(12)
    seqs = []
    for w in (unit - 1, unit, unit + 1, 2 * unit, 2 * unit + 1):
        for extra in (0, 1, 2):
            seqs.append(dna(rng, 3 * (w + ce.K - 1) + extra))
            assert len(ce.frame_aa(seqs[-1], 0)) - ce.K + 1 == w
    for q in seqs:  # one by one: a unit that ran past its genome would read the next one's bases
        s2, t2 = twice([q])
        check_db(taxo, tree, s2, t2, syncmer, smer)
    s2, t2 = twice(seqs)
    check_db(taxo, tree, s2, t2, syncmer, smer)


@pytest.mark.parametrize("cfg", CONFIGS, ids=CFG_IDS)
def test_letters_that_do_not_translate(cfg):
    """N, IUPAC codes and lower-case letters, a run of stop codons, next to an empty genome."""
    _, syncmer, smer = cfg
    taxo, tree, *_ = world()
    rng = np.random.default_rng(13)
    g = (dna(rng, 70) + b"N" + dna(rng, 50) + b"RYKMSWBDHV" + dna(rng, 61) + dna(rng, 90).lower() + b"n" +
         b"TAATAGTGATAA" * 5 + dna(rng, 45) + b"NN" + dna(rng, 36) + b"N" + dna(rng, 35))
    seqs, taxids = twice([g, b"", g[::-1], b"N" * 50])
    values = check_db(taxo, tree, seqs, taxids, syncmer, smer)
    assert 0 < len(values) < 2 * len(g)


def test_a_genome_of_many_units():
    """240 kb: 7,500 units of frame 0 alone, from the host and from device-resident sequence."""
    taxo, tree, *_ = world()
    rng = np.random.default_rng(14)
    g = dna(rng, 240_011)
    seqs, taxids = twice([g])
    exp = ce.expected_db(tree, seqs, taxids, 0, 5, 16)
    assert len(exp[4]) > 400_000
    check_db(taxo, tree, seqs, taxids, 0, 5, 16, expected=exp)
    check_db(taxo, tree, seqs, taxids, 0, 5, 16, device=True, expected=exp)
    seqs5, taxids5 = twice([g[:90_007]])
    check_db(taxo, tree, seqs5, taxids5, 1, 6, 4096)


@pytest.mark.parametrize("cfg", CONFIGS, ids=CFG_IDS)
def test_fixture_genomes_emit_the_reference_scanners_kmers(cfg):
    """The reference's extractKmer_dna2aa output for the fixture's genomes (ref_common.npz; the read path's
    ref_group_kmers.npz trims every frame to getMaxCoveredLength and is not comparable at a genome's ends)."""
    name, syncmer, smer = cfg
    fx = fixture()
    taxo, tree, *_ = world()
    seqs = [s.encode() for s in fx["genomes"].tolist()]
    s2, t2 = twice(seqs)
    values = check_db(taxo, tree, s2, t2, syncmer, smer)
    assert values.tobytes() == np.unique(fx[f"{name}_value"]).tobytes()


# ---- the rule -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def designed():
    """40 genomes over 10 species in 3 genera with planted segments. Genome order matters to the batch tests: the
    genus segment's second species arrives three genomes after its first."""
    taxo, tree, species, strains, genus = world()
    rng = np.random.default_rng(15)
    seg_strain, seg_genus, seg_far, seg_all = (dna(rng, n) for n in (150, 150, 150, 120))
    sister = [s for s in species if genus[s] == genus[species[0]]][:2]
    far = [species[0], next(s for s in species if genus[s] != genus[species[0]])]
    order = [sister[0], far[1], species[2], sister[1]] + [s for s in species if s not in (sister + [far[1], species[2]])]
    order = [s for s in order for _ in range(2)] + order + order  # 40 genomes: 4 per species
    assert len(order) == 40
    seqs, taxids, seen = [], [], {}
    for i, s in enumerate(order):
        k = seen.get(s, 0)
        seen[s] = k + 1
        g = dna(rng, 15 + i % 7)  # little of its own: the kept values reach splitNum 16's offsets
        if s == species[2]:
            g += seg_strain + dna(rng, k)       # strains of one species only: absent
        if s in sister and k < 2:
            g += seg_genus + dna(rng, 1 + k)    # two species of one genus
        if s in far and k % 2 == 0:
            g += dna(rng, 2) + seg_far          # species of two genera
        g += dna(rng, k) + seg_all + dna(rng, 40)  # every species
        seqs.append(g)
        taxids.append(strains[s][k % 2])
    return seqs, taxids, (seg_strain, seg_genus, seg_far, seg_all), (sister, far)


def test_designed_set_holds_its_cases():
    taxo, tree, species, strains, genus = world()
    seqs, taxids, (seg_strain, seg_genus, seg_far, seg_all), (sister, far) = designed()
    diff, info, split, ids, values = ce.expected_db(tree, seqs, taxids, 0, 5, 16)
    lca = dict(zip(values.tolist(), info.tolist()))

    def inner(seg):  # the windows of frame 0 that lie inside the segment wherever it is planted
        return ce.frame_kmers(seg, 0)

    assert not np.isin(inner(seg_strain), values).any()
    assert {lca[v] for v in inner(seg_genus).tolist()} == {genus[sister[0]]}
    assert {lca[v] for v in inner(seg_far).tolist()} == {tree.lca(far[0], far[1])}
    assert {lca[v] for v in inner(seg_all).tolist()} == {tree.lca(tree.lca(species[0], species[4]), species[9])}


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("batch", [None, 1, 2, 7])
def test_designed_set_in_batches(batch, device, monkeypatch):
    taxo, tree, *_ = world()
    seqs, taxids, _, _ = designed()
    if batch is not None:
        monkeypatch.setenv("MTB_COMMON_BATCH_GENOMES", str(batch))
    check_db(taxo, tree, seqs, taxids, 0, 5, 16, device=device)
    ms = common_last_ms()
    assert len(ms) == 6 and ms[5] > 0 and ms[5] >= max(ms[:5])


@pytest.mark.parametrize("split_num", [4, 16, 4096])
@pytest.mark.parametrize("cfg", CONFIGS, ids=CFG_IDS)
def test_designed_set_split_tables(cfg, split_num, monkeypatch):
    _, syncmer, smer = cfg
    taxo, tree, *_ = world()
    seqs, taxids, _, _ = designed()
    monkeypatch.setenv("MTB_COMMON_BATCH_GENOMES", "7")
    check_db(taxo, tree, seqs, taxids, syncmer, smer, split_num)


@pytest.mark.parametrize("split_num", [4, 16, 4096])
@pytest.mark.parametrize("cfg", CONFIGS, ids=CFG_IDS)
def test_split_tables_reach_their_offsets(cfg, split_num):
    """Every k-mer kept (two pairs per kept value): sizeOfSplit is two thirds of the DB at splitNum 4 and a
    seventh at 16, so entries are written at each; at 4096 sizeOfSplit is 0 (fewer pairs than entries) and the
    table stays empty."""
    _, syncmer, smer = cfg
    taxo, tree, *_ = world()
    seqs, taxids = twice([dna(np.random.default_rng(20), 900)])
    exp = ce.expected_db(tree, seqs, taxids, syncmer, smer, split_num)
    entries = int((exp[2].reshape(-1, 3)[1:, 1] != 0).sum())
    assert entries >= {4: 1, 16: 5, 4096: 0}[split_num]
    check_db(taxo, tree, seqs, taxids, syncmer, smer, split_num, expected=exp)


@pytest.mark.parametrize("batch", [None, 100])
def test_runs_longer_than_a_wave_and_a_block(batch, monkeypatch):
    """One value under 65 species (more than a wave's lanes) and under 1025 (more than the reduction's block
    of 256 pairs, so its state crosses lanes, waves and blocks, at every alignment the other runs leave)."""
    taxo = synth.make_taxonomy(1025, 1, seed=9, n_genera=40)
    tree = Tree(taxo)
    strains = [t for t, r in zip(taxo.taxid.tolist(), taxo.rank) if r == "no rank" and t != 1]
    assert len(strains) == 1025
    rng = np.random.default_rng(16)
    seg_all, seg_65 = dna(rng, 48), dna(rng, 51)
    seqs = []
    for i in range(1025):
        g = seg_all
        if 300 <= i < 365:
            g = dna(rng, i % 3) + seg_65 + b"N" + g
        if i % 97 == 0:
            g = dna(rng, 60) + b"N" + g   # k-mers of one species between the long runs
        seqs.append(g)
    if batch is not None:
        monkeypatch.setenv("MTB_COMMON_BATCH_GENOMES", str(batch))
    values = check_db(taxo, tree, seqs, strains, 0, 5, 16)
    assert len(values) >= len(np.unique(ce.genome_kmers(seg_all))) + 3


def test_fixture_genomes_equal_the_reference_merge(monkeypatch):
    """The fixture's genomes through the device against the reference's own merge of their three flush files
    (from_genomes: the flushes split the genomes by species, so the k-mers before the merge are the distinct
    (value, species) pairs), built whole and in batches."""
    fx = fixture()
    taxo = synth.Taxonomy(fx["tax_id"].astype(np.int32), fx["tax_parent"].astype(np.int32), fx["tax_rank"].tolist(),
                          [f"n{t}" for t in fx["tax_id"].tolist()])
    seqs = [s.encode() for s in fx["genomes"].tolist()]
    taxids = fx["genome_taxid"].tolist()
    exp = (fx["from_genomes_diffIdx"], fx["from_genomes_info"], fx["from_genomes_split"],
           np.unique(fx["genome_taxid"]), decode_diff(fx["from_genomes_diffIdx"]))
    assert int(fx["from_genomes_split_num"]) == 16
    check_db(taxo, fixture_tree(), seqs, taxids, 0, 5, 16, expected=exp)
    monkeypatch.setenv("MTB_COMMON_BATCH_GENOMES", "4")
    check_db(taxo, fixture_tree(), seqs, taxids, 0, 5, 16, expected=exp)


def test_zero_genomes_give_an_empty_db():
    taxo, tree, *_ = world()
    values = check_db(taxo, tree, [], [], 0, 5, 16)
    assert len(values) == 0


# ---- the directory and the grouping round trip ----------------------------------------------------------------
def _pairs(genomes, n_pairs, seed):
    """Pairs of 150-nt mates from 300-nt fragments of the genomes, either strand."""
    rng = np.random.default_rng(seed)
    comp = np.zeros(256, np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    m1, m2 = [], []
    for _ in range(n_pairs):
        g = np.frombuffer(genomes[int(rng.integers(0, len(genomes)))], np.uint8)
        st = int(rng.integers(0, len(g) - 300))
        frag = g[st:st + 300]
        rc = comp[frag[::-1]]
        a, b = (rc, frag) if rng.random() < 0.5 else (frag, rc)
        m1.append(a[:150].tobytes())
        m2.append(b[:150].tobytes())
    return m1, m2


def test_round_trip_through_group_reads(tmp_path):
    """The directory build_common_kmer_db writes goes into group_reads unchanged: the same filter counts and
    groupMap as a ReadGrouper given the expected values; kmer_params in the reference's three-line form; a DB
    built without syncmers is refused by a grouper with syncmers."""
    from metabuli_work_amd.grouping import GroupParams, ReadGrouper, group_reads

    taxo, tree, species, strains, _ = world()
    rng = np.random.default_rng(17)
    shared = dna(rng, 6000)
    seqs = [dna(rng, 9000) + shared + dna(rng, 5000), dna(rng, 7000) + shared + dna(rng, 8000), dna(rng, 20000)]
    taxids = [strains[species[0]][0], strains[species[5]][0], strains[species[5]][1]]
    par = GroupParams()
    db = build_common_kmer_db(genomes_of(seqs, taxids), taxo, str(tmp_path / "db"), syncmer=par.syncmer,
                              smer_len=par.smer_len, split_num=16)
    diff, info, split, ids, values = ce.expected_db(tree, seqs, taxids, par.syncmer, par.smer_len, 16)
    assert len(values) > 100
    for name, arr in (("diffIdx", diff), ("info", info), ("split", split)):
        assert (tmp_path / "db" / name).read_bytes() == arr.tobytes()
    assert (tmp_path / "db" / "taxID_list").read_text() == "".join(f"{t}\n" for t in ids.tolist())
    assert (tmp_path / "db" / "kmer_params").read_text() == f"syncmer 1\nsmer_len {par.smer_len}\nkmer_format 5\n"
    assert "Kmer_format\t5\n" in (tmp_path / "db" / "db.parameters").read_text()
    assert (tmp_path / "db" / "taxonomy" / "nodes.dmp").exists()
    assert db.n_kmers == len(values)

    m1, m2 = _pairs(seqs, 1500, 18)
    for name, mates in (("r1.fq", m1), ("r2.fq", m2)):
        (tmp_path / name).write_bytes(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, m, b"I" * 150) for i, m in enumerate(mates)))
    gm, st = group_reads(tmp_path / "r1.fq", tmp_path / "r2.fq", tmp_path / "out", par, max_reads=600,
                         common_db=tmp_path / "db")
    with ReadGrouper(par) as rg:
        rg.set_common_kmers(values)
        for a in range(0, len(m1), 600):
            rg.add_reads(m1[a:a + 600], m2[a:a + 600])
        want_filter = rg.filter_stats()
        rg.build_edges()
        want_gm, _ = rg.finish()
    keys = ("extracted", "db_values", "hit", "removed", "kept")
    assert {k: st["filter"][k] for k in keys} == {k: want_filter[k] for k in keys}
    assert st["filter"]["params_checked"] == 1 and 0 < st["filter"]["hit"] < st["filter"]["extracted"]
    assert np.array_equal(gm, want_gm) and gm.any()

    build_common_kmer_db(genomes_of(seqs, taxids), taxo, str(tmp_path / "db3"), syncmer=0, split_num=16)
    assert (tmp_path / "db3" / "kmer_params").read_text() == "syncmer 0\nsmer_len 5\nkmer_format 3\n"
    with ReadGrouper(par) as rg:
        with pytest.raises(MtbError, match=r"\(-1\).*do not match"):
            rg.set_common_db(tmp_path / "db3")


# ---- errors ---------------------------------------------------------------------------------------------------
def test_argument_errors():
    import ctypes

    from metabuli_work_amd.dbbuild import HostDb, MtbBuildInput, MtbDbBuilt, _lib_build

    taxo, tree, species, strains, genus = world()
    rng = np.random.default_rng(19)
    gen = genomes_of([dna(rng, 90)], [strains[species[0]][0]])
    with pytest.raises(MtbError, match=r"\(-1\).*smer_len"):
        build_common_kmer_db(gen, taxo, None, syncmer=1, smer_len=4)
    with pytest.raises(MtbError, match=r"\(-1\).*smer_len"):
        build_common_kmer_db(gen, taxo, None, syncmer=1, smer_len=13)
    with pytest.raises(MtbError, match=r"\(-1\).*split_num"):
        build_common_kmer_db(gen, taxo, None, split_num=1)
    for bad in (genus[species[0]], 1, int(taxo.taxid.max()) + 5):  # a genus, the root, no such taxon
        with pytest.raises(MtbError, match=r"\(-4\).*no species"):
            build_common_kmer_db(genomes_of([dna(rng, 90)], [bad]), taxo, None)
    # n_blocks != 0 through the C-ABI
    L = _lib_build()
    hdb = HostDb(taxo)
    tax_struct = hdb.c_struct()
    inp, out = MtbBuildInput(), MtbDbBuilt()
    taxid = np.asarray(gen.taxid, np.int32)
    inp.seq, inp.off, inp.n_genomes, inp.genome_taxid = gen.seq.ctypes.data, gen.off.ctypes.data, 1, taxid.ctypes.data
    inp.n_blocks, inp.split_num, inp.flags = 1, 16, 0
    assert L.mtb_build_common_db(ctypes.byref(inp), ctypes.byref(tax_struct), 0, 5, 0, ctypes.byref(out)) == -1
    assert b"n_blocks" in lib().mtb_last_error()
    inp.n_blocks = 0
    assert L.mtb_build_common_db(ctypes.byref(inp), ctypes.byref(tax_struct), 0, 5, 0, ctypes.byref(out)) == 0
    L.mtb_free_built(ctypes.byref(out))
