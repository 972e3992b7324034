"""GPU merge of reference DBs (mtb_merge_db: IndexCreator::mergeTargetFiles<DB_CREATION>,
IndexCreator.h:322-472) against the oracle's builds and numpy written here: merging per-part DBs
gives the diffIdx / info of one build of all genomes (LCA is associative, the dedupe key is
(value, species)); the split table follows the merge's own rule (sizeOfSplit from the k-mer count
before merging, IndexCreator.h:343)."""
import ctypes
import functools
import os
import tempfile

import numpy as np
import pytest

from metabuli_work_amd import synth
from metabuli_work_amd._abi import default_params
from metabuli_work_amd._lib import MtbError, lib
from metabuli_work_amd.dbbuild import HostDb, build_db, merge_db_dirs, merge_dbs, merge_last_ms, subset_genomes, update_db
from tests import oracle_ctypes as oc
from tests.dbref import Tree, decode_diff
from tests.merge_expect import expected_merge, merge_rule_split

pytestmark = pytest.mark.gpu

SPLIT_NUM = 64
MTB_ERR_DB, MTB_ERR_UNSUPPORTED = -4, -6
_TMP = tempfile.TemporaryDirectory(prefix="mtb_merge_")


def read_dir(d, taxo):
    diff = np.fromfile(os.path.join(d, "diffIdx"), np.uint16)
    info = np.fromfile(os.path.join(d, "info"), np.uint32)
    split = np.fromfile(os.path.join(d, "split"), np.uint64)
    ids = np.loadtxt(os.path.join(d, "taxID_list"), dtype=np.int32, ndmin=1)
    return HostDb(taxo, diff, info, split, ids)


# ---- fixtures: the oracle builds the parts and the union once per format ------------------------
@functools.lru_cache(maxsize=None)
def world():
    taxo = synth.make_taxonomy(12, 3, seed=31, block_species=12, block_size=3)
    gen = synth.make_genomes(taxo, genome_len=15000, strain_div=0.01, species_div=0.01, seed=32)
    return taxo, gen, Tree(taxo)


@functools.lru_cache(maxsize=None)
def oracle_dbs(fmt, syncmer, groups):
    """Oracle-built DB directories: one per genome group (groups: tuple of index tuples), then the union."""
    taxo, gen, _ = world()
    par = default_params(kmer_format=fmt, syncmer=syncmer)
    root = os.path.join(_TMP.name, f"f{fmt}s{syncmer}g{len(groups)}_{abs(hash(groups))}")
    dirs = []
    for k, g in enumerate(groups):
        d = os.path.join(root, f"part{k}")
        oc.build_db(d, par, taxo, subset_genomes(gen, list(g)), split_num=SPLIT_NUM)
        dirs.append(d)
    u = os.path.join(root, "union")
    oc.build_db(u, par, taxo, gen, split_num=SPLIT_NUM)
    return par, dirs, u


def two_parts():
    _, gen, _ = world()
    n = gen.n
    return (tuple(g for g in range(n) if g % 3 != 1), tuple(g for g in range(n) if g % 3 == 1))


def three_parts():
    _, gen, _ = world()
    return tuple(tuple(g for g in range(gen.n) if g % 3 == k) for k in range(3))


# ---- 1. merge of two parts == the union build ---------------------------------------------------
@pytest.mark.parametrize("fmt,syncmer", [(2, 0), (2, 1), (1, 0)])
def test_merge_equals_union_build(fmt, syncmer):
    taxo, gen, tree = world()
    par, (dA, dB), dU = oracle_dbs(fmt, syncmer, two_parts())
    A, B, U = read_dir(dA, taxo), read_dir(dB, taxo), read_dir(dU, taxo)
    vA, vB, vU = decode_diff(A.diff_idx), decode_diff(B.diff_idx), decode_diff(U.diff_idx)
    assert len(vA) == len(A.info) and len(vB) == len(B.info) and len(vU) == len(U.info)
    # the oracle's data alone exercises every branch
    kA = np.rec.fromarrays([vA, tree.sp[A.info.astype(np.int64)]], names="v,s")
    kB = np.rec.fromarrays([vB, tree.sp[B.info.astype(np.int64)]], names="v,s")
    _, iA, iB = np.intersect1d(kA, kB, return_indices=True)
    cross = len(iA)
    absent = sum(1 for a, b in zip(A.info[iA].tolist(), B.info[iB].tolist()) if tree.lca(a, b) not in (a, b))
    two_species = int((np.unique(vU, return_counts=True)[1] >= 2).sum())
    exp_split = merge_rule_split(vU, len(vA) + len(vB), SPLIT_NUM)
    print(f"fmt {fmt} syncmer {syncmer}: A {len(vA)} B {len(vB)} union {len(vU)} cross groups {cross} "
          f"LCA absent {absent} two-species values {two_species} merge-rule split entries "
          f"{1 + int((exp_split[3::3] != 0).sum())} union split entries {1 + int((U.split[3::3] != 0).sum())}")
    assert cross > 1000
    assert absent > 1000
    assert two_species > 1000
    assert not np.array_equal(exp_split, U.split)
    # the numpy merge of the oracle's parts reproduces the oracle's union (the equivalence itself)
    ev, ei = expected_merge(tree, [(vA, A.info), (vB, B.info)])
    assert np.array_equal(ev, vU) and np.array_equal(ei, U.info)

    m = merge_dbs([A, B], taxo, par, device=0, split_num=SPLIT_NUM)
    assert m.diff_idx.tobytes() == U.diff_idx.tobytes()
    assert m.info.tobytes() == U.info.tobytes()
    assert np.array_equal(m.taxid_list, np.unique(np.concatenate([A.taxid_list, B.taxid_list])))
    assert np.array_equal(m.taxid_list, np.sort(U.taxid_list))
    assert np.array_equal(m.split, exp_split)


def test_merge_db_dirs_writes_the_union_db(tmp_path):
    """mtb_merge_db_dirs over the oracle's part directories: the files of a DB directory, with
    dirs[0]'s parameters and taxonomy."""
    taxo, _, _ = world()
    par, (dA, dB), dU = oracle_dbs(2, 1, two_parts())
    out = str(tmp_path / "merged")
    merge_db_dirs([dA, dB], out, device=0, split_num=SPLIT_NUM)
    A, B, U, M = (read_dir(d, taxo) for d in (dA, dB, dU, out))
    assert M.diff_idx.tobytes() == U.diff_idx.tobytes() and M.info.tobytes() == U.info.tobytes()
    assert np.array_equal(M.split, merge_rule_split(decode_diff(U.diff_idx), len(A.info) + len(B.info), SPLIT_NUM))
    assert np.array_equal(M.taxid_list, np.sort(U.taxid_list))  # ascending, the union
    with open(os.path.join(out, "db.parameters")) as f, open(os.path.join(dA, "db.parameters")) as g:
        assert f.read() == g.read()
    for name in ("nodes.dmp", "names.dmp", "merged.dmp"):
        with open(os.path.join(out, "taxonomy", name)) as f, open(os.path.join(dA, "taxonomy", name)) as g:
            assert f.read() == g.read()
    assert ms_sane(merge_last_ms())


def ms_sane(ms):
    """mtb_merge_last_ms: five phase times of the last merge, the total spanning the phases."""
    return len(ms) == 5 and all(x >= 0 for x in ms) and ms[4] > 0 and sum(ms[:4]) <= ms[4] * 1.001 + 1e-3


# ---- 2. three-way, any order; build_db(parts=3) -------------------------------------------------
def test_merge_three_way_any_order():
    taxo, gen, _ = world()
    par, (dA, dB, dC), dU = oracle_dbs(2, 0, three_parts())
    A, B, C, U = (read_dir(d, taxo) for d in (dA, dB, dC, dU))
    m1 = merge_dbs([A, B, C], taxo, par, device=0, split_num=SPLIT_NUM)
    m2 = merge_dbs([C, A, B], taxo, par, device=0, split_num=SPLIT_NUM)
    for name in ("diff_idx", "info", "split", "taxid_list"):
        assert getattr(m1, name).tobytes() == getattr(m2, name).tobytes(), name
    assert m1.diff_idx.tobytes() == U.diff_idx.tobytes()
    assert m1.info.tobytes() == U.info.tobytes()
    whole = build_db(gen, taxo, par, device=0, split_num=SPLIT_NUM)
    parts = build_db(gen, taxo, par, device=0, split_num=SPLIT_NUM, parts=3)
    assert parts.diff_idx.tobytes() == whole.diff_idx.tobytes()
    assert parts.info.tobytes() == whole.info.tobytes()
    assert np.array_equal(parts.taxid_list, whole.taxid_list)
    assert whole.diff_idx.tobytes() == U.diff_idx.tobytes()


# ---- 3. tile edges on hand-made DBs -------------------------------------------------------------
def pin_db(taxo, tree, values, taxids):
    """A DB from a (value, species, taxID)-sorted list, encoded by the oracle's pinned writer."""
    v = np.ascontiguousarray(values, np.uint64)
    ids = np.ascontiguousarray(taxids, np.uint32)
    n = len(v)
    if n:
        order = np.lexsort((ids, tree.sp[ids.astype(np.int64)], v))
        assert np.array_equal(order, np.arange(n)), "hand-made DB not in compareTargetKmer order"
    diff = np.zeros(5 * n + 5, np.uint16)
    nd = ctypes.c_uint64(0)
    info = np.zeros(max(n, 1), np.uint32)
    split = np.zeros(3 * SPLIT_NUM, np.uint64)
    rc = oc.lib().orc_pin_write_db(v.ctypes.data, ids.ctypes.data, n, SPLIT_NUM, diff.ctypes.data, ctypes.byref(nd),
                                   info.ctypes.data, split.ctypes.data)
    assert rc == 0
    leaves = np.unique(ids).astype(np.int32)
    return HostDb(taxo, diff[:nd.value].copy(), info[:n].copy(), split, leaves)


def tile_cases(T, leaves, tree):
    rng = np.random.default_rng(7)

    def rand_db(n, lo=0, hi=1 << 60):
        v = np.sort(rng.integers(lo, hi, size=n, dtype=np.uint64))
        t = rng.choice(leaves, size=n)
        order = np.lexsort((t, tree.sp[t], v))
        return v[order], t[order]

    cases = {}
    empty = (np.zeros(0, np.uint64), np.zeros(0, np.int64))
    cases["both empty"] = (empty, empty)
    cases["A empty, B of T + 1"] = (empty, rand_db(T + 1))
    cases["A below B"] = (rand_db(T + 3, 0, 1 << 40), rand_db(T + 5, 1 << 41, 1 << 42))
    cases["B below A"] = (rand_db(T + 3, 1 << 41, 1 << 42), rand_db(T + 5, 0, 1 << 40))
    a = rand_db(T + 7)
    cases["B a copy of A"] = (a, (a[0].copy(), a[1].copy()))
    for na, nb in ((T - 1, 1), (T, T), (T + 1, 2 * T + 1)):
        cases[f"sizes ({na}, {nb})"] = (rand_db(na), rand_db(nb))
    # a run of equal (value, species) keys from both inputs across the first tile's diagonal: T - 40
    # small keys in A, then 60 entries of one value and one species (strains 0 / 1 of it) in A and 60
    # more (strains 1 / 2) in B, then larger keys in both
    sp0 = int(tree.sp[leaves[0]])
    strains = np.array(sorted(int(x) for x in leaves if tree.sp[x] == sp0), np.int64)
    assert len(strains) == 3
    lo_v, lo_t = rand_db(T - 40, 0, 1 << 30)
    hiA, hiB = rand_db(50, 1 << 41, 1 << 42), rand_db(70, 1 << 41, 1 << 42)
    run = np.full(60, np.uint64(1 << 40))
    tA = np.sort(np.concatenate([np.full(30, strains[0]), np.full(30, strains[1])]))
    tB = np.sort(np.concatenate([np.full(30, strains[1]), np.full(30, strains[2])]))
    cases["equal run across the first diagonal"] = (
        (np.concatenate([lo_v, run, hiA[0]]), np.concatenate([lo_t, tA, hiA[1]])),
        (np.concatenate([run, hiB[0]]), np.concatenate([tB, hiB[1]])))
    return cases


def test_merge_tile_edges():
    taxo = synth.make_taxonomy(12, 3, seed=5)
    tree = Tree(taxo)
    par = default_params(kmer_format=2)
    T = int(lib().mtb_merge_tile_items())
    assert T >= 64
    leaves = np.array([t for t, r in zip(taxo.taxid.tolist(), taxo.rank) if r == "no rank" and t != 1], np.int64)
    for name, (a, b) in tile_cases(T, leaves, tree).items():
        A, B = pin_db(taxo, tree, *a), pin_db(taxo, tree, *b)
        ev, ei = expected_merge(tree, [(decode_diff(A.diff_idx), A.info), (decode_diff(B.diff_idx), B.info)])
        for order in ((A, B), (B, A)):
            m = merge_dbs(list(order), taxo, par, device=0, split_num=SPLIT_NUM)
            assert np.array_equal(decode_diff(m.diff_idx), ev), name
            assert np.array_equal(m.info, ei), name
            assert np.array_equal(m.split, merge_rule_split(ev, len(A.info) + len(B.info), SPLIT_NUM)), name
        if name == "B a copy of A":  # every group crosses; one input alone is re-encoded and re-split
            one = merge_dbs([A], taxo, par, device=0, split_num=SPLIT_NUM)
            for got in (m, one):
                assert got.diff_idx.tobytes() == A.diff_idx.tobytes() and got.info.tobytes() == A.info.tobytes()
            assert np.array_equal(one.split, merge_rule_split(ev, len(A.info), SPLIT_NUM))


# ---- 4. update_db ------------------------------------------------------------------------------
def test_update_db_classifies_like_union(tmp_path):
    from metabuli_work_amd.classifier import Classifier, LocalParameters
    from tests.test_gpu_parity import compare_results

    taxo, gen, _ = world()
    groups = two_parts()
    par, (dA, _), dU = oracle_dbs(2, 0, groups)
    out = str(tmp_path / "updated")
    update_db(dA, subset_genomes(gen, list(groups[1])), taxo, par, out, device=0, split_num=SPLIT_NUM)
    assert np.fromfile(os.path.join(out, "diffIdx"), np.uint8).tobytes() == \
        np.fromfile(os.path.join(dU, "diffIdx"), np.uint8).tobytes()
    reads = synth.make_reads(gen, 2000, paired=True, seed=9)
    lp = LocalParameters(seqMode=2).load_db_parameters(out)
    ref_lp = LocalParameters(seqMode=2).load_db_parameters(dU)
    assert lp.to_c().kmer_format == ref_lp.to_c().kmer_format == 2
    with Classifier(lp, db_dir=out, device=0) as clf:
        br = clf.classify_batch(reads.seq1, reads.off1, reads.seq2, reads.off2)
    odb = oc.OracleDb(dU)
    ores, otc = oc.classify(odb, ref_lp.to_c(), reads)
    odb.close()
    compare_results(br.results, br.taxcnt, ores, otc)
    assert int(ores["is_classified"].sum()) > 1000


# ---- 5. bad inputs ------------------------------------------------------------------------------
def _refused(dbs, taxo, par, code):
    with pytest.raises(MtbError) as e:
        merge_dbs(dbs, taxo, par, device=0, split_num=SPLIT_NUM)
    assert f"({code})" in str(e.value), str(e.value)
    assert lib().mtb_last_error().decode() != ""


def test_merge_refuses_bad_input():
    taxo, _, _ = world()
    par, (dA, dB), _ = oracle_dbs(2, 0, two_parts())
    A, B = read_dir(dA, taxo), read_dir(dB, taxo)
    short = HostDb(taxo, A.diff_idx, A.info[:-1].copy(), A.split, A.taxid_list)
    _refused([short, B], taxo, par, MTB_ERR_DB)
    # B's k-mers, but its taxa are in no list: their taxIDs have no species in the union's map
    foreign = HostDb(taxo, B.diff_idx, B.info, B.split, np.zeros(0, np.int32))
    only_a = set(A.info.tolist())
    assert any(t not in only_a for t in B.info.tolist())
    lone = HostDb(taxo, A.diff_idx[:0].copy(), A.info[:0].copy(), A.split, A.taxid_list[:1].copy())
    _refused([foreign, lone], taxo, par, MTB_ERR_DB)
    flagged = A.info.copy()
    flagged[len(flagged) // 2] |= np.uint32(1 << 31)
    _refused([HostDb(taxo, A.diff_idx, flagged, A.split, A.taxid_list), B], taxo, par, MTB_ERR_UNSUPPORTED)
