"""Read grouping on the device (include/mtb_gpu.h's mtb_group_* section, metabuli_work_amd/grouping.py)
against the reference's own phases (tests/golden/ref_groups.npz) — every comparison exact."""
import ctypes
import functools
import json
import pathlib
import subprocess

import numpy as np
import pytest

from tests import group_cases, group_expect

ROOT = pathlib.Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"
CASE_NAMES = [c[0] for c in group_cases.cases()]

GROUP_SYMBOLS = ["mtb_group_default_params", "mtb_group_make_groups", "mtb_group_open", "mtb_group_close",
                 "mtb_group_add_batch", "mtb_group_get_kmers", "mtb_group_build_edges", "mtb_group_get_edges",
                 "mtb_group_get_skipped", "mtb_group_finish"]


@functools.lru_cache(maxsize=None)
def ref_groups():
    return np.load(GOLDEN / "ref_groups.npz")


@functools.lru_cache(maxsize=None)
def cases():
    return {c[0]: c for c in group_cases.cases()}


def _params(core, weak, n):
    from metabuli_work_amd.grouping import GroupParams

    ratio, band, total = group_cases.params_for(core, weak, n)
    return GroupParams(min_overlap_ratio=ratio, weak_band_ratio=band), total


def _relations(edges):
    from metabuli_work_amd.grouping import relations

    return relations(edges[:, 0], edges[:, 1], edges[:, 2])


# ---- phases ---------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_make_groups_equals_reference_after_each_phase(name):
    from metabuli_work_amd.grouping import make_groups

    _, n, edges, core, weak = cases()[name]
    par, total = _params(core, weak, n)
    maps, st = make_groups(_relations(edges), n, total, par)
    assert (st["core_thr"], st["weak_thr"]) == (core, weak)
    want = ref_groups()[f"{name}_maps"]
    for p in range(3):
        assert np.array_equal(maps[p], want[p]), f"{name}: groupMap after phase {('1', '1.5', '2')[p]}"
        assert st["groups_after"][p] == int((want[p][1:] == np.arange(1, n + 1)).sum())
        assert st["grouped_after"][p] == int((want[p] != 0).sum())
    assert st["reads"] == n and st["edges"] == len(edges) and st["kmers"] == total


@pytest.mark.gpu
def test_make_groups_ignores_ids_outside_the_reads():
    """An edge naming read 0 or a read past n_reads is skipped (GroupGenerator.cpp:1484-1485)."""
    from metabuli_work_amd.grouping import make_groups

    par, total = _params(15, 5, 48)
    edges = np.array([(1, 2, 20), (0, 3, 20), (3, 49, 20), (4, 5, 9), (4, 4000000000, 9)], np.int64)
    maps, _ = make_groups(_relations(edges), 48, total, par)
    assert list(maps[2][1:6]) == [1, 1, 0, 4, 4]


# ---- ABI ------------------------------------------------------------------------------------------

LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "mtb_gpu.h"
#define F(s, f) printf("%s\"" #f "\": %zu", first++ ? ", " : "", offsetof(s, f))
#define S(s) first = 0; printf("%s\"" #s "\": {\"size\": %zu, \"fields\": {", sep, sizeof(s)); sep = ", "
#define E() printf("}}")
int main(void) {
  int first = 0; const char *sep = "";
  printf("{");
  S(mtb_group_params); F(mtb_group_params, seq_mode); F(mtb_group_params, syncmer); F(mtb_group_params, smer_len);
  F(mtb_group_params, max_kmer_reads); F(mtb_group_params, max_kmer_quantile); F(mtb_group_params, min_overlap_ratio);
  F(mtb_group_params, weak_band_ratio); F(mtb_group_params, merge_support_ratio);
  F(mtb_group_params, merge_max_unit_reads); F(mtb_group_params, reserved); E();
  S(mtb_relation); F(mtb_relation, id1); F(mtb_relation, id2); F(mtb_relation, weight); F(mtb_relation, pad); E();
  S(mtb_group_stats); F(mtb_group_stats, reads); F(mtb_group_stats, kmers); F(mtb_group_stats, distinct_kmers);
  F(mtb_group_stats, skipped_kmers); F(mtb_group_stats, kept_pair_occurrences); F(mtb_group_stats, edges);
  F(mtb_group_stats, rounds); F(mtb_group_stats, cap); F(mtb_group_stats, hist_kmers); F(mtb_group_stats, hist_pairs);
  F(mtb_group_stats, groups_after); F(mtb_group_stats, grouped_after); F(mtb_group_stats, core_thr);
  F(mtb_group_stats, weak_thr); F(mtb_group_stats, ms); E();
  printf("}\n");
  return 0;
}
"""


@pytest.mark.gpu
def test_group_symbols_exported_and_layouts_match_compiled_c(tmp_path):
    """Every mtb_group_* symbol is exported, and sizeof / offsetof of the three structs as a C compiler
    lays out include/mtb_gpu.h equal the _abi.py mirrors (a small C program compiled here)."""
    from metabuli_work_amd import _abi
    from metabuli_work_amd._lib import EXPORTED, lib

    L = lib()
    for s in GROUP_SYMBOLS:
        assert s in EXPORTED and hasattr(L, s), s
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_C)
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    lay = json.loads(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout)
    for name, cls in (("mtb_group_params", _abi.MtbGroupParams), ("mtb_group_stats", _abi.MtbGroupStats)):
        assert lay[name]["size"] == ctypes.sizeof(cls), name
        assert list(lay[name]["fields"]) == [f for f, _ in cls._fields_], name
        for f, off in lay[name]["fields"].items():
            assert getattr(cls, f).offset == off, f"{name}.{f}"
    dt = _abi.RELATION_DTYPE
    assert lay["mtb_relation"]["size"] == dt.itemsize == 12
    assert list(lay["mtb_relation"]["fields"]) == list(dt.names)
    for f, off in lay["mtb_relation"]["fields"].items():
        assert dt.fields[f][1] == off, f


@pytest.mark.gpu
def test_unsupported_parameters_give_their_status_codes():
    from metabuli_work_amd._abi import MtbGroupStats
    from metabuli_work_amd._lib import lib
    from metabuli_work_amd.grouping import GroupParams

    L = lib()
    maps = np.zeros(3 * 49, np.uint32)
    e = _relations(np.array([(1, 2, 20)], np.int64))

    def run(par, n=48, total=15 * 48):
        cp = par.to_c()
        st = MtbGroupStats()
        return L.mtb_group_make_groups(0, e.ctypes.data, 1, n, total, ctypes.byref(cp), maps.ctypes.data, ctypes.byref(st))

    ok = GroupParams(min_overlap_ratio=1.0)
    assert run(ok) == 0
    assert run(GroupParams(min_overlap_ratio=1.0, merge_support_ratio=0.1)) == -6  # MTB_ERR_UNSUPPORTED
    assert run(GroupParams(min_overlap_ratio=1.0, merge_max_unit_reads=100)) == -6
    assert run(ok, total=48) == -1  # coreThr = 1 < 2: MTB_ERR_ARG
    assert b"core threshold" in L.mtb_last_error()
    assert run(ok, n=0xFFFFFFFF) == -1  # 2^32 - 1 reads
    assert run(GroupParams(min_overlap_ratio=0.0)) == -1
    assert run(GroupParams(min_overlap_ratio=1.0, weak_band_ratio=1.0)) == -1


# ---- extraction -----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def ref_kmers():
    return np.load(GOLDEN / "ref_group_kmers.npz")


def _pairs_sorted(values, ids):
    o = np.lexsort((ids, values))
    return np.asarray(values)[o], np.asarray(ids)[o]


@pytest.mark.gpu
@pytest.mark.parametrize("name,syncmer,smer,cuts", [("fmt3", 0, 5, (0,)), ("fmt5_s5", 1, 5, (0, 61, 100)),
                                                    ("fmt5_s6", 1, 6, (0,))])
def test_kmers_equal_reference_scanners(name, syncmer, smer, cuts):
    """kmers() equals the reference's fillQueryKmerBuffer over KmerScanner_dna2aa / SyncmerScanner_dna2aa as
    a multiset of (value, seqID); the paired reads run in seq_mode 2 and the single-end ones in seq_mode 1,
    the syncmer-5 case in several add_batch calls (IDs continue)."""
    from metabuli_work_amd.grouping import GroupParams, ReadGrouper

    g = ref_kmers()
    s1, s2 = g["seq1"].tolist(), g["seq2"].tolist()
    want_v, want_id = g[f"{name}_value"], g[f"{name}_seq"]
    for paired in (True, False):
        idx = [i for i in range(len(s1)) if bool(s2[i]) == paired]
        new_id = np.zeros(len(s1) + 1, np.uint32)
        new_id[np.array(idx) + 1] = np.arange(1, len(idx) + 1)
        keep = np.isin(want_id, np.array(idx) + 1)
        wv, wi = _pairs_sorted(want_v[keep], new_id[want_id[keep]])
        par = GroupParams(seq_mode=2 if paired else 1, syncmer=syncmer, smer_len=smer)
        with ReadGrouper(par) as rg:
            bounds = [c for c in cuts if c < len(idx)] + [len(idx)]
            for a, b in zip(bounds[:-1], bounds[1:]):
                rg.add_reads([s1[i] for i in idx[a:b]], [s2[i] for i in idx[a:b]] if paired else None)
            assert rg.reads == len(idx)
            gv, gi = _pairs_sorted(*rg.kmers())
        assert len(gv) == len(wv) and len(wv) > 1000, (name, paired, len(gv), len(wv))
        assert np.array_equal(gv, wv) and np.array_equal(gi, wi), (name, paired)


# ---- edges ----------------------------------------------------------------------------------------

M_CLASSES = (1, 2, 3, 63, 64, 65, 256, 257, 1000, 1001)


@functools.lru_cache(maxsize=None)
def block_reads():
    """Hand-made single-end reads: one shared 36-nt block per class (so its 12-mer is in m reads) followed
    by a 36-nt block of the read's own, all blocks distinct; plus two reads sharing three blocks (a pair
    with several shared k-mers far apart in value)."""
    rng = np.random.default_rng(11)
    n_blocks = sum(M_CLASSES) + len(M_CLASSES) + 8
    pool = set()
    while len(pool) < n_blocks:
        pool.add(bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 36)]))
    pool = sorted(pool)
    rng.shuffle(pool)
    it = iter(pool)
    reads = []
    for m in M_CLASSES:
        shared = next(it)
        reads += [shared + next(it) for _ in range(m)]
    a, b, c = next(it), next(it), next(it)
    reads += [a + b + c + next(it), next(it) + a + b + c]
    order = rng.permutation(len(reads))  # a class's reads are spread over the IDs
    return [reads[i] for i in order]


@functools.lru_cache(maxsize=None)
def block_run(cap, quantile=0.0, budget=0, split=False):
    """(kmers, stats, edges, skipped) of the block reads on the device."""
    from metabuli_work_amd.grouping import GroupParams, ReadGrouper

    reads = block_reads()
    par = GroupParams(seq_mode=1, syncmer=0, max_kmer_reads=cap, max_kmer_quantile=quantile)
    with ReadGrouper(par) as rg:
        if split:  # classes span the two batches
            rg.add_reads(reads[:len(reads) // 2])
            rg.add_reads(reads[len(reads) // 2:])
        else:
            rg.add_reads(reads)
        km = rg.kmers()
        st = rg.build_edges(budget)
        return km, st, rg.edges(), rg.skipped()


@functools.lru_cache(maxsize=None)
def block_expect(cap, quantile=0.0):
    km = block_run(1000)[0]
    return group_expect.edges_from_kmers(km[0], km[1], max_kmer_reads=cap, max_kmer_quantile=quantile)


def _check_edges(run, exp):
    _, st, edges, (sv, sm) = run
    assert np.array_equal(np.stack([edges["id1"], edges["id2"], edges["weight"]], 1).astype(np.int64), exp["edges"])
    assert not edges["pad"].any()
    assert np.array_equal(np.stack([sv, sm.astype(np.uint64)], 1), exp["skipped"])
    assert st["hist_kmers"] == exp["hist_kmers"] and st["hist_pairs"] == exp["hist_pairs"]
    assert (st["cap"], st["distinct_kmers"], st["skipped_kmers"]) == (exp["cap"], exp["distinct"], len(exp["skipped"]))
    assert st["kept_pair_occurrences"] == exp["kept_pair_occurrences"] and st["edges"] == len(exp["edges"])


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [1000, 0])
def test_edges_equal_expectation_for_every_m_class(cap):
    exp = block_expect(cap)
    ms = set(exp["runs"][:, 1].tolist())
    assert set(M_CLASSES) <= ms, "the shared blocks fix m"
    assert (len(exp["skipped"]) > 0) == (cap == 1000) and (cap == 0 or (exp["skipped"][:, 1] == 1001).all())
    _check_edges(block_run(cap), exp)


@pytest.mark.gpu
def test_edges_of_a_run_spanning_two_batches():
    a, b = block_run(1000), block_run(1000, split=True)
    assert np.array_equal(np.sort(a[0][0]), np.sort(b[0][0])) and np.array_equal(a[2], b[2])
    _check_edges(b, block_expect(1000))


@pytest.mark.gpu
def test_quantile_cap():
    """max_kmer_reads = 0: the cap comes from the histogram (capFromQuantile)."""
    exp = block_expect(0, 0.9)
    assert 0 < exp["cap"] < 1000 and len(exp["skipped"]) > 0
    _check_edges(block_run(0, 0.9), exp)


@pytest.mark.gpu
def test_pair_budget_rounds_give_identical_edges():
    """A budget of exactly the largest kept clique: several rounds, and the two 12-mers of the m = 1000
    block (forward and reverse strand: every pair of its reads holds both) land in different rounds, so a
    pair's occurrences are split across rounds and summed by the cross-round merge."""
    exp = block_expect(1000)
    budget = exp["max_clique"]
    assert budget == 1000 * 999 // 2
    runs = exp["runs"][exp["runs"][:, 1] <= 1000]
    rounds, used, big = 0, 0, []
    for m in runs[:, 1].tolist():  # the greedy rounds of the build, over the kept runs in value order
        p = m * (m - 1) // 2
        if used + p > budget:
            rounds, used = rounds + 1, 0
        used += p
        if m == 1000:
            big.append(rounds)
    assert len(big) >= 2 and len(set(big)) == len(big) and rounds + 1 >= 3
    one = block_run(1000)
    many = block_run(1000, budget=budget)
    assert one[1]["rounds"] == 1 and many[1]["rounds"] >= 3
    assert np.array_equal(one[2], many[2])
    _check_edges(many, exp)


@pytest.mark.gpu
def test_budget_below_largest_clique_is_an_argument_error():
    from metabuli_work_amd._lib import MtbError
    from metabuli_work_amd.grouping import GroupParams, ReadGrouper

    with ReadGrouper(GroupParams(seq_mode=1, syncmer=0)) as rg:
        rg.add_reads(block_reads())
        with pytest.raises(MtbError, match=r"\(-1\).*largest kept clique"):
            rg.build_edges(1000 * 999 // 2 - 1)
        rg.build_edges()  # the grouper is still good: the same edges as a first build, and again
        first = rg.edges()
        rg.build_edges(1000 * 999 // 2)
        assert np.array_equal(first, block_run(1000)[2]) and np.array_equal(rg.edges(), first)


def _revcomp(s: bytes) -> bytes:
    return s[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))


@pytest.mark.gpu
def test_kmer_in_both_mates_and_strands_counts_once():
    from metabuli_work_amd.grouping import GroupParams, ReadGrouper

    rng = np.random.default_rng(5)
    x, y, z = (bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 90)]) for _ in range(3))
    reads1, reads2 = [x, x, z], [_revcomp(x), y, x]  # read 1 holds x's k-mers in both mates, on both strands
    with ReadGrouper(GroupParams(seq_mode=2, syncmer=0)) as rg:
        rg.add_reads(reads1, reads2)
        v, ids = rg.kmers()
        rg.build_edges()
        e = rg.edges()
    inst = np.stack([v, ids.astype(np.uint64)], 1)
    assert len(np.unique(inst[ids == 1], axis=0)) < (ids == 1).sum(), "read 1 repeats its k-mers"
    exp = group_expect.edges_from_kmers(v, ids)
    assert np.array_equal(np.stack([e["id1"], e["id2"], e["weight"]], 1).astype(np.int64), exp["edges"])
    assert len(e) == 3 and e["weight"][0] == len(np.unique(v[ids == 2][np.isin(v[ids == 2], v[ids == 1])]))


@pytest.mark.gpu
def test_identical_long_reads_saturate_at_65535():
    from metabuli_work_amd.grouping import GroupParams, ReadGrouper

    rng = np.random.default_rng(9)
    long_read = bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 70000)])
    with ReadGrouper(GroupParams(seq_mode=3, syncmer=0)) as rg:
        rg.add_reads([long_read, long_read])
        v, ids = rg.kmers()
        st = rg.build_edges()
        e = rg.edges()
    shared = len(np.unique(v))
    assert shared > 65535 and st["kept_pair_occurrences"] == shared
    assert e.tolist() == [(1, 2, 65535, 0)]


# ---- phases on resident edges, end to end ------------------------------------------------------------

@pytest.mark.gpu
def test_finish_equals_make_groups_on_the_edges():
    from metabuli_work_amd.grouping import GroupParams, ReadGrouper, make_groups

    par = GroupParams(seq_mode=1, syncmer=0, min_overlap_ratio=0.05)
    with ReadGrouper(par) as rg:
        rg.add_reads(block_reads())
        st = rg.build_edges()
        e = rg.edges()
        gm, fst = rg.finish()
    maps, mst = make_groups(e, rg.reads, st["kmers"], par)
    assert np.array_equal(gm, maps[2]) and gm.any()
    assert (fst["core_thr"], fst["weak_thr"]) == (mst["core_thr"], mst["weak_thr"])
    assert (fst["core_thr"], fst["weak_thr"]) == group_expect.thresholds(0.05, par.weak_band_ratio, st["kmers"], rg.reads)
    assert fst["groups_after"] == mst["groups_after"] and fst["grouped_after"] == mst["grouped_after"]


def _synthetic_pairs(n_pairs=20000, genome_len=400000, seed=3):
    """Pairs of 150-nt mates from 300-nt fragments of three random genomes, either strand, 0.5% substitutions."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    genomes = acgt[rng.integers(0, 4, (3, genome_len))]
    g = rng.integers(0, 3, n_pairs)
    st = rng.integers(0, genome_len - 300, n_pairs)
    frag = genomes[g[:, None], st[:, None] + np.arange(300)[None, :]]
    comp = np.zeros(256, np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    rc = comp[frag[:, ::-1]]
    flip = rng.random(n_pairs) < 0.5
    fwd, rev = np.where(flip[:, None], rc, frag), np.where(flip[:, None], frag, rc)
    m1, m2 = fwd[:, :150].copy(), rev[:, :150].copy()
    for m in (m1, m2):
        sub = rng.random(m.shape) < 0.005
        m[sub] = acgt[rng.integers(0, 4, int(sub.sum()))]
    off = (np.arange(n_pairs + 1) * 150).astype(np.uint64)
    return m1.reshape(-1), off, m2.reshape(-1), off.copy()


def _fastq(seq, off):
    n = len(off) - 1
    rows = seq.reshape(n, 150)
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, rows[i].tobytes(), b"I" * 150) for i in range(n))


@pytest.mark.gpu
def test_end_to_end_group_map_bytes(tmp_path):
    """group_reads over FASTQ files of about 20k synthetic pairs: the groupMap bytes equal the file written
    from the Python expectation (edges_from_kmers + the reference-checked phases), and two runs are
    byte-identical (groupMap, groups and skipped_kmers)."""
    from metabuli_work_amd.grouping import GroupParams, ReadGrouper, group_reads

    s1, o1, s2, o2 = _synthetic_pairs()
    (tmp_path / "r1.fq").write_bytes(_fastq(s1, o1))
    (tmp_path / "r2.fq").write_bytes(_fastq(s2, o2))
    par = GroupParams()
    outs = []
    for run in ("a", "b"):
        gm, st = group_reads(tmp_path / "r1.fq", tmp_path / "r2.fq", tmp_path / run, par, max_reads=7000)
        outs.append({f: (tmp_path / run / f).read_bytes() for f in ("groupMap", "groups", "skipped_kmers")})
    assert outs[0] == outs[1]
    with ReadGrouper(par) as rg:
        rg.add_batch(s1, o1, s2, o2)
        v, ids = rg.kmers()
    assert st["reads"] == 20000 and st["kmers"] == len(v)
    exp = group_expect.edges_from_kmers(v, ids)
    assert st["edges"] == len(exp["edges"]) > 20000
    core, weak = group_expect.thresholds(par.min_overlap_ratio, par.weak_band_ratio, len(v), 20000)
    assert (st["core_thr"], st["weak_thr"]) == (core, weak)
    maps = group_expect.phases(20000, exp["edges"], core, weak)
    assert outs[0]["groupMap"] == group_expect.group_map_bytes(maps[2])
    assert np.array_equal(gm, maps[2]) and (maps[2] != 0).sum() > 5000
    first = outs[0]["groups"].split(b"\n")[0].split(b"\t")
    assert first[-1] == b"" and int(first[0]) == int(first[1]) == int(maps[2][maps[2] != 0].min())


@pytest.mark.gpu
def test_pair_with_a_mate_too_short_emits_nothing():
    """The shared empty-read rule with kmerLen 12 (KmerExtractor.cpp:451-494): a pair one of whose mates
    holds no 12-mer is dropped whole; its ID is still counted. A single-end read that short emits nothing."""
    from metabuli_work_amd.grouping import GroupParams, ReadGrouper

    rng = np.random.default_rng(4)
    x, y = (bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 150)]) for _ in range(2))
    with ReadGrouper(GroupParams(seq_mode=2, syncmer=0)) as rg:
        # 37 nt: 33 covered, 11 codons, no window; 38 nt: 36 covered, one window; 150 nt: 49 codons, 38 windows
        rg.add_reads([x, x[:37], x], [y[:37], y, y[:38]])
        _, ids = rg.kmers()
    assert rg.reads == 3 and set(ids.tolist()) == {3} and len(ids) == 6 * (38 + 1)
    with ReadGrouper(GroupParams(seq_mode=1, syncmer=0)) as rg:
        rg.add_reads([x[:37], x[:38], x[:2], b""])
        _, ids = rg.kmers()
    assert rg.reads == 4 and ids.tolist() == [2] * 6
