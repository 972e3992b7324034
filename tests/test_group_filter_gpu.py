"""The common-k-mer filter on the device (mtb_group_set_common_db / _kmers, the filtered mtb_group_add_batch,
mtb_group_filter_common) against the reference's own filterCommonKmers (tests/golden/ref_group_filter.npz)
and the filter's predicate (tests/group_filter_cases.py) — every comparison exact."""
import ctypes
import functools
import json
import pathlib
import subprocess

import numpy as np
import pytest

from tests import group_expect
from tests import group_filter_cases as gc

ROOT = pathlib.Path(__file__).resolve().parents[1]
CFG = {name: (syn, smer) for name, syn, smer in gc.CONFIGS}
FILTER_SYMBOLS = ["mtb_group_set_common_db", "mtb_group_set_common_kmers", "mtb_group_get_filter_stats",
                  "mtb_group_get_kmer_pos", "mtb_group_filter_common", "mtb_group_filter_constants"]


@functools.lru_cache(maxsize=None)
def fx():
    return gc.load()


@functools.lru_cache(maxsize=None)
def subset(cfg, paired):
    """The fixture's paired (or single-end) reads and the configuration's instances of those reads under the
    IDs a run of them alone gives: (reads1, reads2, value, id, pos, index into the configuration's instances)."""
    f = fx()
    s1, s2 = f["seq1"].tolist(), f["seq2"].tolist()
    idx = [i for i in range(len(s1)) if bool(s2[i]) == paired]
    new_id = np.zeros(len(s1) + 1, np.uint32)
    new_id[np.array(idx) + 1] = np.arange(1, len(idx) + 1)
    v, s, p, _ = gc.extraction(f, cfg)
    sel = np.nonzero(np.isin(s, np.array(idx) + 1))[0]
    return [s1[i] for i in idx], ([s2[i] for i in idx] if paired else None), v[sel], new_id[s[sel]], p[sel], sel


def _params(cfg, paired, **kw):
    from metabuli_work_amd.grouping import GroupParams

    return GroupParams(seq_mode=2 if paired else 1, syncmer=CFG[cfg][0], smer_len=CFG[cfg][1], **kw)


def _kmer_params(cfg):
    return {"syncmer": CFG[cfg][0], "smer_len": CFG[cfg][1], "kmer_format": 5 if CFG[cfg][0] else 3}


def _add(rg, r1, r2, cuts):
    bounds = [0] + [c for c in cuts if 0 < c < len(r1)] + [len(r1)]
    for a, b in zip(bounds[:-1], bounds[1:]):
        rg.add_reads(r1[a:b], r2[a:b] if r2 is not None else None)


def _stored(rg):
    v, ids = rg.kmers()
    return gc.multiset(v, ids, rg.kmer_pos())


# ---- positions --------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("cfg", list(CFG))
def test_positions_equal_reference_scanners(cfg):
    """With an empty set attached nothing is removed: the stored (value, seqID, pos) are the reference's
    fillQueryKmerBuffer output, mate 2 after getMaxCoveredLength(len1) + 3."""
    from metabuli_work_amd.grouping import ReadGrouper

    for paired in (True, False):
        r1, r2, v, ids, p, _ = subset(cfg, paired)
        with ReadGrouper(_params(cfg, paired)) as rg:
            rg.set_common_kmers([])
            _add(rg, r1, r2, ())
            got = _stored(rg)
            st = rg.filter_stats()
        assert len(v) > 1000 and np.array_equal(got, gc.multiset(v, ids, p)), (cfg, paired)
        assert (st["extracted"], st["db_values"], st["hit"], st["removed"], st["kept"]) == (len(v), 0, 0, 0, len(v))


# ---- kept k-mers ------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("db", gc.DBS)
@pytest.mark.parametrize("cfg", list(CFG))
def test_kept_kmers_equal_reference_filter(cfg, db, tmp_path):
    """kmers() after the filtered add_batch equals what the reference's filterCommonKmers keeps, from a DB
    directory written from the stored values: paired and single-end, one batch and three batches cut inside
    the read list; the filter's counts are the fixture's."""
    from metabuli_work_amd.grouping import ReadGrouper

    dbv = gc.db_values(fx(), cfg, db)
    gc.write_db(tmp_path / "db", dbv, 4, _kmer_params(cfg))
    keep_ref = gc.reference_result(fx(), cfg, db)[0]
    for paired in (True, False):
        r1, r2, v, ids, p, sel = subset(cfg, paired)
        keep = keep_ref[sel]
        want = gc.multiset(v[keep], ids[keep], p[keep])
        hits = int(np.isin(v, dbv).sum())
        for cuts in ((), (len(r1) // 3, len(r1) // 3 + 1 + len(r1) // 2)):
            with ReadGrouper(_params(cfg, paired)) as rg:
                rg.set_common_db(tmp_path / "db")
                _add(rg, r1, r2, cuts)
                got = _stored(rg)
                st = rg.filter_stats()
                gst = rg.build_edges()
            assert np.array_equal(got, want), (cfg, db, paired, cuts)
            assert (st["extracted"], st["hit"], st["removed"], st["kept"]) == (len(v), hits, len(v) - len(want), len(want))
            assert st["db_values"] == len(np.unique(dbv)) and st["params_checked"] == 1
            assert gst["kmers"] == len(want)
            assert st["removed"] + st["kept"] == st["extracted"] and st["hit"] <= st["removed"]


@pytest.mark.gpu
def test_kept_kmers_from_host_values_and_chunked_decode(tmp_path, monkeypatch):
    """The same kept k-mers through set_common_kmers, and through a diffIdx decoded in chunks of 1000 words
    (k-mers cut by a chunk's end, repeats across chunk ends)."""
    from metabuli_work_amd.grouping import ReadGrouper

    cfg, db = "fmt5_s5", "fifth"
    dbv = gc.db_values(fx(), cfg, db)
    r1, r2, v, ids, p, sel = subset(cfg, True)
    keep = gc.reference_result(fx(), cfg, db)[0][sel]
    want = gc.multiset(v[keep], ids[keep], p[keep])
    with ReadGrouper(_params(cfg, True)) as rg:
        rg.set_common_kmers(dbv)
        _add(rg, r1, r2, ())
        assert np.array_equal(_stored(rg), want)
        assert rg.filter_stats()["db_values"] == len(np.unique(dbv))
    gc.write_db(tmp_path / "db", dbv, 4)
    assert (tmp_path / "db" / "diffIdx").stat().st_size > 2 * 5000
    monkeypatch.setenv("MTB_DECODE_CHUNK_WORDS", "1000")
    with ReadGrouper(_params(cfg, True)) as rg:
        rg.set_common_db(tmp_path / "db")
        _add(rg, r1, r2, ())
        assert np.array_equal(_stored(rg), want)
        st = rg.filter_stats()
    assert st["db_values"] == len(np.unique(dbv)) and st["params_checked"] == 0  # no kmer_params file


# ---- the staged kernels at their edges ----------------------------------------------------------------------

def _check_staged(dbv, v, ids, p):
    from metabuli_work_amd.grouping import filter_common

    hit, keep = filter_common(dbv, v, ids, p)
    whit, wkeep = gc.predicate(dbv, v, ids, p)
    assert np.array_equal(hit, whit) and np.array_equal(keep, wkeep)
    return hit, keep


def _index_sizes():
    """DB sizes around every size at which the set's index changes shape: one leaf to two (set_leaf), and
    the top level from every leaf head to every second one (set_leaf * set_top), then every third."""
    from metabuli_work_amd.grouping import filter_constants

    c = filter_constants()
    leaf, full = c["set_leaf"], c["set_leaf"] * c["set_top"]
    assert (leaf, c["set_top"]) == (64, 4096)
    return [0, 1, 2, leaf - 1, leaf, leaf + 1, 2 * leaf, 2 * leaf + 1, full - 1, full, full + 1, 2 * full, 2 * full + 1]


@pytest.mark.gpu
def test_membership_at_every_index_shape():
    rng = np.random.default_rng(31)
    pool = np.unique(rng.integers(2, (1 << 60) - 2, 600000, dtype=np.uint64))
    for n_db in _index_sizes():
        dbv = pool[:: max(1, len(pool) // max(n_db, 1))][:n_db].copy()
        assert len(dbv) == n_db
        if n_db >= 2 and n_db % 2:
            dbv[0] = 0  # value 0 in the DB on the odd sizes (the pool starts at 2)
        written = np.repeat(dbv, 1 + (np.arange(len(dbv)) % 5 == 0)) if n_db > 2 else dbv  # duplicates
        q = [np.array([0, 1, (1 << 60) - 1], np.uint64), rng.integers(0, 1 << 60, 500, dtype=np.uint64)]
        if n_db:
            lo, hi = dbv[0], dbv[-1]
            q.append(np.array([lo, hi, hi + np.uint64(1)] + ([lo - np.uint64(1)] if lo else []), np.uint64))
            q.append(rng.choice(dbv, 1500))
            heads = dbv[::64]  # leaf heads, their neighbours in value and in the array
            q += [heads, heads + np.uint64(1), heads[heads > 0] - np.uint64(1), dbv[63::64], dbv[-3:]]
        v = np.concatenate(q)
        rng.shuffle(v)
        ids = np.sort(rng.integers(1, 400, len(v))).astype(np.uint32)
        p = rng.integers(0, 300, len(v)).astype(np.uint32)
        hit, _ = _check_staged(written, v, ids, p)
        assert hit.sum() >= (2 if n_db else 0) and not hit.all()


@pytest.mark.gpu
def test_neighbourhood_edges():
    from metabuli_work_amd.grouping import filter_common, filter_constants

    lds = filter_constants()["lds_bits"]
    H, N = 7, 9  # a DB value, a value of no DB
    dbv = np.array([H], np.uint64)
    rows = []  # (value, read, pos)
    # read 2: a hit at pos 0 (no wrap to anything): 0 and 1 fall, 2 stays
    rows += [(H, 2, 0), (N, 2, 0), (N, 2, 1), (N, 2, 2)]
    # read 5 (IDs with gaps): hits at x and x + 2, so x + 1 falls to both; x - 1, x + 3 fall, x - 2, x + 4 stay
    rows += [(N, 5, x) for x in range(98, 105)] + [(H, 5, 100), (H, 5, 102)]
    # reads 6 and 7: identical pos lists, only 7 has a hit; read 8 starts at pos 0 right after a hit at 7's last pos
    rows += [(N, 6, x) for x in (10, 11, 12, 40)] + [(N, 7, 10), (H, 7, 11), (N, 7, 12), (H, 7, 40)]
    rows += [(N, 8, 0), (N, 8, 41), (N, 8, 39)]
    # reads 20 .. 22: the last hit at lds - 2, lds - 1, lds (the bitmap moves from LDS to HBM at lds - 1)
    for r, x in ((20, lds - 2), (21, lds - 1), (22, lds)):
        rows += [(N, r, x - 2), (N, r, x - 1), (H, r, x), (N, r, x + 1), (N, r, x + 2), (N, r, 0)]
    # read 30: 20,000 positions in no order, hits spread over them; read 31 after it has none
    rng = np.random.default_rng(8)
    pos = rng.permutation(20000)
    hits = set(rng.choice(20000, 40, replace=False).tolist()) | {0, 19999}
    rows += [(H if x in hits else N, 30, int(x)) for x in pos]
    rows += [(N, 31, x) for x in (0, 1, 19998, 19999, 20000)]
    a = np.array(rows, np.uint64)
    hit, keep = _check_staged(dbv, a[:, 0], a[:, 1].astype(np.uint32), a[:, 2].astype(np.uint32))
    r, p = a[:, 1], a[:, 2]
    assert p[(r == 2) & keep].tolist() == [2]
    assert sorted(p[(r == 5) & keep].tolist()) == [98, 104]
    assert keep[r == 6].all() and not keep[r == 7].any() and keep[r == 8].all() and keep[r == 31].all()
    for rr in (20, 21, 22):
        assert keep[r == rr].sum() == 3
    assert 0 < keep[r == 30].sum() < 20000 - 42
    # n = 0, an empty DB, and both
    for d, n in ((dbv, 0), (np.zeros(0, np.uint64), 5), (np.zeros(0, np.uint64), 0)):
        h, k = filter_common(d, a[:n, 0], a[:n, 1].astype(np.uint32), a[:n, 2].astype(np.uint32))
        assert len(h) == n and not h.any() and k.all()


# ---- thresholds ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def family_reads():
    """60 single-end reads of 180 nt in 12 families: a family's reads share their first 120 nt."""
    rng = np.random.default_rng(17)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    reads = []
    for _ in range(12):
        shared = bytes(acgt[rng.integers(0, 4, 120)])
        reads += [shared + bytes(acgt[rng.integers(0, 4, 60)]) for _ in range(5)]
    order = rng.permutation(len(reads))
    return [reads[i] for i in order]


@pytest.mark.gpu
def test_thresholds_come_from_the_kept_count():
    from metabuli_work_amd._lib import MtbError
    from metabuli_work_amd.grouping import GroupParams, ReadGrouper, make_groups

    reads = family_reads()
    par = GroupParams(seq_mode=1, syncmer=0)
    with ReadGrouper(par) as rg:
        rg.add_reads(reads)
        v, _ = rg.kmers()
        rg.build_edges()
        _, plain = rg.finish()
    distinct = np.unique(v)
    common = distinct[np.random.default_rng(2).random(len(distinct)) < 0.12]
    with ReadGrouper(par) as rg:
        rg.set_common_kmers(common)
        rg.add_reads(reads)
        kept = rg.filter_stats()["kept"]
        st = rg.build_edges()
        e = rg.edges()
        gm, fst = rg.finish()
    assert st["kmers"] == kept < len(v) and len(e) > 0
    maps, mst = make_groups(e, len(reads), kept, par)
    assert np.array_equal(gm, maps[2]) and gm.any()
    want = group_expect.thresholds(par.min_overlap_ratio, par.weak_band_ratio, kept, len(reads))
    assert (fst["core_thr"], fst["weak_thr"]) == (mst["core_thr"], mst["weak_thr"]) == want
    assert fst["core_thr"] < plain["core_thr"], "the set moves the core threshold"
    with ReadGrouper(par) as rg:  # every k-mer common: nothing is left, the core threshold resolves to 0
        rg.set_common_kmers(distinct)
        rg.add_reads(reads)
        assert rg.filter_stats()["kept"] == 0 and rg.build_edges()["kmers"] == 0
        with pytest.raises(MtbError, match=r"\(-1\).*core threshold"):
            rg.finish()


# ---- end to end ---------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_end_to_end_with_a_common_db(tmp_path):
    """group_reads(..., common_db=dir) writes the groupMap and groups of: filter_common over the instances
    of the same reads, then the edge rule and the phases in Python. Without the argument, and with
    common_db=None, the files are the same bytes."""
    from metabuli_work_amd.grouping import GroupParams, ReadGrouper, filter_common, group_reads, write_group_files
    from tests.test_group_gpu import _fastq, _synthetic_pairs

    n = 3000
    s1, o1, s2, o2 = _synthetic_pairs(n_pairs=n, genome_len=60000, seed=5)
    (tmp_path / "r1.fq").write_bytes(_fastq(s1, o1))
    (tmp_path / "r2.fq").write_bytes(_fastq(s2, o2))
    par = GroupParams()
    with ReadGrouper(par) as rg:  # an empty set removes nothing and keeps the positions
        rg.set_common_kmers([])
        rg.add_batch(s1, o1, s2, o2)
        v, ids = rg.kmers()
        pos = rg.kmer_pos()
    distinct = np.unique(v)
    dbv = distinct[np.random.default_rng(3).random(len(distinct)) < 0.2]
    gc.write_db(tmp_path / "db", dbv, 4, {"syncmer": par.syncmer, "smer_len": par.smer_len, "kmer_format": 5})
    files = ("groupMap", "groups", "skipped_kmers")
    outs = {}
    for name, kw in (("plain", {}), ("none", {"common_db": None}), ("filtered", {"common_db": tmp_path / "db"})):
        gm, st = group_reads(tmp_path / "r1.fq", tmp_path / "r2.fq", tmp_path / name, par, max_reads=1100, **kw)
        outs[name] = ({f: (tmp_path / name / f).read_bytes() for f in files}, gm, st)
    assert outs["plain"][0] == outs["none"][0] and "filter" not in outs["none"][2]
    hit, keep = filter_common(dbv, v, ids, pos)
    assert 0 < keep.sum() < len(v) - hit.sum()
    got, gm, st = outs["filtered"]
    assert st["filter"]["kept"] == int(keep.sum()) == st["kmers"] and st["filter"]["hit"] == int(hit.sum())
    assert st["filter"]["extracted"] == len(v) and st["filter"]["params_checked"] == 1
    exp = group_expect.edges_from_kmers(v[keep], ids[keep])
    core, weak = group_expect.thresholds(par.min_overlap_ratio, par.weak_band_ratio, int(keep.sum()), n)
    assert (st["core_thr"], st["weak_thr"]) == (core, weak) and st["edges"] == len(exp["edges"])
    maps = group_expect.phases(n, exp["edges"], core, weak)
    assert np.array_equal(gm, maps[2]) and maps[2].any()
    assert got["groupMap"] == group_expect.group_map_bytes(maps[2])
    write_group_files(tmp_path / "want", maps[2])
    assert got["groups"] == (tmp_path / "want" / "groups").read_bytes()
    assert got["groupMap"] != outs["plain"][0]["groupMap"], "the filter changes the groups"


# ---- errors -------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_set_order_and_value_errors(tmp_path):
    from metabuli_work_amd._lib import MtbError
    from metabuli_work_amd.grouping import GroupParams, ReadGrouper, filter_common

    reads = family_reads()[:4]
    par = GroupParams(seq_mode=1, syncmer=0)
    gc.write_db(tmp_path / "db", [3, 9, 9, 1 << 50], 4)
    with ReadGrouper(par) as rg:
        rg.add_reads(reads)
        with pytest.raises(MtbError, match=r"\(-1\).*before the first batch"):
            rg.set_common_kmers([1, 2])
        with pytest.raises(MtbError, match=r"\(-1\).*before the first batch"):
            rg.set_common_db(tmp_path / "db")
        with pytest.raises(MtbError, match=r"\(-1\).*common k-mer set attached"):
            rg.kmer_pos()
    with ReadGrouper(par) as rg:
        rg.set_common_db(tmp_path / "db")
        assert rg.filter_stats()["db_values"] == 3
        with pytest.raises(MtbError, match=r"\(-1\).*attached already"):
            rg.set_common_kmers([1, 2])
        with pytest.raises(MtbError, match=r"\(-1\).*attached already"):
            rg.set_common_db(tmp_path / "db")
    with ReadGrouper(par) as rg:
        with pytest.raises(MtbError, match=r"\(-1\).*descend"):
            rg.set_common_kmers([1, 5, 4])
        rg.set_common_kmers([1, 4, 4, 5])  # the failed call attached nothing
        rg.add_reads(reads)
        assert rg.filter_stats()["db_values"] == 3
    one = np.ones(3, np.uint32)
    with pytest.raises(MtbError, match=r"\(-1\).*db_values descend"):
        filter_common([5, 4], [1, 2, 3], one, one)
    with pytest.raises(MtbError, match=r"\(-1\).*read_ids descend"):
        filter_common([4, 5], [1, 2, 3], [1, 3, 2], one)
    with pytest.raises(MtbError, match=r"\(-1\).*2\^31"):
        filter_common([4, 5], [1, 2, 3], one, [0, 1 << 31, 2])


@pytest.mark.gpu
def test_truncated_diffidx_is_a_db_error(tmp_path):
    from metabuli_work_amd._lib import MtbError
    from metabuli_work_amd.grouping import GroupParams, ReadGrouper

    words = gc.encode_diffidx([5, 1 << 40, (1 << 40) + (1 << 33)])
    assert len(words) == 1 + 3 + 3
    par = GroupParams(seq_mode=1, syncmer=0)
    for i, blob in enumerate((words[:-1].tobytes(), words.tobytes()[:-1], words[:2].tobytes())):
        d = tmp_path / f"db{i}"
        d.mkdir()
        (d / "diffIdx").write_bytes(blob)
        with ReadGrouper(par) as rg:
            with pytest.raises(MtbError, match=r"\(-4\).*mid k-mer"):
                rg.set_common_db(d)
            rg.set_common_kmers([])  # still attachable
    with ReadGrouper(par) as rg:
        with pytest.raises(MtbError, match=r"\(-2\)"):
            rg.set_common_db(tmp_path / "absent")
    d = tmp_path / "empty"
    d.mkdir()
    (d / "diffIdx").write_bytes(b"")
    with ReadGrouper(par) as rg:
        rg.set_common_db(d)
        assert rg.filter_stats()["db_values"] == 0


@pytest.mark.gpu
def test_kmer_params_mismatches(tmp_path):
    from metabuli_work_amd._lib import MtbError
    from metabuli_work_amd.grouping import GroupParams, ReadGrouper

    def attach(par, params, name):
        gc.write_db(tmp_path / name, [3, 9], 4, params)
        with ReadGrouper(par) as rg:
            rg.set_common_db(tmp_path / name)
            return rg.filter_stats()["params_checked"]

    syn = GroupParams(seq_mode=1, syncmer=1, smer_len=5)
    plain = GroupParams(seq_mode=1, syncmer=0, smer_len=5)
    assert attach(syn, {"syncmer": 1, "smer_len": 5, "kmer_format": 5}, "ok5") == 1
    assert attach(plain, {"syncmer": 0, "smer_len": 5, "kmer_format": 3}, "ok3") == 1
    assert attach(syn, None, "absent") == 0
    bad = [(syn, {"syncmer": 0, "smer_len": 5, "kmer_format": 5}, "DB syncmer 0 .*request syncmer 1"),
           (syn, {"syncmer": 1, "smer_len": 6, "kmer_format": 5}, "DB syncmer 1 smer_len 6 .*request syncmer 1 smer_len 5"),
           (syn, {"syncmer": 1, "smer_len": 5, "kmer_format": 3}, "kmer_format 3, request .*kmer_format 5"),
           (plain, {"syncmer": 0, "smer_len": 5, "kmer_format": 5}, "kmer_format 5, request .*kmer_format 3"),
           (plain, {"syncmer": 0, "smer_len": 6, "kmer_format": 3}, "smer_len 6 .*request syncmer 0 smer_len 5"),
           (syn, {"syncmer": 1, "smer_len": 5}, "kmer_format -1")]
    for i, (par, params, msg) in enumerate(bad):
        with pytest.raises(MtbError, match=r"\(-1\).*do not match.*" + msg):
            attach(par, params, f"bad{i}")


# ---- ABI ----------------------------------------------------------------------------------------------------

LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "mtb_gpu.h"
#define F(f) printf("%s\"" #f "\": %zu", first++ ? ", " : "", offsetof(mtb_group_filter_stats, f))
int main(void) {
  int first = 0;
  printf("{\"size\": %zu, \"fields\": {", sizeof(mtb_group_filter_stats));
  F(extracted); F(db_values); F(hit); F(removed); F(kept); F(params_checked); F(reserved); F(ms);
  printf("}}\n");
  return 0;
}
"""


@pytest.mark.gpu
def test_filter_symbols_exported_and_layout_matches_compiled_c(tmp_path):
    from metabuli_work_amd import _abi
    from metabuli_work_amd._lib import EXPORTED, lib

    L = lib()
    for s in FILTER_SYMBOLS:
        assert s in EXPORTED and hasattr(L, s), s
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_C)
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    lay = json.loads(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout)
    cls = _abi.MtbGroupFilterStats
    assert lay["size"] == ctypes.sizeof(cls) == 64
    assert list(lay["fields"]) == [f for f, _ in cls._fields_]
    for f, off in lay["fields"].items():
        assert getattr(cls, f).offset == off, f
