"""Read grouping on the GPU (the reference fork's groupGeneration workflow): the binding of the
mtb_group_* section of include/mtb_gpu.h.

apply_groups_arrays / apply_groups are the groupApplication workflow (GroupApplier): one representative
taxon per group, the weighted-majority label of its members, applied to the reads the classifier left
unclassified or scored low.

make_groups runs the three grouping phases (makeGroups, mergeBySupport at its defaults,
makeGroupsPhase2) on an edge list and returns the groupMap after each phase. filter_common runs the
common-k-mer filter's kernels (filterCommonKmers) on instance arrays.
"""
import ctypes
import dataclasses

import numpy as np

from ._abi import (MTB_INPUT_DEVICE, MTB_RETRY, RELATION_DTYPE, MtbGroupApplyParams, MtbGroupApplyStats,
                   MtbGroupFilterStats, MtbGroupParams, MtbGroupStats)
from ._lib import check, lib


@dataclasses.dataclass
class GroupParams:
    """setGroupGenerationDefaults (groupGeneration.cpp:9-58)."""
    seq_mode: int = 2
    syncmer: int = 1
    smer_len: int = 5
    max_kmer_reads: int = 1000
    max_kmer_quantile: float = 0.0
    min_overlap_ratio: float = 0.3
    weak_band_ratio: float = 0.3333
    merge_support_ratio: float = 0.0
    merge_max_unit_reads: int = 0

    def to_c(self) -> MtbGroupParams:
        return MtbGroupParams(reserved=0, **dataclasses.asdict(self))

    @classmethod
    def defaults(cls) -> "GroupParams":
        """The library's own defaults (mtb_group_default_params)."""
        p = MtbGroupParams()
        lib().mtb_group_default_params(ctypes.byref(p))
        return cls(**{f.name: getattr(p, f.name) for f in dataclasses.fields(cls)})


def stats_dict(st) -> dict:
    out = {}
    for name, _ in st._fields_:
        v = getattr(st, name)
        out[name] = list(v) if hasattr(v, "__len__") else v
    return out


def relations(id1, id2, weight) -> np.ndarray:
    """An edge list as mtb_relation records (pad 0)."""
    e = np.zeros(len(id1), RELATION_DTYPE)
    e["id1"], e["id2"], e["weight"] = id1, id2, weight
    return e


def make_groups(edges: np.ndarray, n_reads: int, total_kmers: int, par: GroupParams = None, device: int = 0):
    """The three phases on an edge list (RELATION_DTYPE). Returns (maps, stats): maps is a (3, n_reads + 1)
    uint32 array, the groupMap after Phase 1, 1.5 and 2 (column 0 unused)."""
    par = par or GroupParams()
    edges = np.ascontiguousarray(edges, RELATION_DTYPE)
    maps = np.zeros((3, n_reads + 1), np.uint32)
    st = MtbGroupStats()
    cp = par.to_c()
    check(lib().mtb_group_make_groups(device, edges.ctypes.data if len(edges) else None, len(edges), n_reads,
                                      total_kmers, ctypes.byref(cp), maps.ctypes.data, ctypes.byref(st)),
          "mtb_group_make_groups")
    return maps, stats_dict(st)


def filter_constants() -> dict:
    """The sizes at which the filter's kernels change path (mtb_group_filter_constants)."""
    c = (ctypes.c_uint32 * 4)()
    lib().mtb_group_filter_constants(ctypes.byref(c))
    return {"set_leaf": c[0], "set_top": c[1], "lds_bits": c[2]}


def filter_common(db_values, values, read_ids, pos, device: int = 0):
    """The common-k-mer filter on instance arrays in read order (read_ids non-descending) against the
    ascending db_values: (hit, keep), bool arrays. An instance is hit iff its value is in db_values and
    kept iff no hit of its read lies within one nucleotide of it."""
    db = np.ascontiguousarray(db_values, np.uint64)
    v = np.ascontiguousarray(values, np.uint64)
    r = np.ascontiguousarray(read_ids, np.uint32)
    p = np.ascontiguousarray(pos, np.uint32)
    if not (len(v) == len(r) == len(p)):
        raise ValueError("values, read_ids and pos differ in length")
    hit, keep = np.zeros(len(v), np.uint8), np.zeros(len(v), np.uint8)
    check(lib().mtb_group_filter_common(device, db.ctypes.data if len(db) else None, len(db),
                                        v.ctypes.data if len(v) else None, r.ctypes.data if len(v) else None,
                                        p.ctypes.data if len(v) else None, len(v), hit.ctypes.data if len(v) else None,
                                        keep.ctypes.data if len(v) else None), "mtb_group_filter_common")
    return hit.astype(bool), keep.astype(bool)


def write_group_files(out_dir, group_map: np.ndarray) -> None:
    """saveGroupsToFile (GroupGenerator.cpp:2055-2090): groupMap ("i \\t groupId" per read) and groups
    (one line per group: the ID, then its members, each followed by a tab), groups and members ascending."""
    import pathlib

    out = pathlib.Path(out_dir)
    out.mkdir(parents=True, exist_ok=True)
    gm = np.asarray(group_map, np.uint32)
    n = len(gm) - 1
    with open(out / "groupMap", "wb") as f:
        ids = np.arange(1, n + 1)
        f.write("".join(f"{i}\t{g}\n" for i, g in zip(ids.tolist(), gm[1:].tolist())).encode())
    members = np.nonzero(gm[1:])[0] + 1
    order = np.lexsort((members, gm[members]))
    members = members[order]
    labels = gm[members]
    with open(out / "groups", "wb") as f:
        start = 0
        lines = []
        bounds = np.nonzero(np.diff(labels))[0] + 1 if len(labels) else np.array([], np.int64)
        for end in list(bounds) + ([len(labels)] if len(labels) else []):
            lines.append(f"{labels[start]}\t" + "".join(f"{m}\t" for m in members[start:end].tolist()) + "\n")
            start = end
        f.write("".join(lines).encode())


def _flat(reads):
    """Concatenated bases and n + 1 offsets of a list of str / bytes reads."""
    bs = [r.encode() if isinstance(r, str) else bytes(r) for r in reads]
    off = np.zeros(len(bs) + 1, np.uint64)
    off[1:] = np.cumsum([len(b) for b in bs], dtype=np.uint64)
    seq = np.frombuffer(b"".join(bs) or b"\0", np.uint8).copy()
    return seq, off


class ReadGrouper:
    """One grouping run on a device (mtb_grouper): add_batch ... build_edges, edges / skipped, finish."""

    def __init__(self, par: GroupParams = None, device: int = 0):
        self.par = par or GroupParams()
        self._h = ctypes.c_void_p()
        cp = self.par.to_c()
        check(lib().mtb_group_open(ctypes.byref(cp), device, ctypes.byref(self._h)), "mtb_group_open")
        self.reads = 0
        self.stats = None

    def close(self):
        if self._h:
            lib().mtb_group_close(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_common_db(self, db_dir):
        """Attach the common-k-mer DB at db_dir (its diffIdx, and kmer_params when present); before the
        first batch, at most once."""
        check(lib().mtb_group_set_common_db(self._h, str(db_dir).encode()), "mtb_group_set_common_db")

    def set_common_kmers(self, values):
        """Attach the common k-mers from an ascending array (repeats allowed, may be empty)."""
        v = np.ascontiguousarray(values, np.uint64)
        check(lib().mtb_group_set_common_kmers(self._h, v.ctypes.data if len(v) else None, len(v)),
              "mtb_group_set_common_kmers")

    def filter_stats(self) -> dict:
        st = MtbGroupFilterStats()
        check(lib().mtb_group_get_filter_stats(self._h, ctypes.byref(st)), "mtb_group_get_filter_stats")
        return stats_dict(st)

    def kmer_pos(self):
        """pos of the instances kmers() returns (with a common-k-mer set, before build_edges)."""
        n = ctypes.c_uint64()
        check(lib().mtb_group_get_kmer_pos(self._h, None, 0, ctypes.byref(n)), "mtb_group_get_kmer_pos")
        p = np.zeros(n.value, np.uint32)
        check(lib().mtb_group_get_kmer_pos(self._h, p.ctypes.data, n.value, ctypes.byref(n)), "mtb_group_get_kmer_pos")
        return p

    def add_batch(self, seq1, off1, seq2=None, off2=None, flags: int = 0):
        """A batch in mtb_classify_batch's flat layout (uint8 bases, n + 1 uint64 offsets), or device
        pointers (ints) with flags = MTB_INPUT_DEVICE and off1 = (pointer, n_reads)."""
        if isinstance(off1, tuple):
            p_off1, n = off1
            p_seq1, p_seq2, p_off2 = seq1, seq2, (off2[0] if off2 else None)
        else:
            seq1 = np.ascontiguousarray(seq1, np.uint8)
            off1 = np.ascontiguousarray(off1, np.uint64)
            n = len(off1) - 1
            p_seq1, p_off1, p_seq2, p_off2 = seq1.ctypes.data, off1.ctypes.data, None, None
            if seq2 is not None:
                seq2 = np.ascontiguousarray(seq2, np.uint8)
                off2 = np.ascontiguousarray(off2, np.uint64)
                p_seq2, p_off2 = seq2.ctypes.data, off2.ctypes.data
        check(lib().mtb_group_add_batch(self._h, p_seq1, p_off1, p_seq2, p_off2, n, flags), "mtb_group_add_batch")
        self.reads += n

    def add_reads(self, reads1, reads2=None):
        """A batch from lists of str / bytes reads."""
        s1, o1 = _flat(reads1)
        if reads2 is None:
            return self.add_batch(s1, o1)
        s2, o2 = _flat(reads2)
        return self.add_batch(s1, o1, s2, o2)

    def kmers(self):
        """(values, read_ids) of the k-mer instances extracted so far."""
        n = ctypes.c_uint64()
        check(lib().mtb_group_get_kmers(self._h, None, None, 0, ctypes.byref(n)), "mtb_group_get_kmers")
        v, r = np.zeros(n.value, np.uint64), np.zeros(n.value, np.uint32)
        check(lib().mtb_group_get_kmers(self._h, v.ctypes.data, r.ctypes.data, n.value, ctypes.byref(n)),
              "mtb_group_get_kmers")
        return v, r

    def build_edges(self, pair_budget: int = 0) -> dict:
        st = MtbGroupStats()
        check(lib().mtb_group_build_edges(self._h, pair_budget, ctypes.byref(st)), "mtb_group_build_edges")
        self.stats = stats_dict(st)
        return self.stats

    def edges(self) -> np.ndarray:
        n = ctypes.c_uint64()
        check(lib().mtb_group_get_edges(self._h, None, 0, ctypes.byref(n)), "mtb_group_get_edges")
        e = np.zeros(n.value, RELATION_DTYPE)
        check(lib().mtb_group_get_edges(self._h, e.ctypes.data, n.value, ctypes.byref(n)), "mtb_group_get_edges")
        return e

    def skipped(self):
        """(values, m) of the k-mers over the cap."""
        n = ctypes.c_uint64()
        check(lib().mtb_group_get_skipped(self._h, None, None, 0, ctypes.byref(n)), "mtb_group_get_skipped")
        v, m = np.zeros(n.value, np.uint64), np.zeros(n.value, np.uint32)
        check(lib().mtb_group_get_skipped(self._h, v.ctypes.data, m.ctypes.data, n.value, ctypes.byref(n)),
              "mtb_group_get_skipped")
        return v, m

    def finish(self):
        """The three phases on the resident edges: (groupMap of reads + 1 entries, stats)."""
        gm = np.zeros(self.reads + 1, np.uint32)
        st = MtbGroupStats()
        check(lib().mtb_group_finish(self._h, gm.ctypes.data, ctypes.byref(st)), "mtb_group_finish")
        self.stats = stats_dict(st)
        return gm, self.stats


def group_reads(query1, query2, out_dir, par: GroupParams = None, device: int = 0, pair_budget: int = 0,
                max_reads: int = 1 << 20, max_bases: int = 1 << 30, common_db=None):
    """groupGeneration over FASTA / FASTQ files (plain or gzip): batches streamed through mtb_reader_*,
    the graph and the phases on the device; writes out_dir/groupMap, groups and skipped_kmers
    ("value \\t m" per skipped k-mer). common_db: a common-k-mer DB directory (the reference's create_common_kmer_list's, or
    dbbuild.build_common_kmer_db's); every batch then goes
    through the common-k-mer filter and stats["filter"] holds its counts. Returns (groupMap, stats)."""
    import pathlib

    from ._abi import MtbReadBatch

    par = par or GroupParams()
    if (par.seq_mode == 2) != bool(query2):
        raise ValueError("seq_mode 2 takes two query files, seq_mode 1 and 3 take one")
    L = lib()
    rd = ctypes.c_void_p()
    check(L.mtb_reader_open(str(query1).encode(), str(query2).encode() if query2 else None, ctypes.byref(rd)),
          "mtb_reader_open")
    try:
        with ReadGrouper(par, device) as g:
            if common_db is not None:
                g.set_common_db(common_db)
            batch = MtbReadBatch()
            while True:
                check(L.mtb_reader_next(rd, max_reads, max_bases, ctypes.byref(batch)), "mtb_reader_next")
                if batch.n_reads == 0:
                    break
                check(L.mtb_group_add_batch(g._h, batch.seq1, ctypes.cast(batch.off1, ctypes.c_void_p), batch.seq2,
                                            ctypes.cast(batch.off2, ctypes.c_void_p) if query2 else None,
                                            batch.n_reads, 0), "mtb_group_add_batch")
                g.reads += batch.n_reads
            g.build_edges(pair_budget)
            sv, sm = g.skipped()
            gm, st = g.finish()
            if common_db is not None:
                st["filter"] = g.filter_stats()
    finally:
        L.mtb_reader_close(rd)
    write_group_files(out_dir, gm)
    with open(pathlib.Path(out_dir) / "skipped_kmers", "wb") as f:
        f.write("".join(f"{v}\t{m}\n" for v, m in zip(sv.tolist(), sm.tolist())).encode())
    return gm, st


# ---- group application (mtb_group_apply*, the reference's GroupApplier) -----------------------------
@dataclasses.dataclass
class ApplyParams:
    """setGroupApplicationDefaults (groupApplication.cpp:7-15): weight_mode 0 uniform, 1 score,
    2 score^2; a member votes with score >= min_vote_score (modes 1 and 2)."""
    weight_mode: int = 1
    min_vote_score: float = 0.15

    def to_c(self) -> MtbGroupApplyParams:
        return MtbGroupApplyParams(weight_mode=self.weight_mode, min_vote_score=self.min_vote_score)

    @classmethod
    def defaults(cls) -> "ApplyParams":
        """The library's own defaults (mtb_group_apply_default_params)."""
        p = MtbGroupApplyParams()
        lib().mtb_group_apply_default_params(ctypes.byref(p))
        return cls(weight_mode=p.weight_mode, min_vote_score=p.min_vote_score)


def apply_constants() -> dict:
    """The sizes at which the applier's kernels change path (mtb_group_apply_constants)."""
    c = (ctypes.c_uint32 * 4)()
    lib().mtb_group_apply_constants(ctypes.byref(c))
    return {"slice": c[0], "thread_labels": c[1], "wave_labels": c[2]}


def _taxonomy_struct(taxo):
    from .dbbuild import HostDb

    h = HostDb(taxo)
    return h, h.c_struct()


def lineage_ranks(taxo) -> np.ndarray:
    """The lineage rank of every node of taxo (node order), as the applier uploads it."""
    keep, h = _taxonomy_struct(taxo)
    out = np.zeros(len(taxo.taxid), np.int32)
    check(lib().mtb_group_apply_lineage_ranks(ctypes.byref(h), out.ctypes.data), "mtb_group_apply_lineage_ranks")
    return out


def apply_groups_arrays(group_map, tax_ids, scores, taxo, par: ApplyParams = None, device: int = 0):
    """One representative taxon per group and the per-read labels after applying it (mtb_group_apply).

    group_map: reads + 1 uint32 entries as ReadGrouper.finish() returns them (entry 0 unused); tax_ids:
    int32 internal taxIDs of taxo (a synth.Taxonomy: taxid, parent, rank, name), 0 = unclassified;
    scores: float32 (None in weight mode 0). numpy arrays, or torch tensors on the device: then nothing
    is copied to the host and the results are device tensors too (import torch before the library is first
    used). Returns (rep_groups, rep_tax, out_tax,
    out_classified, applied, stats): every group ID ascending with its representative (0 = none), and
    per read its label, is_classified and whether it took the representative.

        gm, _ = grouper.finish()                          # ReadGrouper
        res = classifier.classify(reads)                  # RESULT_DTYPE records
        groups, reps, tax, cls, applied, st = apply_groups_arrays(
            gm, res["classification"], res["score"], taxo, ApplyParams.defaults())
    """
    par = par or ApplyParams.defaults()
    keep, h = _taxonomy_struct(taxo)
    cp = par.to_c()
    st = MtbGroupApplyStats()
    on_device = hasattr(group_map, "data_ptr")
    if on_device:
        import torch

        dev = group_map.device
        gm = group_map.to(torch.int32) if group_map.dtype not in (torch.int32, torch.uint32) else group_map
        gm = gm.contiguous()
        tx = tax_ids.to(device=dev, dtype=torch.int32).contiguous()
        sc = None if scores is None else scores.to(device=dev, dtype=torch.float32).contiguous()
        n = gm.numel() - 1
        if tx.numel() != n or (sc is not None and sc.numel() != n):
            raise ValueError("group_map holds reads + 1 entries; tax_ids and scores one per read")
        out_tax = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        out_cls = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)
        out_app = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)
        cap = max(int(n), 1)
        rg = torch.zeros(cap, dtype=torch.int32, device=dev)
        rt = torch.zeros(cap, dtype=torch.int32, device=dev)
        ng = ctypes.c_uint64(cap)
        torch.cuda.synchronize(dev)
        check(lib().mtb_group_apply(device, ctypes.byref(h), ctypes.byref(cp), gm.data_ptr(), tx.data_ptr(),
                                    sc.data_ptr() if sc is not None else None, n, MTB_INPUT_DEVICE, rg.data_ptr(),
                                    rt.data_ptr(), ctypes.byref(ng), out_tax.data_ptr(), out_cls.data_ptr(),
                                    out_app.data_ptr(), ctypes.byref(st)), "mtb_group_apply")
        g = ng.value
        return rg[:g], rt[:g], out_tax[:n], out_cls[:n].bool(), out_app[:n].bool(), stats_dict(st)
    gm = np.ascontiguousarray(group_map, np.uint32)
    tx = np.ascontiguousarray(tax_ids, np.int32)
    sc = None if scores is None else np.ascontiguousarray(scores, np.float32)
    n = len(gm) - 1
    if n < 0 or len(tx) != n or (sc is not None and len(sc) != n):
        raise ValueError("group_map holds reads + 1 entries; tax_ids and scores one per read")
    out_tax, out_cls, out_app = np.zeros(n, np.int32), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    cap = max(len(np.unique(gm[1:][gm[1:] != 0])), 1)
    rg, rt = np.zeros(cap, np.uint32), np.zeros(cap, np.int32)
    ng = ctypes.c_uint64(cap)
    p = lambda a: a.ctypes.data if a is not None and len(a) else None
    check(lib().mtb_group_apply(device, ctypes.byref(h), ctypes.byref(cp), gm.ctypes.data, p(tx), p(sc), n, 0,
                                rg.ctypes.data, rt.ctypes.data, ctypes.byref(ng), p(out_tax), p(out_cls), p(out_app),
                                ctypes.byref(st)), "mtb_group_apply")
    g = ng.value
    return rg[:g], rt[:g], out_tax, out_cls.astype(bool), out_app.astype(bool), stats_dict(st)


def apply_label_sums(group_map, tax_ids, scores, taxo, par: ApplyParams = None, device: int = 0):
    """Staged: the per-label sums of apply_groups_arrays on host arrays: (groups, labels, sums) of every
    voting (group, label) pair, ascending (mtb_group_apply_label_sums)."""
    par = par or ApplyParams.defaults()
    keep, h = _taxonomy_struct(taxo)
    cp = par.to_c()
    gm = np.ascontiguousarray(group_map, np.uint32)
    tx = np.ascontiguousarray(tax_ids, np.int32)
    sc = None if scores is None else np.ascontiguousarray(scores, np.float32)
    n = len(gm) - 1
    cap = max(n, 1)
    keys, sums = np.zeros(cap, np.uint64), np.zeros(cap, np.float64)
    k = ctypes.c_uint64()
    p = lambda a: a.ctypes.data if a is not None and len(a) else None
    check(lib().mtb_group_apply_label_sums(device, ctypes.byref(h), ctypes.byref(cp), gm.ctypes.data, p(tx), p(sc), n,
                                           keys.ctypes.data, sums.ctypes.data, cap, ctypes.byref(k)),
          "mtb_group_apply_label_sums")
    keys, sums = keys[:k.value], sums[:k.value]
    vote = (keys & np.uint64(0xFFFFFFFF)) != 0
    return ((keys[vote] >> np.uint64(32)).astype(np.uint32), (keys[vote] & np.uint64(0xFFFFFFFF)).astype(np.int32),
            sums[vote])


def apply_groups(group_dir, taxonomy_dir, classifications_tsv, out_dir, par: ApplyParams = None, taxid_col: int = 3,
                 score_col: int = 5, read_id_col: int = 2, device: int = 0, check_groups: bool = True) -> dict:
    """groupApplication over files (mtb_group_apply_files): group_dir holds groupMap and groups as
    group_reads wrote them, taxonomy_dir the dmp files, classifications_tsv the classifier's per-read
    TSV (columns 1-based). Writes out_dir/groupRep (groups ascending) and
    out_dir/updated_classifications.tsv; returns the stats. check_groups: also hold group_dir/groups
    against groupMap."""
    import pathlib

    par = par or ApplyParams.defaults()
    gd = pathlib.Path(group_dir)
    pathlib.Path(out_dir).mkdir(parents=True, exist_ok=True)
    cp = par.to_c()
    st = MtbGroupApplyStats()
    groups = str(gd / "groups").encode() if check_groups and (gd / "groups").exists() else None
    check(lib().mtb_group_apply_files(groups, str(gd / "groupMap").encode(), str(taxonomy_dir).encode(),
                                      str(classifications_tsv).encode(), str(out_dir).encode(), ctypes.byref(cp),
                                      taxid_col, score_col, read_id_col, device, ctypes.byref(st)),
          "mtb_group_apply_files")
    return stats_dict(st)
