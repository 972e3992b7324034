"""Reference-DB construction and in-memory DB handles.

``build_db`` runs the GPU builder (mtb_build_db, csrc/mtb_build.hip): genomes + gene blocks +
taxonomy -> diffIdx / info / split / taxID_list in the reference's on-disk format
(IndexCreator.cpp:316-376,811-886). ``merge_dbs`` / ``merge_db_dirs`` / ``update_db`` run the GPU
merge (mtb_merge_db, csrc/mtb_merge.hip: IndexCreator::mergeTargetFiles<DB_CREATION>), the second
half of the reference's updateDB and of its builds of several flushes. ``HostDb`` keeps the arrays (and the numpy buffers the C
structs point into) alive, can write them as a DB directory, and yields the ``mtb_db_host``
struct that mtb_open_host / the oracle consume.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

import numpy as np

from ._abi import MTB_INPUT_DEVICE, MtbDbHost, MtbParams, ptr
from ._lib import check, lib


class MtbBuildInput(ctypes.Structure):
    _fields_ = [("seq", ctypes.c_void_p), ("off", ctypes.c_void_p), ("n_genomes", ctypes.c_uint32),
                ("genome_taxid", ctypes.c_void_p), ("blk_genome", ctypes.c_void_p), ("blk_start", ctypes.c_void_p),
                ("blk_end", ctypes.c_void_p), ("blk_strand", ctypes.c_void_p), ("n_blocks", ctypes.c_uint64),
                ("split_num", ctypes.c_int32), ("flags", ctypes.c_uint32)]


class MtbDbBuilt(ctypes.Structure):
    _fields_ = [("diff_idx", ctypes.c_void_p), ("n_diff_idx", ctypes.c_uint64),
                ("info", ctypes.c_void_p), ("n_info", ctypes.c_uint64),
                ("split", ctypes.c_void_p), ("n_split", ctypes.c_uint64),
                ("taxid_list", ctypes.c_void_p), ("n_taxid_list", ctypes.c_uint64),
                ("dev_values", ctypes.c_void_p), ("dev_info", ctypes.c_void_p)]


class MtbMergeInput(ctypes.Structure):
    _fields_ = [("diff_idx", ctypes.c_void_p), ("n_diff_idx", ctypes.c_uint64),
                ("info", ctypes.c_void_p), ("n_info", ctypes.c_uint64)]


MTB_BUILD_DEVICE_OUT = 8


def _pool(strings):
    enc = [s.encode() + b"\0" for s in strings]
    off = np.zeros(len(enc), np.uint64)
    if enc:
        off[1:] = np.cumsum([len(e) for e in enc[:-1]])
    return np.frombuffer(b"".join(enc) or b"\0", np.uint8).copy(), off


class HostDb:
    """A reference DB in host memory (diffIdx, info, split, taxID_list + taxonomy)."""

    def __init__(self, taxo, diff_idx=None, info=None, split=None, taxid_list=None):
        self.taxo = taxo
        self.diff_idx = diff_idx
        self.info = info
        self.split = split
        self.taxid_list = taxid_list
        self._rank_pool, self._rank_off = _pool(taxo.rank)
        self._name_pool, self._name_off = _pool(taxo.name)
        self._node_taxid = np.ascontiguousarray(taxo.taxid, np.int32)
        self._node_parent = np.ascontiguousarray(taxo.parent, np.int32)

    def c_struct(self) -> MtbDbHost:
        h = MtbDbHost()
        h.node_taxid, h.node_parent, h.n_nodes = ptr(self._node_taxid), ptr(self._node_parent), len(self._node_taxid)
        h.rank_pool, h.rank_off = ptr(self._rank_pool), ptr(self._rank_off)
        h.name_pool, h.name_off = ptr(self._name_pool), ptr(self._name_off)
        h.merged_old = h.merged_new = None
        h.n_merged = 0
        if self.diff_idx is not None:
            h.diff_idx, h.n_diff_idx = ptr(self.diff_idx), len(self.diff_idx)
            h.info, h.n_info = ptr(self.info), len(self.info)
            h.split, h.n_split = ptr(self.split), len(self.split) // 3
        if self.taxid_list is not None:
            h.taxid_list, h.n_taxid_list = ptr(self.taxid_list), len(self.taxid_list)
        return h

    @property
    def n_kmers(self) -> int:
        return 0 if self.info is None else len(self.info)

    @property
    def nbytes(self) -> int:
        return int(self.diff_idx.nbytes + self.info.nbytes)

    def write(self, directory: str, par: MtbParams) -> None:
        """Write a DB directory the reference's classify (and mtb_open) can read."""
        os.makedirs(directory, exist_ok=True)
        self.diff_idx.tofile(os.path.join(directory, "diffIdx"))
        self.info.tofile(os.path.join(directory, "info"))
        self.split.tofile(os.path.join(directory, "split"))
        with open(os.path.join(directory, "taxID_list"), "w") as f:
            f.write("".join(f"{t}\n" for t in self.taxid_list.tolist()))
        with open(os.path.join(directory, "db.parameters"), "w") as f:  # writeDbParameters
            f.write("DB_name\tsynthetic\nCreation_date\t1970-01-01\nMetabuli commit used to create the DB\tmtb-gpu\n")
            f.write(f"Reduced_alphabet\t{par.reduced_aa}\nAccession_level\t{par.accession_level}\n")
            f.write("Mask_mode\t0\nMask_prob\t0.900000\nSkip_redundancy\t1\n")
            f.write(f"Syncmer\t{par.syncmer}\n")
            if par.syncmer == 1:
                f.write(f"Syncmer_len\t{par.smer_len}\n")
            f.write(f"Kmer_format\t{par.kmer_format}\n")
        self.taxo.write_dmp(os.path.join(directory, "taxonomy"))


def _build_input(gen, device_seq, split_num, flags):
    inp = MtbBuildInput()
    if device_seq is not None:
        inp.seq, inp.off = device_seq[0].data_ptr(), device_seq[1].data_ptr()
        inp.flags = MTB_INPUT_DEVICE | flags
    else:
        inp.seq, inp.off = ptr(gen.seq).value, ptr(gen.off).value
        inp.flags = flags
    keep = [np.ascontiguousarray(a, np.int32) for a in (gen.taxid, gen.blk_genome, gen.blk_start, gen.blk_end,
                                                         gen.blk_strand)]
    inp.n_genomes = len(gen.taxid)
    inp.genome_taxid, inp.blk_genome, inp.blk_start, inp.blk_end, inp.blk_strand = [a.ctypes.data for a in keep]
    inp.n_blocks = len(keep[1])
    inp.split_num = split_num
    return inp, keep


def _lib_build():
    L = lib()
    L.mtb_build_db.argtypes = [ctypes.POINTER(MtbBuildInput), ctypes.POINTER(MtbDbHost), ctypes.POINTER(MtbParams),
                               ctypes.c_int, ctypes.POINTER(MtbDbBuilt)]
    L.mtb_build_common_db.argtypes = [ctypes.POINTER(MtbBuildInput), ctypes.POINTER(MtbDbHost), ctypes.c_int, ctypes.c_int,
                                      ctypes.c_int, ctypes.POINTER(MtbDbBuilt)]
    L.mtb_free_built.argtypes = [ctypes.POINTER(MtbDbBuilt)]
    L.mtb_merge_db.argtypes = [ctypes.POINTER(MtbMergeInput), ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64,
                               ctypes.POINTER(MtbDbHost), ctypes.POINTER(MtbParams), ctypes.c_int, ctypes.c_int,
                               ctypes.POINTER(MtbDbBuilt)]
    return L


def _take_built(hdb: "HostDb", out: MtbDbBuilt, L) -> "HostDb":
    """The malloc'd arrays of a mtb_db_built copied into hdb; the struct is released."""
    try:
        def arr(p, n, dt):
            if n == 0:
                return np.zeros(0, dt)
            return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(np.ctypeslib.as_ctypes_type(dt))),
                                         shape=(n,)).copy()
        hdb.diff_idx = arr(out.diff_idx, out.n_diff_idx, np.uint16)
        hdb.info = arr(out.info, out.n_info, np.uint32)
        hdb.split = arr(out.split, 3 * out.n_split, np.uint64)
        hdb.taxid_list = arr(out.taxid_list, out.n_taxid_list, np.int32)
    finally:
        L.mtb_free_built(ctypes.byref(out))
    return hdb


def subset_genomes(gen, idx):
    """The genomes ``idx`` (indices into ``gen``) with their gene blocks, as a Genomes of their own."""
    idx = np.asarray(idx, np.int64)
    off = np.asarray(gen.off, np.uint64)
    new_off = np.zeros(len(idx) + 1, np.uint64)
    new_off[1:] = np.cumsum(off[idx + 1] - off[idx])
    seq = (np.concatenate([gen.seq[int(off[g]):int(off[g + 1])] for g in idx]) if len(idx)
           else np.zeros(0, np.uint8))
    new_of = np.full(len(off) - 1, -1, np.int64)
    new_of[idx] = np.arange(len(idx))
    blk = new_of[np.asarray(gen.blk_genome, np.int64)]
    keep = blk >= 0
    order = np.argsort(blk[keep], kind="stable")

    def pick(a):
        return np.ascontiguousarray(np.asarray(a)[keep][order], np.int32)
    return type(gen)(np.ascontiguousarray(seq, np.uint8), new_off, np.ascontiguousarray(gen.taxid[idx], np.int32),
                     np.ascontiguousarray(gen.species[idx], np.int32), blk[keep][order].astype(np.int32),
                     pick(gen.blk_start), pick(gen.blk_end), pick(gen.blk_strand))


def build_db(gen, taxo, par: MtbParams, device: int = 0, split_num: int = 4096, device_seq=None,
             parts: int = 1) -> HostDb:
    """Build the reference DB on the GPU. ``device_seq`` = (seq, off) torch tensors already in HBM
    (bench path); otherwise ``gen.seq`` / ``gen.off`` are uploaded. ``parts`` = k > 1: the genomes
    are built in k groups (genome g in group g % k) and the k DBs merged, the reference's build of
    several flushes (numOfFlush > 1): diffIdx and info equal the single build's, the split table
    follows the merge's rule (see ``merge_dbs``)."""
    if parts > 1:
        if device_seq is not None:
            raise ValueError("parts > 1 builds from host genomes")
        groups = [np.arange(len(gen.taxid))[k::parts] for k in range(parts)]
        dbs = [build_db(subset_genomes(gen, g), taxo, par, device, split_num) for g in groups if len(g)]
        return merge_dbs(dbs, taxo, par, device, split_num)
    hdb = HostDb(taxo)
    inp, keep = _build_input(gen, device_seq, split_num, 0)
    out = MtbDbBuilt()
    L = _lib_build()
    tax_struct = hdb.c_struct()
    check(L.mtb_build_db(ctypes.byref(inp), ctypes.byref(tax_struct), ctypes.byref(par), device, ctypes.byref(out)),
          "mtb_build_db")
    return _take_built(hdb, out, L)


def merge_dbs(dbs, taxo, par: MtbParams, device: int = 0, split_num: int = 4096) -> HostDb:
    """Merge reference DBs on the GPU (mtb_merge_db): the k-mers of ``dbs`` (HostDb, 1 to 64 of them)
    in (value, species, taxID) order, one entry per (value, species) with the LCA of its taxIDs; the
    taxID list is the sorted union of theirs. diffIdx and info equal those of one build over all
    the genomes; the split table is sized by the k-mer count before merging
    (IndexCreator.h:343), unlike a single build's (IndexCreator.cpp:819)."""
    hdb = HostDb(taxo)
    L = _lib_build()
    ins = (MtbMergeInput * max(1, len(dbs)))()
    keep = []
    for i, d in enumerate(dbs):
        di, inf = np.ascontiguousarray(d.diff_idx, np.uint16), np.ascontiguousarray(d.info, np.uint32)
        keep += [di, inf]
        ins[i].diff_idx, ins[i].n_diff_idx = di.ctypes.data, len(di)
        ins[i].info, ins[i].n_info = inf.ctypes.data, len(inf)
    ids = [np.asarray(d.taxid_list, np.int32) for d in dbs if d.taxid_list is not None]
    union = np.unique(np.concatenate(ids)).astype(np.int32) if ids else np.zeros(0, np.int32)
    out = MtbDbBuilt()
    tax_struct = hdb.c_struct()
    check(L.mtb_merge_db(ins, len(dbs), union.ctypes.data, len(union), ctypes.byref(tax_struct), ctypes.byref(par),
                         split_num, device, ctypes.byref(out)), "mtb_merge_db")
    return _take_built(hdb, out, L)


def merge_db_dirs(dirs, out_dir: str, device: int = 0, split_num: int = 4096) -> None:
    """Merge DB directories into ``out_dir`` (mtb_merge_db_dirs): their db.parameters must agree in
    Kmer_format, Syncmer, Reduced_alphabet and Accession_level; taxonomy and db.parameters come
    from ``dirs[0]``."""
    arr = (ctypes.c_char_p * len(dirs))(*[os.fsencode(d) for d in dirs])
    check(lib().mtb_merge_db_dirs(arr, len(dirs), os.fsencode(out_dir), split_num, device), "mtb_merge_db_dirs")


def load_db_dir(directory: str, taxo) -> HostDb:
    """diffIdx / info / split / taxID_list of a DB directory as a HostDb over ``taxo``."""
    def rd(name, dt):
        return np.fromfile(os.path.join(directory, name), dtype=dt)
    ids = np.loadtxt(os.path.join(directory, "taxID_list"), dtype=np.int32, ndmin=1)
    return HostDb(taxo, rd("diffIdx", np.uint16), rd("info", np.uint32), rd("split", np.uint64), ids)


def update_db(old_dir: str, gen, taxo, par: MtbParams, out_dir: str, device: int = 0, split_num: int = 4096) -> HostDb:
    """Add the genomes ``gen`` to the DB in ``old_dir`` and write the result to ``out_dir``: the
    reference's updateDB (updateDB.cpp:134-142) without --new-taxa: the new genomes' DB is built,
    then merged with the old diffIdx / info over the union of the taxID lists. ``taxo`` holds the
    old DB's taxa and the new genomes'."""
    new = build_db(gen, taxo, par, device, split_num)
    merged = merge_dbs([load_db_dir(old_dir, taxo), new], taxo, par, device, split_num)
    merged.write(out_dir, par)
    return merged


def build_common_kmer_db(gen, taxo, out_dir: Optional[str], syncmer: int = 1, smer_len: int = 5, device: int = 0,
                         split_num: int = 4096, device_seq=None) -> HostDb:
    """Build the common-k-mer DB of read grouping on the GPU (mtb_build_common_db, csrc/mtb_common.hip;
    the reference's create_common_kmer_list): the AA 12-mers (``syncmer=1``: the syncmers of ``smer_len``)
    of all six frames of every genome of ``gen`` that genomes of two or more species hold, with the LCA
    of those species as info. ``gen.seq`` / ``gen.off`` / ``gen.taxid`` are read (whole genomes, no gene
    blocks); ``device_seq`` = (seq, off) torch tensors already in HBM. Writes diffIdx, info, split,
    taxID_list, db.parameters (Kmer_format 3, or 5 with syncmers) and kmer_params to ``out_dir`` (None:
    nothing is written) with the taxonomy as ``HostDb.write`` writes it (``taxo.write_dmp``: every taxonomy
    this package holds is one in memory; there is no loader from a DB directory whose files could be
    copied). ``grouping.group_reads(..., common_db=out_dir)`` takes the directory."""
    hdb = HostDb(taxo)
    inp = MtbBuildInput()
    if device_seq is not None:
        inp.seq, inp.off = device_seq[0].data_ptr(), device_seq[1].data_ptr()
        inp.flags = MTB_INPUT_DEVICE
    else:
        seq, off = np.ascontiguousarray(gen.seq, np.uint8), np.ascontiguousarray(gen.off, np.uint64)
        inp.seq, inp.off = seq.ctypes.data, off.ctypes.data
        inp.flags = 0
    taxid = np.ascontiguousarray(gen.taxid, np.int32)
    inp.n_genomes = len(taxid)
    inp.genome_taxid = taxid.ctypes.data
    inp.n_blocks = 0
    inp.split_num = split_num
    out = MtbDbBuilt()
    L = _lib_build()
    tax_struct = hdb.c_struct()
    check(L.mtb_build_common_db(ctypes.byref(inp), ctypes.byref(tax_struct), int(syncmer), int(smer_len), device,
                                ctypes.byref(out)), "mtb_build_common_db")
    _take_built(hdb, out, L)
    if out_dir is not None:
        par = MtbParams()
        lib().mtb_default_params(ctypes.byref(par))
        par.syncmer, par.smer_len, par.kmer_format = int(syncmer), int(smer_len), 5 if syncmer else 3
        hdb.write(out_dir, par)
        with open(os.path.join(out_dir, "kmer_params"), "w") as f:  # create_common_kmer_list.cpp:98-107
            f.write(f"syncmer {int(syncmer)}\nsmer_len {int(smer_len)}\nkmer_format {5 if syncmer else 3}\n")
    return hdb


def common_last_ms():
    """Phase times of this process's last common-k-mer build in ms: extraction, sort, reduce, fold,
    encode + split, total."""
    ms = (ctypes.c_float * 6)()
    check(lib().mtb_common_last_ms(ms, 6), "mtb_common_last_ms")
    return [float(x) for x in ms]


def merge_last_ms():
    """Phase times of this process's last merge in ms: upload + decode, merge passes, dedupe + LCA,
    encode + split, total."""
    ms = (ctypes.c_float * 5)()
    check(lib().mtb_merge_last_ms(ms, 5), "mtb_merge_last_ms")
    return [float(x) for x in ms]


_HIP = None


def _hip():
    global _HIP
    if _HIP is None:
        _HIP = ctypes.CDLL("libamdhip64.so.7")  # the runtime torch (and libmtbgpu) already use
        _HIP.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    return _HIP


def build_db_device(gen, taxo, par: MtbParams, device: int = 0, device_seq=None):
    """Build the reference DB on the GPU and keep it there (MTB_BUILD_DEVICE_OUT): returns torch
    tensors (values in resident rank form int64, taxIDs int32), deduplicated and sorted."""
    import torch

    inp, keep = _build_input(gen, device_seq, 4096, MTB_BUILD_DEVICE_OUT)
    out = MtbDbBuilt()
    L = _lib_build()
    htax = HostDb(taxo)  # keeps the arrays the struct points into alive
    tax_struct = htax.c_struct()
    check(L.mtb_build_db(ctypes.byref(inp), ctypes.byref(tax_struct), ctypes.byref(par), device, ctypes.byref(out)),
          "mtb_build_db")
    try:
        n = int(out.n_info)
        dev = torch.device("cuda", device)
        v = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        t = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        if n:
            H = _hip()
            if H.hipMemcpy(v.data_ptr(), out.dev_values, 8 * n, 3) or H.hipMemcpy(t.data_ptr(), out.dev_info, 4 * n, 3):
                raise RuntimeError("hipMemcpy of the built DB failed")
    finally:
        L.mtb_free_built(ctypes.byref(out))
    return v[:n], t[:n]
