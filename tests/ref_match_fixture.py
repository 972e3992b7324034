"""What tests/golden/ref_match.npz holds (shared by tests/test_ref_match.py and the fixture's generator,
tests/golden/make_ref_match.py): loading it, writing one of its DBs to a directory, and the count of
the shapes it covers, recomputed in plain numpy from its stored inputs and outputs."""
import os
import pathlib

import numpy as np

from metabuli_work_amd._abi import KMER_DTYPE, MATCH_DTYPE, info_frame, info_seq

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"
RUN_LENGTHS = (1, 2, 3, 47, 48, 49, 63, 64, 65, 128)  # and at least one above 256
FLAG = np.uint32(1 << 31)
_golden = None


def golden():
    global _golden
    if _golden is None:
        _golden = dict(np.load(GOLDEN / "ref_match.npz"))
    return _golden


def matches_of(g, db):
    m = np.zeros(len(g[f"{db}_m_ham"]), MATCH_DTYPE)
    m["qinfo"] = g[f"{db}_m_qinfo"]
    m["target_id"] = g[f"{db}_m_target"]
    m["species_id"] = g[f"{db}_m_species"]
    m["dna_encoding"] = g[f"{db}_m_dna"]
    m["right_end_hamming"] = g[f"{db}_m_reh"]
    m["hamming"] = g[f"{db}_m_ham"]
    return m


def query_of(g, db):
    return np.ascontiguousarray(g[f"{db}_query"]).view(KMER_DTYPE).reshape(-1)


def taxonomy(g):
    from metabuli_work_amd import synth
    n_species, strains, seed = (int(x) for x in g["tax_params"])
    return synth.make_taxonomy(n_species, strains, seed=seed)


def info_words(g, db, split_num, skip_redundancy):
    """The info file of a run: bit 31 set on a share of the words with skipRedundancy 0 (the matcher masks
    it off); clean words with skipRedundancy 1 (nothing is masked: a set bit would be part of the taxID)."""
    info = g[f"{db}_info"]
    return info if skip_redundancy == 0 else info & ~FLAG


def write_db(g, db, split_num, skip_redundancy, out_dir):
    """diffIdx / info / split from the fixture, the taxonomy through write_dmp, db.parameters and taxID_list
    as the oracle's builder writes them (oracle/orc_dbwriter.cpp), Skip_redundancy as asked."""
    os.makedirs(out_dir, exist_ok=True)
    g[f"{db}_diffIdx"].tofile(os.path.join(out_dir, "diffIdx"))
    info_words(g, db, split_num, skip_redundancy).tofile(os.path.join(out_dir, "info"))
    g[f"{db}_s{split_num}_split"].tofile(os.path.join(out_dir, "split"))
    taxo = taxonomy(g)
    taxo.write_dmp(os.path.join(out_dir, "taxonomy"))
    fmt, syn, smer = (int(x) for x in g[f"{db}_fmt"])
    genome_ids = sorted(int(t) for t, r in zip(taxo.taxid.tolist(), taxo.rank) if r == "no rank" and t != 1)
    with open(os.path.join(out_dir, "taxID_list"), "w") as f:
        f.write("".join(f"{t}\n" for t in genome_ids))
    with open(os.path.join(out_dir, "db.parameters"), "w") as f:
        f.write("DB_name\tsynthetic\nCreation_date\t1970-01-01\nMetabuli commit used to create the DB\toracle\n"
                "Reduced_alphabet\t0\nAccession_level\t0\nMask_mode\t0\nMask_prob\t0.900000\n"
                f"Skip_redundancy\t{skip_redundancy}\nSyncmer\t{syn}\n")
        if syn:
            f.write(f"Syncmer_len\t{smer}\n")
        f.write(f"Kmer_format\t{fmt}\n")
    return out_dir


def reads_of(g, db, kind):
    """synth.Reads of the fixture: "short" (the single-end reads of 60-150 bp: a uniform batch), "long"
    (the same with the >= 400-bp read after them: a non-uniform batch) or "paired". Returns the reads and
    the sequenceID of the first of them in the fixture's numbering (1-based)."""
    from metabuli_work_amd import synth
    s1, s2 = g[f"{db}_seq1"].tolist(), g[f"{db}_seq2"].tolist()
    ns, npair = int(g[f"{db}_n_single"]), int(g[f"{db}_n_pair"])
    lo, hi = {"short": (0, ns), "long": (0, ns + 1), "paired": (ns + 1, ns + 1 + npair)}[kind]

    def pack(strs):
        off = np.zeros(len(strs) + 1, np.uint64)
        off[1:] = np.cumsum([len(s) for s in strs])
        return np.frombuffer("".join(strs).encode(), np.uint8).copy(), off
    a, oa = pack(s1[lo:hi])
    b, ob = pack(s2[lo:hi]) if kind == "paired" else (None, None)
    return synth.Reads(a, oa, b, ob, np.full(hi - lo, -1, np.int32)), lo + 1


def subset(g, db, first_seq, n_reads):
    """The fixture's matches and query k-mer number of reads first_seq .. first_seq + n_reads - 1, renumbered
    from 1 (matches are per query, so the subset is exact; the canonical order sorts on sequenceID first)."""
    m, q = matches_of(g, db), query_of(g, db)
    s = info_seq(m["qinfo"]).astype(np.int64)
    m = m[(s >= first_seq) & (s < first_seq + n_reads)].copy()
    m["qinfo"] -= np.uint64(first_seq - 1) << np.uint64(32)
    qs = info_seq(q["info"]).astype(np.int64)
    return m, int(((qs >= first_seq) & (qs < first_seq + n_reads)).sum())


def decode(diff):
    """diffIdx words to k-mer values (15-bit groups, most significant first, bit 15 ends a delta)."""
    diff = diff.astype(np.uint64)
    term = np.nonzero(diff & np.uint64(0x8000))[0]
    starts = np.concatenate([[0], term[:-1] + 1])
    kidx = np.repeat(np.arange(len(term)), term - starts + 1)
    shift = (term[kidx] - np.arange(len(diff))) * 15
    return np.cumsum(np.add.reduceat((diff & np.uint64(0x7FFF)) << shift.astype(np.uint64), starts), dtype=np.uint64)


def runs_of(values):
    """Per record: the index of its AA run; per run: its start and length."""
    aa = values >> np.uint64(24)
    first = np.ones(len(aa), bool)
    first[1:] = aa[1:] != aa[:-1]
    start = np.nonzero(first)[0]
    return np.cumsum(first) - 1, start, np.diff(np.append(start, len(aa))), aa[start]


def kmer_list(g, db):
    """The DB's sorted unique (value, taxID) list: diffIdx decoded, info without bit 31."""
    return decode(g[f"{db}_diffIdx"]), g[f"{db}_info"] & ~FLAG


def long_run_queries(g, db, first_seq, n_reads, long_run=48):
    """Queries of reads first_seq .. first_seq + n_reads - 1 whose AA run, without the DB's last k-mer, holds
    more than long_run candidates (kLongRun in mtb_kernels.hip: they go to k_match_long)."""
    values, _ = kmer_list(g, db)
    _, _, length, run_aa = runs_of(values)
    length = length.copy()
    length[-1] -= 1
    q = query_of(g, db)
    qs = info_seq(q["info"]).astype(np.int64)
    q_aa = (q["value"] >> np.uint64(24))[(qs >= first_seq) & (qs < first_seq + n_reads)]
    r = np.minimum(np.searchsorted(run_aa, q_aa), len(run_aa) - 1)
    return int(((run_aa[r] == q_aa) & (length[r] > long_run)).sum())


def record_of_match(g, db, m, q_aa_of):
    """The DB record every match names: value = the query's AA part with the match's DNA part, species = the
    match's (a (value, species) pair is one record)."""
    values, ids = kmer_list(g, db)
    sp = dict(g[f"{db}_species_table"].tolist())
    rec_sp = np.array([sp[int(t)] for t in ids], np.uint64)
    key = {(int(v), int(s)): i for i, (v, s) in enumerate(zip(values, rec_sp))}
    return np.array([key[(int(a) << 24 | int(d), int(s))] for a, d, s in
                     zip(q_aa_of, m["dna_encoding"], m["species_id"])], np.int64)


def coverage_table(g):
    c = {}

    def add(k, v=1):
        c[k] = c.get(k, 0) + int(v)
    for db in g["dbs"].tolist():
        values, _ = kmer_list(g, db)
        rec_run, start, length, run_aa = runs_of(values)
        q = query_of(g, db)
        q_aa = q["value"] >> np.uint64(24)
        r = np.searchsorted(run_aa, q_aa)
        present = (r < len(run_aa)) & (run_aa[np.minimum(r, len(run_aa) - 1)] == q_aa)
        qlen = np.where(present, length[np.minimum(r, len(run_aa) - 1)], 0)
        for n in RUN_LENGTHS:
            add(f"{db}: queries of a run of {n}", (qlen == n).sum())
        add(f"{db}: queries of a run above 256", (qlen > 256).sum())
        add(f"{db}: queries of the DB's first run", (present & (r == 0)).sum())
        add(f"{db}: queries with the last k-mer's AA", (q_aa == run_aa[-1]).sum())
        add(f"{db}: length of the DB's first run", length[0])
        add(f"{db}: length of the DB's last run", length[-1])
        add(f"{db}: queries above every DB k-mer", (q_aa > run_aa[-1]).sum())
        add(f"{db}: queries below every DB k-mer", (q_aa < run_aa[0]).sum())
        add(f"{db}: queries between two present AA 8-mers", (~present & (q_aa > run_aa[0]) & (q_aa < run_aa[-1])).sum())
        same_v = present[1:] & (q["value"][1:] == q["value"][:-1])
        f3 = info_frame(q["info"]) // np.uint64(3)
        add(f"{db}: identical queries, equal frame/3", (same_v & (f3[1:] == f3[:-1])).sum())
        add(f"{db}: identical queries, unequal frame/3", (same_v & (f3[1:] != f3[:-1])).sum())
        add(f"{db}: AA-equal, DNA-different neighbours", (present[1:] & (q_aa[1:] == q_aa[:-1]) &
                                                           (q["value"][1:] != q["value"][:-1])).sum())
        add(f"{db}: equal consecutive DB values", (values[1:] == values[:-1]).sum())
        m = matches_of(g, db)
        qmap = dict(zip(q["info"].tolist(), q_aa.tolist()))
        rec = record_of_match(g, db, m, [qmap[int(i)] for i in m["qinfo"]])
        c[f"{db}: matches naming the DB's last k-mer"] = int((rec == len(values) - 1).sum())
        add(f"{db}: matched records with bit 31 set", ((g[f"{db}_info"][rec] & FLAG) != 0).sum())
        for sn in g["splits"].tolist():
            size = len(values) // (sn - 1)
            offs = np.arange(1, sn) * size
            offs = offs[(offs > 0) & (offs < len(values))]
            add(f"{db}: split {sn}: offsets inside an AA run", (rec_run[offs - 1] == rec_run[offs]).sum())
            sp = g[f"{db}_s{sn}_split"].reshape(-1, 3)
            add(f"{db}: split {sn}: filtered entries", (sp[1:, 0] == 0).sum())
        nonuni = info_seq(m["qinfo"]) == int(g[f"{db}_n_single"]) + 1
        add(f"{db}: matches of the long read", nonuni.sum())
        add(f"{db}: matches of the paired reads", (info_seq(m["qinfo"]) > int(g[f"{db}_n_single"]) + 1).sum())
        add(f"{db}: matches with a non-zero hamming", (m["hamming"] > 0).sum())
    return c
