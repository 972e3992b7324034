"""Regenerate tests/golden/ref_group_filter.npz: what the reference's OWN GroupGenerator::filterCommonKmers
keeps of the AA 12-mers its own scanners extract, for designed common-k-mer DBs.

Runs only where the reference tree is mounted; the committed .npz is what the tests read. Nothing of the
reference enters the repository: as in make_ref_match.py and make_ref_group_kmers.py the code is cut out
of the reference's files at run time into a throw-away C++ file in a temporary directory, compiled
(g++ -O1 -std=c++17 -fopenmp), run and deleted. The cut code (reference file):
* GroupGenerator.cpp `GroupGenerator::filterCommonKmers`, whole; GroupGenerator.h `COMMON_KMER_NEIGHBOR_SPAN`
* DeltaIdxReader.h `class KmerDbReader`; common.h `likely` / `unlikely`, `struct Buffer`, `struct ReadBuffer`;
  Mmap.h `MmapedData` / `mmapData`; KmerMatcher.h `struct QueryKmerSplit`
* Kmer.h `QueryKmerInfo`, `TargetKmerInfo`, `Kmer` (with compareQueryKmer and compareQKmerByIdAndPos),
  `DiffIdxSplit`
* the extraction of make_ref_group_kmers.py: `KmerScanner`, `KmerScanner_dna2aa`, `SyncmerScanner_dna2aa`,
  the `atcg` / `iRCT` tables, `getMaxCoveredLength`, `fillQueryKmerBuffer`
Stand-ins are declarations only: `LocalParameters{threads}`, a `GroupGenerator` with `par` and
`totalFilteredKmers`, the `KmerExtractor` declaration; `SORT_PARALLEL` is std::sort. The driver fills the
query buffer through fillQueryKmerBuffer (mate 2 under mate 1's seqID, after getMaxCoveredLength(len1) + 3),
sorts it with compareQueryKmer as extractQueryKmers does, and calls filterCommonKmers.

The DB files are written by tests/group_filter_cases.py (plain-Python diffIdx encoder, split table by
SURVEY Appendix B's rule) with 4 and with 4096 split entries; the cut code runs on each with 1, 3 and 16
threads, and all six outputs must agree (asserted; they did). Two traps of the reference are kept clear of
(asserted): a DB must hold more k-mers than split entries, or filterCommonKmers indexes the split table
out of range; and a run must hold at least as many query k-mers as threads.

Reads: those of ref_group_kmers.npz, plus 300-bp reads (frames of more than 32 windows), one 6-kb single
read, a pair of a 150-bp and a 75-bp mate, a read whose 12-mers have value 0 (found by trying every codon),
and two consecutive single reads whose last and first k-mer are hits. DBs per scanner configuration:
"fifth" (the smallest and the largest value, value 0, the two k-mers of one read at pos x and x + 2, the
last k-mer of one read and the first of the next, and random values up to a fifth of the instances), "all"
(every value) and "none"; each with group_filter_cases.FOREIGN values of no read and every 7th value twice.
"""
import pathlib
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
REF = pathlib.Path("/root/reference/src/commons")
REF_GROUP = pathlib.Path("/root/reference/src/read-group")
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))

import group_filter_cases as gc  # noqa: E402
from make_ref_functions import definitions  # noqa: E402
from make_ref_scanners import class_text  # noqa: E402

THREADS = (1, 3, 16)


def program() -> str:
    ks = (REF / "KmerScanner.h").read_text()
    ss = (REF / "SyncmerScanner.h").read_text()
    cc = (REF / "common.cpp").read_text()
    ch = (REF / "common.h").read_text()
    lu = (REF / "LocalUtil.h").read_text()
    ke = (REF / "KmerExtractor.cpp").read_text()
    km = (REF / "Kmer.h").read_text()
    kh = (REF / "KmerMatcher.h").read_text()
    mm = (REF / "Mmap.h").read_text()
    dr = (REF / "DeltaIdxReader.h").read_text()
    gh = (REF_GROUP / "GroupGenerator.h").read_text()
    gg = (REF_GROUP / "GroupGenerator.cpp").read_text()
    macros = [re.search(r"(?m)^#define %s.*$" % n, ch).group(0) for n in ("likely", "unlikely")]
    span = re.search(r"(?m)^.*\bCOMMON_KMER_NEIGHBOR_SPAN\s*=.*;$", gh).group(0)
    classes = [class_text(ks, "class KmerScanner {"), class_text(ks, "class KmerScanner_dna2aa : public KmerScanner {"),
               class_text(ss, "class SyncmerScanner_dna2aa : public KmerScanner_dna2aa {")]
    tables = [cc[m.start():cc.index(";", m.start()) + 1] for m in re.finditer(r"const std::string (atcg|iRCT) =", cc)]
    assert len(tables) == 2
    covered = definitions(lu, r"template\s*<typename T>\s*T LocalUtil::getMaxCoveredLength\(")
    fill = definitions(ke, r"void KmerExtractor::fillQueryKmerBuffer\(")
    filt = definitions(gg, r"void GroupGenerator::filterCommonKmers\(")
    assert len(covered) == 1 and len(fill) == 1 and len(filt) == 1
    mmap = "template <typename T>\n" + class_text(mm, "struct MmapedData") + "\n" + \
        definitions(mm, r"template <typename T>\s*MmapedData<T> mmapData\(")[0]
    return "\n".join([
        "#include <algorithm>", "#include <bitset>", "#include <cstdint>", "#include <cstdio>", "#include <cstdlib>",
        "#include <cstring>", "#include <ctime>", "#include <deque>", "#include <fcntl.h>", "#include <iostream>",
        "#include <omp.h>", "#include <string>", "#include <sys/mman.h>", "#include <sys/stat.h>", "#include <sys/types.h>",
        "#include <unistd.h>", "#include <utility>", "#include <vector>", '#include "GeneticCode.h"',
        "using namespace std;", "typedef int TaxID;", *macros, "#define SORT_PARALLEL std::sort", span,
        class_text(km, "struct QueryKmerInfo {"), class_text(km, "struct TargetKmerInfo {"),
        class_text(km, "struct Kmer {"), class_text(km, "struct DiffIdxSplit{"),
        "template<typename T>\n" + class_text(ch, "struct Buffer {"),
        "template<typename T>\n" + class_text(ch, "struct ReadBuffer {"), mmap,
        class_text(dr, "class KmerDbReader {"), class_text(kh, "struct QueryKmerSplit {"),
        *tables, *classes,
        "struct LocalUtil { template<typename T> static T getMaxCoveredLength(T queryLength); };", *covered,
        "struct KmerExtractor {",
        "  KmerScanner **kmerScanners;",
        "  void fillQueryKmerBuffer(const char *seq, int seqLen, Buffer<Kmer> &kmerBuffer, size_t &posToWrite,"
        " uint32_t seqID, uint32_t offset);",
        "};", *fill,
        "struct LocalParameters { int threads; };",
        "struct GroupGenerator {",
        "  LocalParameters par; size_t totalFilteredKmers = 0;",
        "  void filterCommonKmers(Buffer<Kmer> &qKmers, Buffer<std::pair<uint32_t, uint32_t>> &matchBuffer,"
        " const string &commonKmerDB);",
        "};", *filt, DRIVER])


# argv: syncmer smerLen threads dbDir ("-": extraction only) outFile; stdin: "<nReads>", then per read
# "<len1> <len2>" and the mates' bases on their own lines (len2 = 0: single-end).
# outFile, extraction only: per emitted k-mer "value seqID pos frame". With a DB: "H seqID pos" per entry of
# the sorted, de-duplicated matchBuffer, "K value seqID pos" per kept k-mer, "T totalFilteredKmers".
DRIVER = r"""
int main(int argc, char **argv) {
  if (argc != 6) return 2;
  int syncmer = atoi(argv[1]), smerLen = atoi(argv[2]), threads = atoi(argv[3]);
  std::string db = argv[4];
  long n;
  if (scanf("%ld", &n) != 1) return 1;
  GeneticCode gc(false);
  KmerScanner *sc = syncmer ? (KmerScanner *)new SyncmerScanner_dna2aa(gc, 12, smerLen)
                            : (KmerScanner *)new KmerScanner_dna2aa(gc, 12);
  KmerExtractor ex; ex.kmerScanners = &sc;
  Buffer<Kmer> q(1 << 21);
  static char s1[1 << 20], s2[1 << 20];
  size_t pos = 0;
  for (long i = 0; i < n; i++) {
    int l1, l2;
    if (scanf("%d %d", &l1, &l2) != 2) return 3;
    if (scanf("%s", s1) != 1) return 4;
    if (l2 && scanf("%s", s2) != 1) return 5;
    ex.fillQueryKmerBuffer(s1, l1, q, pos, (uint32_t)i + 1, 0);
    if (l2) ex.fillQueryKmerBuffer(s2, l2, q, pos, (uint32_t)i + 1, (uint32_t)LocalUtil::getMaxCoveredLength(l1) + 3);
    if (pos + (1 << 18) > q.bufferSize) return 6;
  }
  q.startIndexOfReserve = pos;
  FILE *out = fopen(argv[5], "w");
  if (!out) return 7;
  if (db == "-") {
    for (size_t k = 0; k < pos; k++)
      fprintf(out, "%llu %u %u %u\n", (unsigned long long)q.buffer[k].value, (unsigned)q.buffer[k].qInfo.sequenceID,
              (unsigned)q.buffer[k].qInfo.pos, (unsigned)q.buffer[k].qInfo.frame);
    fclose(out);
    return 0;
  }
  std::sort(q.buffer, q.buffer + pos, Kmer::compareQueryKmer);
  omp_set_num_threads(threads);
  GroupGenerator g; g.par.threads = threads;
  Buffer<std::pair<uint32_t, uint32_t>> m(pos * 8 + 4096);
  g.filterCommonKmers(q, m, db);
  std::pair<uint32_t, uint32_t> *e = std::unique(m.buffer, m.buffer + m.startIndexOfReserve);
  for (std::pair<uint32_t, uint32_t> *p = m.buffer; p != e; p++) fprintf(out, "H %u %u\n", p->first, p->second);
  for (size_t k = 0; k < q.startIndexOfReserve; k++)
    fprintf(out, "K %llu %u %u\n", (unsigned long long)q.buffer[k].value, (unsigned)q.buffer[k].qInfo.sequenceID,
            (unsigned)q.buffer[k].qInfo.pos);
  fprintf(out, "T %zu\n", g.totalFilteredKmers);
  fclose(out);
  return 0;
}
"""


def rand_dna(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes().decode()


def extra_reads(rng):
    """The reads added to ref_group_kmers.npz's, without the value-0 read."""
    rs = [(rand_dna(rng, 300), rand_dna(rng, 300)) for _ in range(3)]
    rs += [(rand_dna(rng, 301), ""), (rand_dna(rng, 302), "")]
    rs += [(rand_dna(rng, 6001), "")]
    rs += [(rand_dna(rng, 150), rand_dna(rng, 75))]
    return rs


def stdin_of(rs):
    inp = [str(len(rs))]
    for a, b in rs:
        inp.append(f"{len(a)} {len(b)}")
        inp.append(a)
        if b:
            inp.append(b)
    return "\n".join(inp) + "\n"


def run(exe, d, syn, smer, threads, db, rs):
    out = pathlib.Path(d) / "out.txt"
    subprocess.run([str(exe), str(syn), str(smer), str(threads), str(db), str(out)], input=stdin_of(rs), text=True,
                   check=True, stdout=subprocess.DEVNULL)
    return out.read_text().splitlines()


def extract(exe, d, syn, smer, rs):
    got = " ".join(run(exe, d, syn, smer, 1, "-", rs)).split()
    return np.array(got, dtype=np.uint64).reshape(-1, 4)


def canonical(x):
    """Instances in (seqID, frame, pos) order."""
    return x[np.lexsort((x[:, 0], x[:, 2], x[:, 3], x[:, 1]))]


def choose_db(rng, v, s, p):
    """The "fifth" DB's own values (a mask over the distinct values)."""
    distinct = np.unique(v)
    pick = {int(distinct[0]), int(distinct[-1])}
    if distinct[0] != 0:
        print("  no value 0 in this configuration")
    # two k-mers of one read at pos x and x + 2 with one between them
    key = s.astype(np.int64) * (1 << 33) + p.astype(np.int64)
    ks = set(key.tolist())
    for i in np.argsort(key):
        if int(key[i]) + 1 in ks and int(key[i]) + 2 in ks:
            pick.add(int(v[i]))
            pick.add(int(v[np.nonzero(key == key[i] + 2)[0][0]]))
            print(f"  x / x + 2 pair: read {s[i]} pos {p[i]}")
            break
    else:
        raise AssertionError("no instances at x, x + 1, x + 2")
    # the last k-mer of the last-but-one read and the first k-mer of the last read
    a, b = int(s.max()) - 1, int(s.max())
    ia = np.nonzero(s == a)[0]
    ib = np.nonzero(s == b)[0]
    pick.add(int(v[ia[np.argmax(p[ia])]]))
    pick.add(int(v[ib[np.argmin(p[ib])]]))
    own = np.isin(distinct, np.array(sorted(pick), np.uint64))
    order = rng.permutation(len(distinct))
    for j in order:  # random values until a fifth of the instances is hit
        if np.isin(v, distinct[own]).sum() * 5 >= len(v):
            break
        own[j] = True
    return own


def reference(exe, d, cfg, syn, smer, rs, dbv, ext):
    """filterCommonKmers on the DB values, over every split count and thread count: (keep mask over ext, hit
    position mask, kept count)."""
    assert len(ext) >= max(THREADS), "fewer query k-mers than threads"
    results = []
    for n_split in gc.SPLITS:
        assert len(dbv) > n_split, "a DB must hold more k-mers than split entries"
        db_dir = pathlib.Path(d) / f"db_{n_split}"
        gc.write_db(db_dir, dbv, n_split)
        usable = (np.fromfile(db_dir / "split", gc.SPLIT_DTYPE)["ADkmer"][1:] != 0).sum() + 1
        assert usable >= 2, "fewer than two usable split entries"
        for t in THREADS:
            results.append(sorted(run(exe, d, syn, smer, t, db_dir, rs)))
    assert all(r == results[0] for r in results), f"{cfg}: the outputs differ between thread or split counts"
    hits = np.array([ln.split()[1:] for ln in results[0] if ln[0] == "H"], dtype=np.uint64).reshape(-1, 2)
    kept = np.array([ln.split()[1:] for ln in results[0] if ln[0] == "K"], dtype=np.uint64).reshape(-1, 3)
    total = [int(ln.split()[1]) for ln in results[0] if ln[0] == "T"]
    assert total == [len(kept)]
    # the kept multiset as a mask over the instances: both sorted by (seqID, pos, value)
    v, s, p = ext[:, 0], ext[:, 1], ext[:, 2]
    key = np.stack([s, p, v], 1)
    order = np.lexsort((v, p, s))
    kk = kept[:, [1, 2, 0]]
    kk = kk[np.lexsort((kk[:, 2], kk[:, 1], kk[:, 0]))]
    keep = np.zeros(len(ext), bool)
    j = 0
    for i in order:  # kept is a sub-multiset of the instances
        if j < len(kk) and tuple(key[i]) == tuple(kk[j]):
            keep[i] = True
            j += 1
    assert j == len(kk), "a kept k-mer that was never extracted"
    sp = s.astype(np.int64) * (1 << 33) + p.astype(np.int64)
    hk = hits[:, 0].astype(np.int64) * (1 << 33) + hits[:, 1].astype(np.int64)
    at_hit = np.isin(sp, hk)
    assert len(np.unique(sp[at_hit])) == len(hk), "a hit at a position without an instance"
    return keep, at_hit, len(kept)


if __name__ == "__main__":
    rng = np.random.default_rng(20261021)
    base = np.load(HERE / "ref_group_kmers.npz")
    rs = list(zip(base["seq1"].tolist(), base["seq2"].tolist())) + extra_reads(rng)
    arrays = {}
    with tempfile.TemporaryDirectory() as d:
        src = pathlib.Path(d) / "ref_group_filter.cpp"
        exe = pathlib.Path(d) / "ref_group_filter"
        src.write_text(program())
        subprocess.run(["g++", "-O1", "-std=c++17", "-fopenmp", "-w", f"-I{REF}", str(src), "-o", str(exe)], check=True)
        # the read whose 12-mers are 0: 13 copies of the first codon that gives one
        zero = None
        for c in [a + b + c for a in "ACGT" for b in "ACGT" for c in "ACGT"]:
            x = extract(exe, d, 0, 5, [(c * 14, "")])
            if len(x) and (x[:, 0] == 0).any():
                zero = c * 14
                print("value 0 from codon", c)
                break
        assert zero is not None
        rs += [(zero, ""), (rand_dna(rng, 150), ""), (rand_dna(rng, 150), "")]
        arrays["seq1"] = np.array([a for a, _ in rs])
        arrays["seq2"] = np.array([b for _, b in rs])
        full = canonical(extract(exe, d, 0, 5, rs))
        arrays["fmt3_value"] = full[:, 0]
        arrays["fmt3_seq"] = full[:, 1].astype(np.uint32)
        arrays["fmt3_pos"] = full[:, 2].astype(np.uint32)
        arrays["fmt3_frame"] = full[:, 3].astype(np.uint8)
        full_rows = {tuple(r): i for i, r in enumerate(full.tolist())}
        assert len(full_rows) == len(full), "an instance emitted twice"
        for cfg, syn, smer in gc.CONFIGS:
            ext = full if cfg == "fmt3" else canonical(extract(exe, d, syn, smer, rs))
            if cfg != "fmt3":  # a subset of the plain scanner's windows
                mask = np.zeros(len(full), bool)
                mask[[full_rows[tuple(r)] for r in ext.tolist()]] = True
                assert mask.sum() == len(ext) and np.array_equal(full[mask], ext)
                arrays[f"{cfg}_mask"] = np.packbits(mask)
            v, s, p = ext[:, 0], ext[:, 1], ext[:, 2]
            distinct = np.unique(v)
            print(cfg, len(ext), "instances,", len(distinct), "distinct values")
            owns = {"fifth": choose_db(rng, v, s, p), "all": np.ones(len(distinct), bool),
                    "none": np.zeros(len(distinct), bool)}
            for db, own in owns.items():
                arrays[f"{cfg}_{db}_own"] = np.packbits(own)
                probe = {k: arrays[k] for k in arrays}
                dbv = gc.db_values(probe, cfg, db)
                keep, at_hit, kept = reference(exe, d, cfg, syn, smer, rs, dbv, ext)
                arrays[f"{cfg}_{db}_keep"] = np.packbits(keep)
                arrays[f"{cfg}_{db}_hitpos"] = np.packbits(at_hit)
                arrays[f"{cfg}_{db}_kept"] = np.int64(kept)
                print(f"  {db}: {len(dbv)} DB k-mers, {int(np.isin(v, dbv).sum())} hit instances, {kept} kept")
    np.savez_compressed(HERE / "ref_group_filter.npz", **arrays)
    print("wrote", HERE / "ref_group_filter.npz", (HERE / "ref_group_filter.npz").stat().st_size, "bytes")
