"""Regenerate tests/golden/ref_match.npz: the matches the reference's OWN KmerMatcher::matchKmers returns
for designed DBs and reads. Until now the merge loop was restatement-only on both sides
(oracle/orc_match.cpp and the K3 / K4 kernels), so every GPU join test compared two readings of it.

Fixture-time only, never imported by a test. As in make_ref_assign.py the code is cut out of
/root/reference/src/commons at run time into a throw-away C++ file in a temporary directory next to
stand-in declarations, compiled with BitManipulateMacros.h and GeneticCode.h in place (g++ -O1
-std=c++17 -fopenmp), run and deleted; nothing of the cut text is committed. The same program is also
built with -fsanitize=address,undefined (a stand-alone program with its own main, no LD_PRELOAD) and run
on every case with 1 and 16 threads; it must exit clean with the same output, and did.

The cut code (reference file:line):
* KmerMatcher.cpp:123-481 `KmerMatcher::matchKmers`, whole; :30-32 the constructor's DNA_MASK / AA_MASK
  values; :1080-1083 moveMatches; :1117-1146 compareDna
* KmerMatcher.h:20 `BufferSize`, :22 `AMINO_ACID_PART`, :33-47 `struct QueryKmerSplit`, :66-158 the
  Hamming tables, :266-276 getKmerInfo, :282-297 getNextTargetKmer (index form), :348-360
  getHammingDistanceSum, :386-416 getHammings / getHammings_reverse
* Kmer.h:11-16 `struct QueryKmerInfo`, :18-22 `struct TargetKmerInfo`, :24-109 `struct Kmer` (with
  compareQueryKmer, :89-94, which sorts the query buffer as KmerExtractor.cpp:79 does), :111-119
  `struct DiffIdxSplit`
* Match.h:9-87 `struct Match`; common.h:18-19 likely / unlikely, :147-221 `struct Buffer` (with
  reserveMemory), :348-359 the two loadBuffer templates; Mmap.h:14-58 `MmapedData` / `mmapData`
* through make_ref_scanners.program() and make_ref_writer.program() (imported, not copied): the
  scanners, fillQueryKmerBuffer, getMaxCoveredLength, and writeTargetFilesAndSplits / getDiffIdx

Stand-ins (declarations only): `LocalParameters` (skipRedundancy), an empty `SeqIterator(par)`, a
`TaxonNode` / `TaxonomyWrapper` whose members the unreachable exit(1) diagnostic names, aborting if
called, the `KmerMatcher` class declaration (the members matchKmers reads, the cut tables and
getKmerInfo inside it), `FileUtil::getFileSize` as a stat call (an MMseqs2 service, parity unpinned),
and `taxId2speciesId`, filled from a table the generator passes in (its loader, KmerMatcher.cpp:90-118,
is MMseqs2 taxonomy and stays unpinned). The reserved-but-unfilled slots of the query buffer (blanks,
KmerMatcher.cpp:143-151) are not modelled: the buffer holds the emitted k-mers only, so blankCnt is 0.

Where the inputs come from: "genome" strings (a 24-nt family member between two random 6-nt flanks) go
through the cut scanners (frame 0 of fillQueryKmerBuffer's output) to give target k-mer values; taxIDs
come from synth.make_taxonomy; the list is sorted and reduced to one entry per (value, species) (the
species' ID where several strains share a value, as the LCA gives), and the cut writer writes diffIdx /
info / split. The reads go through the cut scanners and fillQueryKmerBuffer; std::sort with the cut
compareQueryKmer orders the buffer; matchKmers gives the matches.

Thread independence: every case ran with 1, 2, 7 and 16 threads and with split counts 4 and 4096; the
match multiset was the same in all of them (asserted below; it held on every case). That is the
property that lets a GPU join, which has no thread ranges, stand in for the loop.

Dropped: the two tiny DBs (1 and 2 k-mers of one AA 8-mer with a query equal to them). A DB of fewer
k-mers than splitNum - 1 gets no split entry at all (sizeOfSplit is 0, IndexCreator.cpp:811-865), so
numOfDiffIdxSplits_use is 1 and every thread range whose first query lies above AA part 0 takes
`diffIdxSplits.data[numOfDiffIdxSplits_use - 2]` = `data[-1]` (KmerMatcher.cpp:191): outside defined
behaviour under every thread count above 1, and under 1 thread unless the read's smallest k-mer has AA
part 0. A first syncmer DB of 3k k-mers with 4096 splits crashed at that line; the syncmer DB now holds
14k. The oracle refuses such a DB ("fewer than one split").

Kept small on purpose (no committed file passes 1 MiB): 4.7k k-mers per main DB, about 140 reads.
"""
import pathlib
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
ROOT = HERE.parents[1]
REF = pathlib.Path("/root/reference/src/commons")
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(HERE))

import make_ref_scanners  # noqa: E402
import make_ref_writer  # noqa: E402
from make_ref_functions import definitions  # noqa: E402
from make_ref_scanners import class_text  # noqa: E402

THREADS = (1, 2, 7, 16)
SPLITS = (4, 4096)
RUNS = (1, 2, 3, 47, 48, 49, 63, 64, 65, 128, 300)
FLAG_SHARE = 0.3


# ---------------------------------------------------------------------------------------------------
# the program
def program() -> str:
    kh = (REF / "KmerMatcher.h").read_text()
    kc = (REF / "KmerMatcher.cpp").read_text()
    km = (REF / "Kmer.h").read_text()
    mh = (REF / "Match.h").read_text()
    ch = (REF / "common.h").read_text()
    mm = (REF / "Mmap.h").read_text()
    macros = [re.search(r"(?m)^#define %s.*$" % n, t).group(0)
              for n, t in (("likely", ch), ("unlikely", ch), ("BufferSize", kh), ("AMINO_ACID_PART", kh))]
    ctor = definitions(kc, r"KmerMatcher::KmerMatcher\(\s*const LocalParameters & par,\s*TaxonomyWrapper")
    assert len(ctor) == 1
    masks = re.findall(r"(?m)^\s*(?:DNA_MASK|AA_MASK) = [^;]*;", ctor[0])
    assert len(masks) == 3, masks
    tables = kh[kh.index("uint8_t hammingLookup[8][8]"):]
    tables = tables[:tables.index("};", tables.index("HAMMING_LUT7[64]")) + 2]
    get_info = kh[kh.index("template <typename T>\n  static inline T getKmerInfo("):]
    get_info = get_info[:get_info.index("return infoBuffer[infoBufferIdx];")] + "return infoBuffer[infoBufferIdx];\n  }"
    next_idx = [d for d in definitions(kh, r"inline uint64_t KmerMatcher::getNextTargetKmer\(")
                if "diffBufferIdx" in d and "totalPos" in d]
    km_defs = (next_idx +
               definitions(kh, r"(?m)^inline uint8_t KmerMatcher::getHammingDistanceSum\(") +
               definitions(kh, r"(?m)^inline uint16_t KmerMatcher::getHammings\(") +
               definitions(kh, r"(?m)^inline uint16_t KmerMatcher::getHammings_reverse\(") +
               definitions(kc, r"void KmerMatcher::moveMatches\(") +
               definitions(kc, r"void KmerMatcher::compareDna\(") +
               definitions(kc, r"bool KmerMatcher::matchKmers\("))
    assert len(km_defs) == 7, len(km_defs)
    load = definitions(ch, r"template <typename T>\s*size_t loadBuffer\(")
    assert len(load) == 2, len(load)
    mmap = "template <typename T>\n" + class_text(mm, "struct MmapedData") + "\n" + \
        definitions(mm, r"template <typename T>\s*MmapedData<T> mmapData\(")[0]
    return "\n".join([
        "#include <algorithm>", "#include <bitset>", "#include <cstdint>", "#include <cstdio>", "#include <cstdlib>",
        "#include <cstring>", "#include <ctime>", "#include <fcntl.h>", "#include <fstream>", "#include <iostream>",
        "#include <string>", "#include <sys/mman.h>", "#include <sys/stat.h>", "#include <sys/types.h>",
        "#include <unistd.h>", "#include <unordered_map>", "#include <vector>", '#include "BitManipulateMacros.h"',
        '#include "GeneticCode.h"', "using namespace std;", "typedef int TaxID;", *macros,
        class_text(km, "struct QueryKmerInfo {"), class_text(km, "struct TargetKmerInfo {"),
        class_text(km, "struct Kmer {"), class_text(km, "struct DiffIdxSplit{"), class_text(mh, "struct Match {"),
        "template<typename T>\n" + class_text(ch, "struct Buffer {"), *load, mmap,
        class_text(kh, "struct QueryKmerSplit {"), STANDINS,
        "class KmerMatcher {", "public:",
        "  const LocalParameters &par; TaxonomyWrapper *taxonomy = nullptr; int kmerFormat; size_t threads;",
        "  std::string dbDir; uint64_t DNA_MASK; uint64_t AA_MASK; size_t totalMatchCnt = 0;",
        tables,
        "  unordered_map<TaxID, TaxID> taxId2speciesId;",
        "  string targetDiffIdxFileName; string targetInfoFileName; string diffIdxSplitFileName;",
        "  KmerMatcher(const LocalParameters &par, TaxonomyWrapper *taxonomy, int kmerFormat)"
        " : par(par), taxonomy(taxonomy), kmerFormat(kmerFormat) {", *masks, "  }",
        "  void moveMatches(Match *dest, Match *src, size_t & matchNum);",
        "  void compareDna(uint64_t query, std::vector<uint64_t> &targetKmersToCompare, std::vector<uint8_t> &hammingDists,"
        " std::vector<size_t> &selectedMatches, std::vector<uint8_t> &selectedHammingSum,"
        " std::vector<uint16_t> &rightEndHammings, size_t &selectedMatchIdx, uint8_t frame);",
        "  uint8_t getHammingDistanceSum(uint64_t kmer1, uint64_t kmer2);",
        "  uint16_t getHammings(uint64_t kmer1, uint64_t kmer2);",
        "  uint16_t getHammings_reverse(uint64_t kmer1, uint64_t kmer2);",
        "  bool matchKmers(Buffer<Kmer> *queryKmerBuffer, Buffer<Match> *matchBuffer, const string &db = string());",
        "  static uint64_t getNextTargetKmer(uint64_t lookingTarget, const uint16_t *diffIdxBuffer,"
        " size_t &diffBufferIdx, size_t &totalPos);",
        get_info, "};", *km_defs, DRIVER])


STANDINS = r"""
struct LocalParameters { int skipRedundancy = 0; };
struct SeqIterator { explicit SeqIterator(const LocalParameters &) {} };
struct TaxonNode { TaxID taxId; size_t nameIdx; size_t rankIdx; };
struct TaxonomyWrapper {
  const TaxonNode *taxonNode(TaxID) const { abort(); }
  TaxID getOriginalTaxID(TaxID) const { abort(); }
  const char *getString(size_t) const { abort(); }
};
struct FileUtil {
  static size_t getFileSize(const std::string &fileName) {
    struct stat sb;
    if (stat(fileName.c_str(), &sb) != 0) abort();
    return (size_t)sb.st_size;
  }
};
"""

# argv: dbDir kmerFormat skipRedundancy threads queryFile speciesFile sortedOut matchOut.
# queryFile: 16-byte records (value, qInfo word) in emission order; speciesFile: lines "taxID speciesID".
# sortedOut: the buffer after std::sort(compareQueryKmer), same records; matchOut: one line per match
# "seq frame pos target species dna reh ham", then stdout keeps matchKmers' own "Query k-mer number" line.
DRIVER = r"""
int main(int argc, char **argv) {
  if (argc != 9) return 2;
  LocalParameters par; par.skipRedundancy = atoi(argv[3]);
  TaxonomyWrapper tax;
  KmerMatcher km(par, &tax, atoi(argv[2]));
  km.dbDir = argv[1];
  km.threads = (size_t)atoi(argv[4]);
  { std::ifstream in(argv[6]); TaxID t, s; while (in >> t >> s) km.taxId2speciesId[t] = s; }
  FILE *qf = fopen(argv[5], "rb");
  if (!qf) return 3;
  fseek(qf, 0, SEEK_END); size_t n = (size_t)ftell(qf) / 16; fseek(qf, 0, SEEK_SET);
  Buffer<Kmer> q(n + 1);
  static_assert(sizeof(Kmer) == 16, "Kmer is 16 bytes");
  if (fread(q.buffer, 16, n, qf) != n) return 4;
  fclose(qf);
  q.startIndexOfReserve = n;
  std::sort(q.buffer, q.buffer + n, Kmer::compareQueryKmer);
  FILE *sf = fopen(argv[7], "wb"); fwrite(q.buffer, 16, n, sf); fclose(sf);
  Buffer<Match> m(8000000);
  if (!km.matchKmers(&q, &m)) return 5;
  FILE *mf = fopen(argv[8], "w");
  for (size_t i = 0; i < m.startIndexOfReserve; i++) {
    const Match &x = m.buffer[i];
    fprintf(mf, "%u %u %u %d %d %u %u %u\n", (unsigned)x.qInfo.sequenceID, (unsigned)x.qInfo.frame, (unsigned)x.qInfo.pos,
            x.targetId, x.speciesId, x.dnaEncoding, (unsigned)x.rightEndHamming, (unsigned)x.hamming);
  }
  fclose(mf);
  return 0;
}
"""


# ---------------------------------------------------------------------------------------------------
# the design
CODONS = {  # the standard code's amino acids with four or six codons
    "L": ["TTA", "TTG", "CTT", "CTC", "CTA", "CTG"], "S": ["TCT", "TCC", "TCA", "TCG", "AGT", "AGC"],
    "R": ["CGT", "CGC", "CGA", "CGG", "AGA", "AGG"], "A": ["GCT", "GCC", "GCA", "GCG"],
    "G": ["GGT", "GGC", "GGA", "GGG"], "P": ["CCT", "CCC", "CCA", "CCG"], "T": ["ACT", "ACC", "ACA", "ACG"],
    "V": ["GTT", "GTC", "GTA", "GTG"]}
COMP = str.maketrans("ACGTNacgtn", "TGCANtgcan")


def revcomp(s):
    return s.translate(COMP)[::-1]


def rand_dna(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


class Family:
    """One AA 8-mer as N synonymous 24-nt variants: half of them within three codons of the first."""

    def __init__(self, rng, aas, n):
        self.aas = aas
        base = [int(rng.integers(len(CODONS[a]))) for a in aas]
        seen, self.members = set(), []
        while len(self.members) < n:
            c = list(base)
            if self.members and rng.random() < 0.5:
                c = [int(rng.integers(len(CODONS[a]))) for a in aas]
            elif self.members:
                for i in rng.permutation(8)[:int(rng.integers(1, 4))]:
                    c[i] = int(rng.integers(len(CODONS[aas[i]])))
            if tuple(c) not in seen:
                seen.add(tuple(c))
                self.members.append(c)
        self.seen = seen

    def dna(self, c):
        return "".join(CODONS[a][i] for a, i in zip(self.aas, c))

    def changed(self, rng, c, k):
        """c with k codons changed to another synonymous one."""
        c = list(c)
        for i in rng.permutation(8)[:k]:
            n = len(CODONS[self.aas[i]])
            c[i] = (c[i] + int(rng.integers(1, n))) % n
        return c


def design(rng, taxo, aa_sets):
    """Genomes (36 nt: flank, member, flank) with their strain taxIDs, and the families."""
    rank = np.array(taxo.rank)
    species = taxo.taxid[rank == "species"].tolist()
    parent = dict(zip(taxo.taxid.tolist(), taxo.parent.tolist()))
    strains = [t for t, r in zip(taxo.taxid.tolist(), taxo.rank) if r == "no rank" and t != 1]
    fams, genomes = [], []
    for aas, run in aa_sets:
        # a run of `run` records: run - dups variants, and dups of them again under another species
        dups = 0 if run == 1 else max(1, run // 8)
        f = Family(rng, aas, run - dups)
        f.dups = dups
        f.genomes = []
        for c in f.members:
            g = rand_dna(rng, 6) + f.dna(c) + rand_dna(rng, 6)
            f.genomes.append(g)
            genomes.append((g, strains[int(rng.integers(len(strains)))]))
        fams.append(f)
    # the same genome under a strain of another species (a diff of 0) and under a sister strain (one
    # record, the species' ID) for a few members of every run of at least two
    for f in fams:
        for g in f.genomes[:f.dups]:
            t = next(t for gg, t in genomes if gg == g)
            other = [s for s in strains if parent[s] != parent[t]]
            sister = [s for s in strains if parent[s] == parent[t] and s != t]
            genomes.append((g, other[int(rng.integers(len(other)))]))
            if sister and rng.random() < 0.5:
                genomes.append((g, sister[0]))
    return fams, genomes, species, parent, strains


def sprinkle(rng, s, rate=0.004):
    """N, IUPAC codes and lower case, as in ref_scanners.npz."""
    iupac = "NNNNNNRYKMSWBDHVUn"
    out = list(s)
    for i in range(len(out)):
        r = rng.random()
        if r < rate:
            out[i] = iupac[int(rng.integers(len(iupac)))]
        elif r > 1 - rate:
            out[i] = out[i].lower()
    return "".join(out)


def make_reads(rng, fams, extra_windows):
    """(mate 1, mate 2) strings. Singles of 60-150 bp first, then a paired set, the long read last."""
    def piece(f, exact=False):
        j = int(rng.integers(len(f.members)))
        k = 0 if exact else int(rng.integers(0, 4))
        g = f.genomes[j]
        if k:
            g = g[:6] + f.dna(f.changed(rng, f.members[j], k)) + g[30:]
        return g

    def embed(p, L, clean=False):
        L = max(L, len(p))
        a = int(rng.integers(0, L - len(p) + 1))
        s = rand_dna(rng, a) + p + rand_dna(rng, L - len(p) - a)
        if rng.random() < 0.5:
            s = revcomp(s)
        return s if clean else sprinkle(rng, s)

    singles = []
    for f in fams:
        for _ in range(1 if len(f.members) < 40 else 3):
            singles.append(embed(piece(f), int(rng.integers(60, 151))))
        singles.append(embed(piece(f, exact=True), int(rng.integers(60, 151)), clean=True))
    # exact duplicates of a window in two reads: the same strand, and opposite strands
    for f in fams[::3]:
        p = piece(f)
        a = rand_dna(rng, 20) + p + rand_dna(rng, 30)
        b = rand_dna(rng, 41) + p + rand_dna(rng, 13)
        singles += [a, b, revcomp(rand_dna(rng, 33) + p + rand_dna(rng, 40))]
    # two members of one family in one read (AA-equal, DNA-different neighbours in the sorted buffer)
    for f in fams[1::2]:
        if len(f.members) > 1:
            singles.append(embed(piece(f) + rand_dna(rng, 9) + piece(f), 100))
    for w in extra_windows:
        singles.append(embed(w, 90, clean=True))
    r = rand_dna(rng, 90)  # one read holds each kind of letter whatever the sprinkling drew
    singles.append(r[:10] + "N" + r[11:40] + "R" + r[41:70] + r[70].lower() + r[71:])
    for _ in range(3):
        singles.append(sprinkle(rng, rand_dna(rng, int(rng.integers(60, 151)))))
    pairs = []
    for i in range(8):
        f, g = fams[int(rng.integers(len(fams)))], fams[int(rng.integers(len(fams)))]
        pairs.append((embed(piece(f), 150), embed(piece(g), int(rng.integers(100, 151)))))
    long_parts = [piece(fams[int(rng.integers(len(fams)))]) + rand_dna(rng, int(rng.integers(3, 30))) for _ in range(10)]
    long_read = sprinkle(rng, "".join(long_parts) + rand_dna(rng, 40))
    assert len(long_read) >= 400
    return singles, pairs, long_read


# ---------------------------------------------------------------------------------------------------
class Tools:
    def __init__(self, d):
        self.d = pathlib.Path(d)
        flags = ["-O1", "-std=c++17", "-w", f"-I{REF}"]
        for name, text, extra in (("scan", make_ref_scanners.program(), []), ("write", make_ref_writer.program(), []),
                                  ("match", program(), ["-fopenmp"])):
            src = self.d / f"ref_{name}.cpp"
            src.write_text(text)
            subprocess.run(["g++", *flags, *extra, str(src), "-o", str(self.d / name)], check=True)
        subprocess.run(["g++", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *flags, "-fopenmp",
                        str(self.d / "ref_match.cpp"), "-o", str(self.d / "match_san")], check=True)
        self.n = 0

    def scan(self, fmt, syn, smer, reads):
        """fillQueryKmerBuffer of every (mate 1, mate 2): rows value, seqID, pos, frame in emission order."""
        inp = [f"{fmt} {syn} {smer} {len(reads)}"]
        for a, b in reads:
            inp += [f"{len(a)} {len(b)}", a] + ([b] if b else [])
        got = subprocess.run([str(self.d / "scan")], input="\n".join(inp) + "\n", capture_output=True, text=True,
                             check=True).stdout.split()
        return np.array(got, dtype=np.uint64).reshape(-1, 4)

    def write(self, values, ids, split_num):
        db = self.d / f"db{self.n}"
        self.n += 1
        db.mkdir()
        inp = f"{len(values)}\n" + "\n".join(f"{int(a)} {int(b)}" for a, b in zip(values, ids)) + "\n"
        subprocess.run([str(self.d / "write"), str(db), str(split_num)], input=inp, capture_output=True, text=True,
                       check=True)
        return db

    def match(self, db, fmt, skip, threads, kmers, sp_table, san=False):
        q, sp, so, mo = (self.d / n for n in ("q.bin", "sp.txt", "sorted.bin", "m.txt"))
        kmers.tofile(q)
        sp.write_text("".join(f"{t} {s}\n" for t, s in sp_table))
        r = subprocess.run([str(self.d / ("match_san" if san else "match")), str(db), str(fmt), str(skip), str(threads),
                            str(q), str(sp), str(so), str(mo)], capture_output=True, text=True)
        assert r.returncode == 0 and (not san or r.stderr == ""), (r.returncode, r.stderr[-3000:])
        qn = int(re.search(r"Query k-mer number\s*:\s*(\d+)", r.stdout).group(1))
        m = np.loadtxt(mo, dtype=np.int64, ndmin=2).reshape(-1, 8) if mo.stat().st_size else np.zeros((0, 8), np.int64)
        return np.fromfile(so, KMER), qn, canonical(m)


KMER = np.dtype([("value", "<u8"), ("info", "<u8")])


def canonical(m):
    """compareMatches order (sequenceID, speciesId, frame, pos, hamming, dnaEncoding), then targetId."""
    if len(m) == 0:
        return m
    return m[np.lexsort((m[:, 3], m[:, 5], m[:, 7], m[:, 2], m[:, 1], m[:, 4], m[:, 0]))]


def pack_info(seq, pos, frame):
    return pos.astype(np.uint64) | (seq.astype(np.uint64) << np.uint64(32)) | (frame.astype(np.uint64) << np.uint64(61))


def build_db(tools, rng, fmt, syn, genomes, parent, keep_between):
    """Target k-mers of the genomes -> sorted unique (value, species) -> taxIDs."""
    rows = tools.scan(fmt, syn, 5, [(g, "") for g, _ in genomes])
    rows = rows[rows[:, 3] == 0]  # frame 0: the genome's forward strand from its first base
    tax = np.array([t for _, t in genomes], np.int64)[rows[:, 1].astype(np.int64) - 1]
    sp = np.array([parent[int(t)] for t in tax], np.int64)
    val = rows[:, 0]
    aa = val >> np.uint64(24)
    if keep_between is not None:  # the first and the last family's runs are the DB's first and last records
        lo, hi = keep_between(val)
        ok = (aa >= lo) & (aa <= hi)
        val, tax, sp = val[ok], tax[ok], sp[ok]
    order = np.lexsort((tax, sp, val))
    val, tax, sp = val[order], tax[order], sp[order]
    first = np.ones(len(val), bool)
    first[1:] = (val[1:] != val[:-1]) | (sp[1:] != sp[:-1])
    grp = np.cumsum(first) - 1
    same = np.ones(grp[-1] + 1, bool)  # one taxID in the group: keep it; several strains: their species
    np.logical_and.at(same, grp[1:], first[1:] | (tax[1:] == tax[:-1]))
    ids = np.where(same[grp[first]], tax[first], sp[first])
    return val[first], ids.astype(np.uint32), int(rows[rows[:, 0] == val[-1]][0, 1]) - 1


def run_case(tools, name, fmt, val, ids, kmers, sp_table, flag_rng, arrays, splits=SPLITS, threads=THREADS):
    """One DB: written with every split count, with bit 31 set on a share of info words (skipRedundancy 0)
    and with clean info words (skipRedundancy 0 and 1); every thread count; the sanitised build."""
    flag = np.where(flag_rng.random(len(ids)) < FLAG_SHARE, np.uint32(1 << 31), np.uint32(0)) if flag_rng else None
    ref, n_runs = None, 0
    for sn in splits:
        variants = [(ids, 0), (ids, 1)] + ([(ids | flag, 0)] if flag is not None else [])
        for k, (info_ids, skip) in enumerate(variants):
            db = tools.write(val, info_ids, sn)
            for t in threads:
                t = min(t, len(kmers))
                sorted_q, qn, m = tools.match(db, fmt, skip, t, kmers, sp_table)
                if ref is None:
                    ref = (sorted_q, qn, m)
                assert qn == ref[1] and np.array_equal(sorted_q, ref[0])
                assert np.array_equal(m, ref[2]), f"{name}: split {sn} skip {skip} threads {t} changed the matches"
                n_runs += 1
                if t in (1, 16) or t == len(kmers):
                    s2, q2, m2 = tools.match(db, fmt, skip, t, kmers, sp_table, san=True)
                    assert q2 == qn and np.array_equal(m2, m) and np.array_equal(s2, sorted_q)
            if k == len(variants) - 1:  # diffIdx and info do not depend on the split count
                files = {f: np.fromfile(db / f, t) for f, t in (("diffIdx", np.uint16), ("info", np.uint32))}
                for f, a in files.items():
                    assert np.array_equal(arrays.setdefault(f"{name}_{f}", a), a)
                arrays[f"{name}_s{sn}_split"] = np.fromfile(db / "split", np.uint64)
    sorted_q, qn, m = ref
    arrays[f"{name}_query"] = sorted_q
    arrays[f"{name}_query_kmer_number"] = np.int64(qn)
    arrays[f"{name}_m_qinfo"] = pack_info(m[:, 0], m[:, 2], m[:, 1])
    arrays[f"{name}_m_target"] = m[:, 3].astype(np.uint32)
    arrays[f"{name}_m_species"] = m[:, 4].astype(np.uint32)
    arrays[f"{name}_m_dna"] = m[:, 5].astype(np.uint32)
    arrays[f"{name}_m_reh"] = m[:, 6].astype(np.uint16)
    arrays[f"{name}_m_ham"] = m[:, 7].astype(np.uint8)
    print(f"{name}: {len(val)} DB k-mers, {qn} query k-mers, {len(m)} matches; {n_runs} runs agree, sanitised runs clean")


TAX = dict(n_species=10, strains_per_species=3, seed=11)
# (name, kmerFormat, syncmer)
MAIN = [("fmt2", 2, 0), ("fmt1", 1, 0), ("fmt2_syncmer", 2, 1)]


def generate():
    from metabuli_work_amd import synth
    taxo = synth.make_taxonomy(**TAX)
    arrays = {"tax_params": np.array([TAX["n_species"], TAX["strains_per_species"], TAX["seed"]], np.int64),
              "threads": np.array(THREADS), "splits": np.array(SPLITS)}
    with tempfile.TemporaryDirectory() as d:
        tools = Tools(d)
        names = []
        for di, (name, fmt, syn) in enumerate(MAIN):
            rng = np.random.default_rng([20261020, di])
            letters = list(CODONS)
            runs = RUNS if not syn else (1, 2, 3, 48, 49, 65)
            aa_sets = [("".join(letters[i] for i in rng.integers(0, len(letters), 8)), n) for n in runs + (2, 5, 70)]
            fams, genomes, species, parent, strains = design(rng, taxo, aa_sets)
            # unrelated genomes: singletons between the families. Syncmers are a share of the windows, and a DB
            # of fewer k-mers than splitNum - 1 gets no split entry at all (sizeOfSplit 0), which sends every
            # query above AA part 0 to data[numOfDiffIdxSplits_use - 2] = data[-1]: outside defined behaviour
            for _ in range(650 if syn else 400):
                genomes.append((rand_dna(rng, 150 if syn else 36), strains[int(rng.integers(len(strains)))]))

            def between(val, fams=fams, fmt=fmt, syn=syn):
                v = tools.scan(fmt, syn, 5, [(f.genomes[0], "") for f in fams])
                v = v[(v[:, 3] == 0) & (v[:, 2] == 6)][:, 0] >> np.uint64(24)
                assert len(v) == len(fams)
                return v.min(), v.max()
            val, ids, last = build_db(tools, rng, fmt, syn, genomes, parent, None if syn else between)
            sp_table = [(t, parent[t]) for t in strains] + [(s, s) for s in species]
            # windows that sort above every DB k-mer and below the first one
            # and exact copies of the genome that holds the DB's last k-mer (never a candidate), both strands
            extra = [rand_dna(rng, 36) for _ in range(4)] + [genomes[last][0], revcomp(genomes[last][0])]
            singles, pairs, long_read = make_reads(rng, fams, extra)
            reads = [(s, "") for s in singles] + [(long_read, "")] + pairs  # the long read: last of the single-end set
            # paired mates share a read: the set is scanned as the reference scans a paired read
            q = tools.scan(fmt, syn, 5, reads)
            kmers = np.zeros(len(q), KMER)
            kmers["value"] = q[:, 0]
            kmers["info"] = pack_info(q[:, 1], q[:, 2], q[:, 3])
            run_case(tools, name, fmt, val, ids, kmers, sp_table, np.random.default_rng([7, di]), arrays)
            arrays[f"{name}_seq1"] = np.array([a for a, _ in reads])
            arrays[f"{name}_seq2"] = np.array([b for _, b in reads])
            arrays[f"{name}_n_single"] = np.int64(len(singles))
            arrays[f"{name}_n_pair"] = np.int64(len(pairs))
            arrays[f"{name}_fmt"] = np.array([fmt, syn, 5], np.int64)
            arrays[f"{name}_species_table"] = np.array(sp_table, np.int32)
            names.append(name)
        arrays["dbs"] = np.array(names)
    return arrays


if __name__ == "__main__":
    arrays = generate()
    out = HERE / "ref_match.npz"
    np.savez_compressed(out, **arrays)
    print("wrote", out, out.stat().st_size, "bytes")
    from tests.ref_match_fixture import coverage_table
    for k, v in coverage_table(dict(np.load(out))).items():
        print(f"{k:44s} {v}")
