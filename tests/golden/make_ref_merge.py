"""Regenerate tests/golden/ref_merge.npz: the diffIdx / info / split files the reference's OWN merge
(IndexCreator::mergeTargetFiles<DB_CREATION>) writes for designed sets of input DBs.

Runs only where the reference tree is mounted; the committed .npz is what the tests read. Nothing of the
reference enters the repository: as in make_ref_writer.py and make_ref_group_filter.py the code is cut out
of the reference's files at run time into a throw-away C++ file in a temporary directory, compiled
(g++ -O1 -std=c++17 -fopenmp, with the reference's GeneticCode.h and BitManipulateMacros.h included in place),
run and deleted. The cut code (reference file), each whole:
* IndexCreator.h `IndexCreator::mergeTargetFiles<M>`, `filterKmers<M>`, `areKmersDuplicate<M>`, the
  `FilterMode` enum, `struct Split` and `AminoAcidPart`
* IndexCreator.cpp the constructor's `MARKER` choice and `IndexCreator::getDiffIdx`
* DeltaIdxReader.h `class DeltaIdxReader`
* common.h `likely` / `unlikely`, `struct Buffer`, `struct ReadBuffer`, `struct WriteBuffer`
* Kmer.h `QueryKmerInfo`, `TargetKmerInfo`, `Kmer` (with compareTargetKmer), `DiffIdxSplit`
Restated in the driver below, because MMseqs2 is not in the reference tree:
* `taxonomy->LCA(vector<TaxID>)`: the pairwise LCA over the list in its order, each by a parent walk over
  arrays read from a file (taxa that do not exist are skipped, as NcbiTaxonomy::LCA does)
* the `taxId2speciesId` table: read from the same file, computed here from the synthetic taxonomy
* `FileUtil::getFileSize` (stat) and `SORT_PARALLEL` (std::sort)
Stand-ins are declarations only: `LocalParameters{splitNum, threads, skipRedundancy, reducedAA}`, an
`IndexCreator` with the members the cut code reads, an `UnirefTree` whose getLCA the DB_CREATION
instantiation never calls.

Buffer sizes. Four literals of mergeTargetFiles are memory devices (about 27 GB as written) and are
replaced textually by variables the driver sets from its arguments; each replacement must hit exactly
once (asserted), so a changed reference stops the generator: the `bufferSize` of the two write buffers
(512M), `valueBufferSize` (16M), the readers' read buffer (4M) and `kmerBufferSize` (1G). Every case runs
at two settings, each with 1, 3 and 16 threads (par.threads and the OpenMP team):
* one pass: a value buffer that holds any input whole and a k-mer buffer that holds every round's
  reservation, so one outer pass loads, sorts and writes everything (the pass count is asserted);
* many passes: a value buffer of 64, a read buffer of 32 and a k-mer buffer of 1, which the code's own
  rule raises to valueBufferSize * files * 2: two getValues rounds per outer pass while every input
  is open, so the `max` cut-offs fall inside the data and lastKmer, the write counts and splitCheck
  carry from pass to pass.
A committed case's six runs give byte-identical diffIdx, info and split (asserted). One class of input
may miss that: a reader whose value buffer ends on value v has not yet loaded its next entry of the same
v (DeltaIdxReader::getValues copies what it holds up to `max`), so an outer pass can end between the
two and the entries of one value are written in two passes. The generator draws a case's random parts
again (next sub-seed) when the many-pass runs differ from the one-pass runs, after checking that the
first difference sits at a value that repeats inside one input; the first such draw is kept in the
.npz as `artefact` with both results, out of the device comparison (comparable = 0), the one-pass
bytes as its expected result.

Never run (read from the code; they hang or read out of bounds): an input with an empty diffIdx / info
(an empty reader never becomes "completed" and holds `max` at 0), and a merge of exactly one k-mer.

kmer_format: the cut code reads kmerFormat only in AminoAcidPart (formats 3 and 4 take the whole
value); formats 1 and 2 run the same code, so the fixture holds one result for both.

Inputs are (value, species, taxID)-sorted lists encoded by tests/group_filter_cases.encode_diffidx (the
plain-Python encoder ref_group_filter.npz pins) and checked against tests/dbref.decode_diff.
"""
import pathlib
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
REF = pathlib.Path("/root/reference/src/commons")
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE.parent.parent))

from dbref import Tree, decode_diff, diff_words  # noqa: E402
from group_filter_cases import encode_diffidx  # noqa: E402
from make_ref_functions import definitions, if_else  # noqa: E402
from make_ref_scanners import class_text  # noqa: E402
from metabuli_work_amd import synth  # noqa: E402

THREADS = (1, 3, 16)
TAXONOMY = (8, 8, 5)  # synth.make_taxonomy(species, strains per species, seed)
MANY = {"write": 4096, "value": 64, "read": 32, "kmer": 1}
RUN_TIMEOUT = 120
SEED = 20261022
TOP = 1 << 62  # above every drawn value: an AA part of its own

# the four literals of mergeTargetFiles and the driver variable each becomes
LITERALS = [(r"1024 \* 1024 \* 512\b", "G_WRITE"), (r"1024 \* 1024 \* 16\b", "G_VALUE"),
            (r"1024 \* 1024 \* 4\b", "G_READ"), (r"1024 \* 1024 \* 1024\b", "G_KMER")]


def program() -> str:
    cm = (REF / "common.h").read_text()
    km = (REF / "Kmer.h").read_text()
    ih = (REF / "IndexCreator.h").read_text()
    ic = (REF / "IndexCreator.cpp").read_text()
    dr = (REF / "DeltaIdxReader.h").read_text()
    macros = [re.search(r"(?m)^#define %s.*$" % n, cm).group(0) for n in ("likely", "unlikely")]
    mode = re.search(r"(?m)^enum class FilterMode \{[^}]*\};", ih).group(0)
    aa = definitions(ih, r"size_t AminoAcidPart\(size_t kmer\)")
    marker = if_else(ic, "par.reducedAA == 1")
    merge = definitions(ih, r"template <FilterMode M>\s*void IndexCreator::mergeTargetFiles\(\)")
    filt = definitions(ih, r"template <FilterMode M>\s*void IndexCreator::filterKmers\(")
    dup = definitions(ih, r"template <FilterMode M>\s*bool IndexCreator::areKmersDuplicate\(")
    diff = definitions(ic, r"void IndexCreator::getDiffIdx\(\s*uint64_t & lastKmer")
    assert [len(x) for x in (aa, merge, filt, dup, diff)] == [1] * 5
    text = merge[0]
    for pat, var in LITERALS:
        text, hits = re.subn(pat, var, text)
        assert hits == 1, f"{pat}: {hits} hits in mergeTargetFiles"
    return "\n".join([
        "#include <algorithm>", "#include <atomic>", "#include <bitset>", "#include <cstdint>", "#include <cstdio>",
        "#include <cstdlib>", "#include <cstring>", "#include <ctime>", "#include <fstream>", "#include <iomanip>",
        "#include <iostream>", "#include <omp.h>", "#include <string>", "#include <sys/stat.h>", "#include <unordered_map>",
        "#include <utility>", "#include <vector>", '#include "GeneticCode.h"',
        '#include "BitManipulateMacros.h"', "using namespace std;", "typedef int TaxID;", *macros, "#define SORT_PARALLEL std::sort",
        "static size_t G_WRITE, G_VALUE, G_READ, G_KMER;",
        "struct FileUtil { static size_t getFileSize(const std::string &f) {"
        " struct stat st; if (stat(f.c_str(), &st) != 0) exit(3); return (size_t)st.st_size; } };",
        class_text(km, "struct QueryKmerInfo {"), class_text(km, "struct TargetKmerInfo {"),
        class_text(km, "struct Kmer {"), class_text(km, "struct DiffIdxSplit{"),
        "template<typename T>\n" + class_text(cm, "struct Buffer {"),
        "template<typename T>\n" + class_text(cm, "struct ReadBuffer {"),
        "template<typename T>\n" + class_text(cm, "struct WriteBuffer {"),
        class_text(dr, "class DeltaIdxReader {"), mode, STANDINS,
        "struct IndexCreator {",
        "  LocalParameters par; int kmerFormat = 2; uint64_t MARKER;",
        "  std::unordered_map<TaxID, TaxID> taxId2speciesId;",
        "  TaxonomyWrapper *taxonomy = nullptr; UnirefTree *unirefTree = nullptr;",
        "  std::string dbDir, mergedDeltaIdxFileName, mergedInfoFileName, deltaIdxSplitFileName;",
        "  std::vector<std::string> deltaIdxFileNames, infoFileNames;",
        class_text(ih, "struct Split{"),
        "  void setMarker() {", marker, "  }",
        *aa,
        "  template <FilterMode M> void mergeTargetFiles();",
        "  template <FilterMode M> void filterKmers(Buffer<Kmer> &kmerBuffer, size_t *uniqeKmerIdx, size_t &uniqKmerCnt,"
        " vector<pair<size_t, size_t>> &uniqKmerIdxRanges);",
        "  template <FilterMode M> bool areKmersDuplicate(const Kmer &kmer1, const Kmer &kmer2);",
        "  static void getDiffIdx(uint64_t &lastKmer, uint64_t entryToWrite, WriteBuffer<uint16_t> &diffBuffer);",
        "};", text, *filt, *dup, *diff, DRIVER])


STANDINS = r"""
struct LocalParameters { int splitNum; int threads; int skipRedundancy; int reducedAA; };
struct TaxonNode { TaxID taxId; };
struct TaxonomyWrapper {  // NcbiTaxonomy::LCA(vector) restated over parent arrays
  std::vector<TaxID> parent; std::vector<int> depth; std::vector<TaxonNode> node;
  bool exists(TaxID t) const { return t > 0 && (size_t)t < parent.size() && parent[t] != 0; }
  TaxID lca2(TaxID a, TaxID b) const {
    while (a != b) {
      int da = depth[a], db = depth[b];
      if (da >= db) a = parent[a];
      if (db >= da) b = parent[b];
    }
    return a;
  }
  const TaxonNode *LCA(const std::vector<TaxID> &taxa) const {
    size_t i = 0;
    while (i < taxa.size() && !exists(taxa[i])) i++;
    if (i == taxa.size()) return nullptr;
    TaxID red = taxa[i++];
    for (; i < taxa.size(); i++) if (exists(taxa[i])) red = lca2(red, taxa[i]);
    return &node[red];
  }
};
struct UnirefTree { uint32_t getLCA(const std::vector<uint32_t> &) const { return 0; } };
"""

# argv: outPrefix splitNum threads write value read kmer taxFile diff0 info0 [diff1 info1 ...]
# taxFile: "<n>", then n lines "taxID parent species" (the root is its own parent; species 0: none)
DRIVER = r"""
int main(int argc, char **argv) {
  if (argc < 11 || (argc - 9) % 2) return 2;
  IndexCreator ic;
  ic.par = LocalParameters{atoi(argv[2]), atoi(argv[3]), 1, 0};
  ic.setMarker();
  G_WRITE = strtoull(argv[4], nullptr, 10); G_VALUE = strtoull(argv[5], nullptr, 10);
  G_READ = strtoull(argv[6], nullptr, 10); G_KMER = strtoull(argv[7], nullptr, 10);
  TaxonomyWrapper tax;
  {
    std::ifstream f(argv[8]);
    size_t n; if (!(f >> n)) return 4;
    std::vector<TaxID> id(n), pa(n), sp(n);
    TaxID mx = 0;
    for (size_t i = 0; i < n; i++) { if (!(f >> id[i] >> pa[i] >> sp[i])) return 4; if (id[i] > mx) mx = id[i]; }
    tax.parent.assign(mx + 1, 0); tax.depth.assign(mx + 1, 0); tax.node.resize(mx + 1);
    for (size_t i = 0; i < n; i++) { tax.parent[id[i]] = pa[i]; tax.node[id[i]].taxId = id[i]; }
    for (size_t i = 0; i < n; i++) {
      int d = 0; for (TaxID x = id[i]; x != 1; x = tax.parent[x]) d++;
      tax.depth[id[i]] = d;
      if (sp[i]) ic.taxId2speciesId[id[i]] = sp[i];
    }
  }
  ic.taxonomy = &tax;
  std::string out = argv[1];
  ic.dbDir = out;
  ic.mergedDeltaIdxFileName = out + "diffIdx"; ic.mergedInfoFileName = out + "info"; ic.deltaIdxSplitFileName = out + "split";
  for (int i = 9; i + 1 < argc; i += 2) { ic.deltaIdxFileNames.push_back(argv[i]); ic.infoFileNames.push_back(argv[i + 1]); }
  omp_set_dynamic(0);
  omp_set_num_threads(ic.par.threads);
  ic.mergeTargetFiles<FilterMode::DB_CREATION>();
  return 0;
}
"""


# ---- the world and the inputs -----------------------------------------------------------------------------
class World:
    def __init__(self):
        self.taxo = synth.make_taxonomy(TAXONOMY[0], TAXONOMY[1], seed=TAXONOMY[2])
        self.tree = Tree(self.taxo)
        leaves = [t for t, r in zip(self.taxo.taxid.tolist(), self.taxo.rank) if r == "no rank" and t != 1]
        self.species = sorted({int(self.tree.sp[t]) for t in leaves})
        self.strains = {s: sorted(t for t in leaves if self.tree.sp[t] == s) for s in self.species}
        self.leaves = np.array(leaves, np.int64)
        assert all(len(v) == TAXONOMY[1] for v in self.strains.values()) and 0 not in self.species

    def tax_file(self, path):
        ids = self.taxo.taxid.tolist()
        pathlib.Path(path).write_text(f"{len(ids)}\n" + "".join(
            f"{t} {p} {int(self.tree.sp[t])}\n" for t, p in zip(ids, self.taxo.parent.tolist())))


def values(rng, n, runs):
    """n distinct non-zero values: AA parts from a pool of about n / runs (runs of several k-mers), DNA parts
    random, one in fifty anywhere below 2^62 (deltas of up to five words)."""
    pool = rng.integers(1, 21 ** 8, max(2, int(n / runs)), dtype=np.uint64)
    out = np.zeros(0, np.uint64)
    while len(out) < n:
        m = n - len(out) + 8
        v = (pool[rng.integers(0, len(pool), m)] << np.uint64(24)) | rng.integers(0, 1 << 24, m, dtype=np.uint64)
        far = rng.random(m) < 0.02
        v[far] = rng.integers(1, 1 << 62, int(far.sum()), dtype=np.uint64)
        out = np.unique(np.concatenate([out, v]))
    return rng.permutation(out)[:n]


def finish(w, entries):
    """One input from (value, taxID) pairs: one entry per (value, taxID), in compareTargetKmer order."""
    e = sorted(set((int(v), int(w.tree.sp[t]), int(t)) for v, t in entries))
    return np.array([x[0] for x in e], np.uint64), np.array([x[2] for x in e], np.uint32)


def scatter(w, rng, sizes, runs=3.0, cross=0.35, within=4):
    """Inputs of the given sizes over one universe of values. A share `cross` of an input's values is also
    drawn by other inputs: under another strain of the same species, under the same taxID, or under another
    species (a third each). `within` values per input come twice under two species of the same input."""
    uni = values(rng, int(sum(sizes)), runs)
    home_sp = rng.choice(w.species, len(uni))
    files, at = [], 0
    for n in sizes:
        own = np.arange(at, at + n)
        at += n
        ent = [(uni[j], rng.choice(w.strains[home_sp[j]])) for j in own]
        files.append(ent)
    for f, n in enumerate(sizes):
        if len(sizes) == 1:
            break
        for _ in range(int(cross * n)):
            g = int(rng.choice([x for x in range(len(sizes)) if x != f]))
            v, t = files[g][int(rng.integers(0, sizes[g]))]
            sp = int(w.tree.sp[t])
            kind = int(rng.integers(0, 3))
            if kind == 0:
                t2 = rng.choice([x for x in w.strains[sp] if x != t])
            elif kind == 1:
                t2 = t
            else:
                t2 = rng.choice(w.strains[int(rng.choice([s for s in w.species if s != sp]))])
            files[f].append((v, t2))
        for _ in range(within):
            v, t = files[f][int(rng.integers(0, n))]
            sp = int(w.tree.sp[t])
            files[f].append((v, rng.choice(w.strains[int(rng.choice([s for s in w.species if s != sp]))])))
    return files


def spread_group(w, rng, files, value=None):
    """One (value, species) group with a member in every input, a different strain in each (as far as the
    species has strains)."""
    v = int(values(rng, 1, 1)[0]) if value is None else value
    st = w.strains[w.species[2]]
    for i, f in enumerate(files):
        f.append((v, st[i % len(st)]))


def case_two(w, rng):
    files = scatter(w, rng, [600, 400], within=3)
    # a group of four strains: two in each input (its own repeat inside an input)
    v = int(values(rng, 1, 1)[0])
    st = w.strains[w.species[1]]
    files[0] += [(v, st[0]), (v, st[1])]
    files[1] += [(v, st[2]), (v, st[3])]
    spread_group(w, rng, files)
    return files, 16


def case_many(n, equal):
    def build(w, rng):
        sizes = [150] * n if equal else [int(x) for x in rng.permutation(np.linspace(60, 420, n).astype(int))]
        files = scatter(w, rng, sizes, within=1)
        spread_group(w, rng, files)
        if equal:  # the same number of entries in every input, whatever the set() in finish() dropped
            m = min(len(finish(w, f)[0]) for f in files)
            files = [list(zip(*[a[:m] for a in finish(w, f)])) for f in files]
            spread_group(w, rng, files, value=TOP + 5)
        return files, 16
    return build


def case_total(split_num, total):
    """`total` k-mers before merging over two inputs, all values distinct."""
    def build(w, rng):
        v = values(rng, total, 2.0)
        t = rng.choice(w.leaves, total)
        a = max(1, total // 3)
        return [list(zip(v[:a], t[:a])), list(zip(v[a:], t[a:]))], split_num
    return build


def case_dups_short(split_num):
    """Two thirds of the entries meet an entry of the other input in one (value, species) group: the written
    count stays below the later offsets."""
    def build(w, rng):
        n = 3 * (split_num - 1)
        v = values(rng, n, 3.0)
        t = rng.choice(w.leaves, n)
        a = list(zip(v, t))
        b = [(x, rng.choice(w.strains[int(w.tree.sp[y])])) for x, y in a[: 2 * n // 3]] + \
            list(zip(values(rng, n // 3, 3.0), rng.choice(w.leaves, n // 3)))
        return [a, b], split_num
    return build


def case_last_run(split_num):
    """The last AA run holds the last reachable offsets: no entry follows them."""
    def build(w, rng):
        n = 5 * (split_num - 1)
        v = values(rng, n - 7, 3.0)  # sizeOfSplit is 5: the last two offsets fall among the last seven k-mers
        top = (np.uint64(TOP) | np.unique(rng.integers(0, 1 << 24, 64, dtype=np.uint64))[:7])
        v = np.concatenate([v, top])
        t = rng.choice(w.leaves, n)
        idx = rng.permutation(n)
        a, b = idx[: n // 2], idx[n // 2:]
        return [list(zip(v[a], t[a])), list(zip(v[b], t[b]))], split_num
    return build


def case_straddle(split_num):
    """AA runs of 15 k-mers over a sizeOfSplit of 6: every run holds two or three offsets."""
    def build(w, rng):
        n = 6 * (split_num - 1)
        aa = np.sort(np.unique(rng.integers(1, 21 ** 8, n, dtype=np.uint64))[: (n + 14) // 15])
        dna = np.unique(rng.integers(0, 1 << 24, 4 * n, dtype=np.uint64))[:n]
        v = (aa[np.arange(n) // 15] << np.uint64(24)) | rng.permutation(dna)
        t = rng.choice(w.leaves, n)
        idx = rng.permutation(n)
        a, b = idx[: n // 3], idx[n // 3:]
        return [list(zip(v[a], t[a])), list(zip(v[b], t[b]))], split_num
    return build


def case_last(dup):
    """An output ending on a duplicate pair or on a singleton; drawn until, with 3 and with 16 threads, one
    thread range ends on a duplicate pair and one on a singleton (ranges of more than 100 k-mers at 16)."""
    def build(w, rng):
        while True:
            files = scatter(w, rng, [900, 700], runs=3.0, cross=0.5, within=2)
            inputs = [finish(w, f) for f in files]
            if all(min(range_ends(w, inputs, th)) > 0 for th in (3, 16)):
                break
        top = TOP + (9 << 24) + 12345
        st = w.strains[w.species[4]]
        files[0].append((top, st[0]))
        if dup:
            files[1].append((top, st[1]))
        return files, 64
    return build


def case_tiny(equal):
    def build(w, rng):
        v = values(rng, 2, 1.0)
        st = w.strains[w.species[3]]
        return [[(v[0], st[0])], [(v[0] if equal else v[1], st[1])]], 4
    return build


def cases():
    out = [("two_meetings", case_two)]
    for n in (3, 5, 8):
        out += [(f"in{n}_unequal", case_many(n, False)), (f"in{n}_equal", case_many(n, True))]
    for s in (4, 16, 64):
        out += [(f"s{s}_total_sm2", case_total(s, s - 2)), (f"s{s}_total_sm1", case_total(s, s - 1)),
                (f"s{s}_total_2sm1", case_total(s, 2 * (s - 1))), (f"s{s}_dups_short", case_dups_short(s)),
                (f"s{s}_last_run", case_last_run(s)), (f"s{s}_straddle", case_straddle(s))]
    out += [("last_dup", case_last(True)), ("last_single", case_last(False)),
            ("tiny_equal", case_tiny(True)), ("tiny_unequal", case_tiny(False))]
    return out


# ---- running the reference --------------------------------------------------------------------------------
def run_ref(exe, d, tax, inputs, split_num, threads, sizes):
    """(diffIdx, info, split, outer passes) of one run."""
    out = pathlib.Path(d) / "out_"
    args = [str(exe), str(out), str(split_num), str(threads), *(str(sizes[k]) for k in ("write", "value", "read", "kmer")),
            str(tax)]
    for i in range(len(inputs)):
        args += [str(pathlib.Path(d) / f"in{i}.diffIdx"), str(pathlib.Path(d) / f"in{i}.info")]
    r = subprocess.run(args, capture_output=True, text=True, check=True, timeout=RUN_TIMEOUT)
    got = tuple(np.fromfile(str(out) + n, dt) for n, dt in (("diffIdx", np.uint16), ("info", np.uint32), ("split", np.uint64)))
    for n in ("diffIdx", "info", "split"):
        pathlib.Path(str(out) + n).unlink()
    return got + (r.stdout.count("K-mer loading"),)


def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3]))


def one_pass_sizes(inputs):
    big = max(len(v) for v, _ in inputs) + 1
    n = len(inputs)
    return {"write": 4096, "value": big, "read": 4096, "kmer": big * n * (n + 1) // 2 + big}


def range_ends(w, inputs, threads):
    """Where filterKmers' thread ranges end when everything is loaded at once (the generator's own reading of
    the splitWidth rule, used only to say what a case holds): (ends on a duplicate pair, ends on a singleton)."""
    v = np.concatenate([a for a, _ in inputs])
    t = np.concatenate([b for _, b in inputs]).astype(np.int64)
    sp = w.tree.sp[t]
    o = np.lexsort((t, sp, v))
    v, sp = v[o], sp[o]
    n, width, start, pair, single = len(v), len(v) // threads, 0, 0, 0
    if width == 0:
        return 0, 0
    for _ in range(threads - 1):
        for j in range(start + width, n - 1):
            if v[j] >> np.uint64(24) != v[j + 1] >> np.uint64(24):
                if j > start and v[j] == v[j - 1] and sp[j] == sp[j - 1]:
                    pair += 1
                else:
                    single += 1
                start = j + 1
                break
    return pair, single


def cross_groups(w, inputs):
    keys = [set(zip(v.tolist(), w.tree.sp[t.astype(np.int64)].tolist())) for v, t in inputs]
    seen, cross = set(), set()
    for k in keys:
        cross |= k & seen
        seen |= k
    return len(cross)


def repeats_inside_an_input(inputs, value):
    return any(int((v == np.uint64(value)).sum()) >= 2 for v, _ in inputs)


def reference_case(exe, d, w, tax, name, build, seed):
    """Draw the case until its six runs agree; returns (inputs, split_num, one-pass result, many-pass passes,
    the rejected draws as (inputs, split_num, one-pass result, many-pass result))."""
    rejected = []
    for sub in range(50):
        rng = np.random.default_rng([seed, sub, sum(name.encode())])
        files, split_num = build(w, rng)
        inputs = [finish(w, f) for f in files]
        assert all(len(v) for v, _ in inputs), "an empty input: the reference's merge never ends"
        assert sum(len(v) for v, _ in inputs) >= 2, "a merge of one k-mer"
        for i, (v, t) in enumerate(inputs):
            words = encode_diffidx(v)
            assert np.array_equal(decode_diff(words), v) and len(words) == int(diff_words(v).sum())
            words.tofile(pathlib.Path(d) / f"in{i}.diffIdx")
            t.astype(np.uint32).tofile(pathlib.Path(d) / f"in{i}.info")
        one = [run_ref(exe, d, tax, inputs, split_num, th, one_pass_sizes(inputs)) for th in THREADS]
        assert all(r[3] == 1 for r in one), f"{name}: the one-pass setting took {[r[3] for r in one]} passes"
        assert all(same(one[0], r) for r in one), f"{name}: the one-pass runs differ between thread counts"
        many = [run_ref(exe, d, tax, inputs, split_num, th, MANY) for th in THREADS]
        assert all(same(many[0], r) for r in many), f"{name}: the many-pass runs differ between thread counts"
        if same(one[0], many[0]):
            return inputs, split_num, one[0], many[0][3], rejected
        # the only excuse: the first difference sits at a value that repeats inside one input
        va, vb = decode_diff(one[0][0]), decode_diff(many[0][0])
        m = min(len(va), len(vb))
        diff = np.flatnonzero((va[:m] != vb[:m]) | (one[0][1][:m] != many[0][1][:m]))
        at = int(diff[0]) if len(diff) else m - 1
        cand = {int(va[min(at, len(va) - 1)]), int(vb[min(at, len(vb) - 1)]), int(vb[max(at - 1, 0)])}
        assert any(repeats_inside_an_input(inputs, c) for c in cand), \
            f"{name}: the settings differ at k-mer {at}, not at a value repeated inside one input"
        print(f"  {name} draw {sub}: many-pass differs from one-pass at k-mer {at} (value {int(vb[min(at, len(vb) - 1)])}, "
              f"repeated inside an input); {len(one[0][1])} vs {len(many[0][1])} entries written; drawn again")
        rejected.append((inputs, split_num, one[0], many[0]))
    raise AssertionError(f"{name}: no draw agreed")


def store(out, name, inputs, split_num, result, comparable):
    out[f"{name}_n_in"] = np.int64(len(inputs))
    out[f"{name}_split_num"] = np.int64(split_num)
    out[f"{name}_comparable"] = np.int64(comparable)
    for i, (v, t) in enumerate(inputs):
        out[f"{name}_in{i}_diffIdx"] = encode_diffidx(v)
        out[f"{name}_in{i}_info"] = t.astype(np.uint32)
    out[f"{name}_diffIdx"], out[f"{name}_info"], out[f"{name}_split"] = result[:3]


if __name__ == "__main__":
    w = World()
    out = {"taxonomy": np.array(TAXONOMY), "tax_id": w.taxo.taxid, "tax_parent": w.taxo.parent,
           "tax_rank": np.array(w.taxo.rank), "threads": np.array(THREADS),
           "many_sizes": np.array([MANY[k] for k in ("write", "value", "read", "kmer")])}
    names, artefact = [], None
    with tempfile.TemporaryDirectory() as d:
        src, exe, tax = (pathlib.Path(d) / n for n in ("ref_merge.cpp", "ref_merge", "tax.txt"))
        src.write_text(program())
        subprocess.run(["g++", "-O1", "-std=c++17", "-fopenmp", "-w", f"-I{REF}", str(src), "-o", str(exe)], check=True)
        w.tax_file(tax)
        for name, build in cases():
            inputs, split_num, res, passes, rejected = reference_case(exe, d, w, tax, name, build, SEED)
            store(out, name, inputs, split_num, res, 1)
            out[f"{name}_one_sizes"] = np.array([one_pass_sizes(inputs)[k] for k in ("write", "value", "read", "kmer")])
            out[f"{name}_many_passes"] = np.int64(passes)
            names.append(name)
            if rejected and artefact is None:
                artefact = (name, *rejected[0])
            total = sum(len(v) for v, _ in inputs)
            entries = int((res[2].reshape(-1, 3)[1:, 1] != 0).sum())
            ends = {th: range_ends(w, inputs, th) for th in (3, 16)}
            print(f"{name}: {len(inputs)} inputs of {[len(v) for v, _ in inputs]} = {total} k-mers, splitNum {split_num}, "
                  f"{cross_groups(w, inputs)} cross-input groups, {len(res[1])} written, {entries} split entries after "
                  f"entry 0, many-pass setting {passes} passes, thread ranges ending (pair, singleton) "
                  f"3: {ends[3]} 16: {ends[16]}, all six runs agree: True")
        if artefact is not None:
            name, inputs, split_num, one, many = artefact
            store(out, "artefact", inputs, split_num, one, 0)
            out["artefact_from"] = np.array(name)
            out["artefact_many_diffIdx"], out["artefact_many_info"], out["artefact_many_split"] = many[:3]
            names.append("artefact")
            print(f"artefact: a rejected draw of {name}, {sum(len(v) for v, _ in inputs)} k-mers, all six runs agree: False")
    out["cases"] = np.array(names)
    np.savez_compressed(HERE / "ref_merge.npz", **out)
    print("wrote", HERE / "ref_merge.npz", (HERE / "ref_merge.npz").stat().st_size, "bytes")
